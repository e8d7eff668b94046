"""The measurements of profiles/chain_parse/README.md: chain_prod.txt's numbers
read back by np.loadtxt (sampler.read_chain as it was), by the host twin, by
the two device calls alone and by chainparse.read_chain end to end, and
fit_summary's wall time with either reader.

    python profiles/chain_parse/bench_chain_parse.py [--shapes 1000x1024x18,200x2048x156] [--loadtxt-rows 49152]
                                                     [--summary-steps 100] [--summary-walkers 1024]

The text is write_chain's for a random walk around one (17 significant digits
in nearly every value, as a real chain has) and a ln_prob of four integer
digits.  HIP events around lfg_chain_parse_count and lfg_chain_parse, wall
clock elsewhere; one warm-up, median (min - max).  Prints a table and one JSON
line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def loadtxt_read_chain(fname):
    """sampler.read_chain as it was before the bulk reader"""
    data = np.loadtxt(fname, skiprows=1)
    nw = int(data[:, 0].max()) + 1
    ns = data.shape[0] // nw
    chain = np.full((nw, ns, data.shape[1] - 1), np.nan)
    for i in range(nw):
        chain[i] = data[data[:, 0] == i, 1:]
    return chain


def wall(fn, repeats=5, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(repeats):
        a = time.perf_counter()
        fn()
        t.append(time.perf_counter() - a)
    return float(np.median(t)), float(min(t)), float(max(t))


def events(fn, repeats=5):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def shape_rows(steps, W, ndim, loadtxt_rows, tmp):
    import torch
    from lfit_python_amd import _native, chainparse, sampler
    rng = np.random.default_rng(5)
    dev = torch.device("cuda", torch.cuda.current_device())
    chain = torch.as_tensor(1.0 + 1e-3 * rng.standard_normal((steps, W, ndim))).to(dev)
    lnp = torch.as_tensor(-1e4 * rng.random((steps, W))).to(dev)
    names = ["p%d" % i for i in range(ndim)]
    full = os.path.join(tmp, "chain_prod.txt")
    sampler.write_chain(full, names, chain, lnp)
    rows, ncol = steps * W, ndim + 2
    out = {"shape": [steps, W, ndim], "rows": rows, "bytes": os.path.getsize(full)}
    # the parent's reader, on as many whole steps as make loadtxt_rows rows
    ls = max(1, min(steps, loadtxt_rows // W))
    part = os.path.join(tmp, "part.txt")
    sampler.write_chain(part, names, chain[:ls], lnp[:ls])
    want = []
    t = wall(lambda: want.append(loadtxt_read_chain(part)), repeats=3, warm=0)
    out["loadtxt"] = {"rows": ls * W, "s": t, "bytes": os.path.getsize(part)}
    got = sampler.read_chain(part)
    assert got.tobytes() == want[-1].tobytes()
    # the file's bytes and the twin
    raw = []
    t = wall(lambda: raw.append(np.fromfile(full, dtype=np.uint8)), repeats=3)
    out["fromfile"] = {"rows": rows, "s": t, "bytes": out["bytes"]}
    a = raw[-1]
    del raw[:]
    off = int(np.flatnonzero(a[:1 << 16] == 10)[0]) + 1
    body = a[off:]
    host = []
    t = wall(lambda: (host.clear(), host.append(chainparse.parse_host(body, ncol)[0])), repeats=3)
    out["twin"] = {"rows": rows, "s": t, "bytes": int(body.size), "loaded": chainparse.twin() is not None}
    assert host[0].shape == (rows, ncol)
    assert host[0].reshape(steps, W, ncol)[:, :, 1:-1].tobytes() == chain.cpu().numpy().tobytes()
    # the copy and the two device calls
    text = []
    t = wall(lambda: (text.clear(), text.append(torch.from_numpy(body).to(dev)), torch.cuda.synchronize()), repeats=3)
    out["copy"] = {"rows": rows, "s": t, "bytes": int(body.size)}
    text = text[0]
    L = _native.lib()
    n = int(text.numel())
    need = L.lfg_chain_parse_workspace_size(n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    info = torch.empty(8, dtype=torch.int64, device=dev)
    vals = torch.empty((rows, ncol), dtype=torch.float64, device=dev)
    st = _native.stream_ptr(dev)

    def count():
        assert L.lfg_chain_parse_count(text.data_ptr(), n, ncol, info.data_ptr(), ws.data_ptr(), need, st) == 0

    def parse():
        assert L.lfg_chain_parse(text.data_ptr(), n, ncol, vals.data_ptr(), rows, info.data_ptr(), ws.data_ptr(),
                                 need, st) == 0
    out["count"] = {"rows": rows, "s": events(count), "bytes": n}
    out["parse"] = {"rows": rows, "s": events(parse), "bytes": n}
    out["kernels"] = {"rows": rows, "s": events(lambda: (count(), parse())), "bytes": n, "ws": need}
    assert info.tolist() == [rows, rows * ncol, 0, 0, 0, -1, 0, 0]
    assert torch.equal(vals.view(steps, W, ncol)[:, :, 1:-1], chain)
    del vals, ws, text, host
    # end to end from the file
    seen = []
    t = wall(lambda: (seen.clear(), seen.append(chainparse.read_chain(full, device=dev)[0]), torch.cuda.synchronize()),
             repeats=3)
    out["read_chain"] = {"rows": rows, "s": t, "bytes": out["bytes"]}
    assert torch.equal(seen[0][:, :, :-1], chain)
    t = wall(lambda: (seen.clear(), seen.append(sampler.read_chain(full))), repeats=3)
    out["read_chain_host"] = {"rows": rows, "s": t, "bytes": out["bytes"]}
    return out


def summary(steps, W, tmp):
    """python -m lfit_python_amd.fit_summary's main() on the golden input:
    the parent's reader (np.loadtxt, walker-major) against the device reader
    and the host twin's"""
    import contextlib
    import io
    import torch
    from lfit_python_amd import chainparse, cvmodel, fit_summary, sampler
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    golden = os.path.join(root, "tests", "golden", "ref_test_data", "mcmc_input.dat")
    model = cvmodel.construct_model(golden)
    names = list(model.dynasty_par_names)
    rng = np.random.default_rng(13)
    x = np.array(model.dynasty_par_vals) * (1.0 + 1e-3 * rng.normal(size=(steps, W, len(names))))
    path = os.path.join(tmp, "summary_chain.txt")
    sampler.write_chain(path, names, x, -1e3 * rng.random((steps, W)))
    out = {"steps": steps, "walkers": W, "ndim": len(names), "bytes": os.path.getsize(path)}
    new_reader = sampler.read_chain
    files = {}
    for label, route, reader in (("parent", False, loadtxt_read_chain), ("twin", False, new_reader),
                                 ("device", True, new_reader)):
        chainparse.DEVICE_ROUTE, sampler.read_chain = route, reader
        times = []
        for rep in range(3):
            d = os.path.join(tmp, "%s%d" % (label, rep))
            os.makedirs(d)
            torch.cuda.synchronize()
            a = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                fit_summary.main([path, golden, "--dir", d])
            torch.cuda.synchronize()
            times.append(time.perf_counter() - a)
        out[label] = times
        files[label] = open(os.path.join(d, "modparams.csv"), "rb").read()
    chainparse.DEVICE_ROUTE, sampler.read_chain = True, new_reader
    out["files_equal"] = len(set(files.values())) == 1
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x1024x18,200x2048x156")
    ap.add_argument("--loadtxt-rows", type=int, default=49152)
    ap.add_argument("--summary-steps", type=int, default=100)
    ap.add_argument("--summary-walkers", type=int, default=1024)
    args = ap.parse_args(argv)
    res = {"shapes": [], "cpus": os.cpu_count(), "omp": os.environ.get("OMP_NUM_THREADS")}
    with tempfile.TemporaryDirectory() as tmp:
        for s in args.shapes.split(","):
            r = shape_rows(*(int(v) for v in s.split("x")), args.loadtxt_rows, tmp)
            res["shapes"].append(r)
            print("%s: %d rows, %d bytes" % (s, r["rows"], r["bytes"]), flush=True)
            for k in ("loadtxt", "fromfile", "twin", "copy", "count", "parse", "kernels", "read_chain",
                      "read_chain_host"):
                e = r[k]
                med = e["s"][0]
                print("  %-16s %10.5f s (%.5f - %.5f)  %12.0f rows/s  %9.1f MB/s" % (
                    k, med, e["s"][1], e["s"][2], e["rows"] / med, e["bytes"] / med / 1e6), flush=True)
        if args.summary_steps:
            res["summary"] = summary(args.summary_steps, args.summary_walkers, tmp)
            print("fit_summary:", res["summary"], flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
