"""The measurements of profiles/chain_text/README.md: chain_prod.txt's rows
from the Python loop sampler.write_chain used to be, from the host twin, from
lfg_chain_text alone and from format_rows, and a production run's wall time
with either writer.

    python profiles/chain_text/bench_chain_text.py [--shapes 1000x1024x18,200x2048x156] [--loop-rows 50000]
                                                   [--run-steps 200] [--run-walkers 1024]

The chain is a random walk around one (17 significant digits in nearly every
value, as a real chain has), ln_prob a negative number of four digits.  HIP
events around lfg_chain_text, wall clock elsewhere; one warm-up and five
repeats, median (min - max).  Prints a table and one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def loop_write_chain(fname, names, chain, lnprob, mode="w"):
    """sampler.write_chain as it was before the bulk writer"""
    chain = np.asarray(chain)
    lnprob = np.asarray(lnprob)
    with open(fname, mode) as fh:
        if mode == "w":
            fh.write("walker_no " + " ".join(names) + " ln_prob\n")
        for s in range(chain.shape[0]):
            rows = ["{0:4d} {1:s} {2:f}\n".format(k, " ".join(map(repr, map(float, chain[s, k]))),
                                                 float(lnprob[s, k]))
                    for k in range(chain.shape[1])]
            fh.write("".join(rows))


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


def shape_rows(steps, W, ndim, loop_rows, tmp):
    import torch
    from lfit_python_amd import _native, chaintext
    rng = np.random.default_rng(5)
    chain = 1.0 + 1e-3 * rng.standard_normal((steps, W, ndim))
    lnp = -1e4 * rng.random((steps, W))
    rows = steps * W
    out = {"shape": [steps, W, ndim], "rows": rows}
    # the Python loop, on as many whole steps as make loop_rows rows
    ls = max(1, min(steps, loop_rows // W))
    f = os.path.join(tmp, "loop.txt")
    t = wall(lambda: loop_write_chain(f, ["p"] * ndim, chain[:ls], lnp[:ls]), repeats=3, warm=0)
    out["loop"] = {"rows": ls * W, "s": t, "bytes": os.path.getsize(f)}
    data = []
    t = wall(lambda: data.append(len(chaintext.format_rows(chain, lnp))), repeats=3)
    out["twin"] = {"rows": rows, "s": t, "bytes": data[-1], "loaded": chaintext.twin() is not None}
    dev = torch.device("cuda", torch.cuda.current_device())
    c, l = torch.as_tensor(chain).to(dev), torch.as_tensor(lnp).to(dev)
    L = _native.lib()
    bound = L.lfg_chain_text_bound(steps, W, ndim, 0)
    buf = torch.empty(bound, dtype=torch.uint8, device=dev)
    nb = torch.empty(2, dtype=torch.int64, device=dev)
    need = L.lfg_chain_text_workspace_size(steps, W, ndim)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = _native.stream_ptr(dev)

    def kernel():
        rc = L.lfg_chain_text(c.data_ptr(), steps, W, ndim, W * ndim, ndim, l.data_ptr(), W, 1, 0, buf.data_ptr(),
                              bound, nb.data_ptr(), ws.data_ptr(), need, st)
        assert rc == 0
    t = events(kernel)
    total, refused = nb.tolist()
    assert refused == 0 and total == data[-1]
    out["kernel"] = {"rows": rows, "s": t, "bytes": total, "bound": bound, "ws": need}
    t = wall(lambda: data.append(len(chaintext.format_rows(c, l))), repeats=5)
    assert data[-1] == total
    out["format_rows"] = {"rows": rows, "s": t, "bytes": total}
    return out


def production(steps, W, tmp):
    """run_mcmc_save's wall time, config 2's single eclipse, the same seed:
    the Python loop, the bulk writer on offloaded chunks (the default), and
    the bulk writer on chunks left on the device"""
    import torch
    from lfit_python_amd import batch, mcmc_utils, sampler, synthetic
    from lfit_python_amd.lfit import flux_batch

    def flux_fn(p, x, w, nsub):
        f, _ = flux_batch(np.asarray(p)[None, :], x, w, nsub=nsub)
        return f[0].cpu().numpy()
    m = synthetic.config_single(300, flux_fn=flux_fn)
    t = batch.compile_tree(m)
    ev = batch.LnProbEvaluator(t, max_walkers=W)
    p0 = np.array(m.dynasty_par_vals)
    init = sampler.initialise_walkers(p0, sampler.comp_scatter(m.dynasty_par_names, 0.1), W,
                                      lambda p: ev(torch.as_tensor(p, device="cuda")).cpu().numpy())
    names = "walker_no " + " ".join(m.dynasty_par_names) + " ln_prob"
    new_writer = sampler.write_chain
    out, files = {"steps": steps, "walkers": W, "ndim": t.ndim}, {}
    for label, writer, offload in (("loop", loop_write_chain, True), ("bulk_host", new_writer, True),
                                   ("bulk_device", new_writer, False), ("no_file", None, True)):
        times = []
        for rep in range(2):
            S = sampler.EnsembleSampler(W, t.ndim, ev, seed=11)
            S.offload = offload
            if writer is loop_write_chain:   # (the loop takes arrays, as its callers gave it)
                sampler.write_chain = lambda f, n, c, l, mode="w": loop_write_chain(f, n, c.cpu().numpy(),
                                                                                    l.cpu().numpy(), mode)
            else:
                sampler.write_chain = new_writer
            f = os.path.join(tmp, label + ".txt") if writer else None
            torch.cuda.synchronize()
            a = time.perf_counter()
            mcmc_utils.run_mcmc_save(S, init, steps, None, f, col_names=names)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - a)
        sampler.write_chain = new_writer
        out[label] = times
        if f:
            files[label] = open(f, "rb").read()
    out["files_equal"] = len(set(files.values())) == 1
    out["file_bytes"] = len(files["loop"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x1024x18,200x2048x156")
    ap.add_argument("--loop-rows", type=int, default=50000)
    ap.add_argument("--run-steps", type=int, default=200)
    ap.add_argument("--run-walkers", type=int, default=1024)
    args = ap.parse_args(argv)
    res = {"shapes": [], "cpus": os.cpu_count(), "omp": os.environ.get("OMP_NUM_THREADS")}
    with tempfile.TemporaryDirectory() as tmp:
        for s in args.shapes.split(","):
            r = shape_rows(*(int(v) for v in s.split("x")), args.loop_rows, tmp)
            res["shapes"].append(r)
            print("%s: %d rows" % (s, r["rows"]))
            for k in ("loop", "twin", "kernel", "format_rows"):
                e = r[k]
                med = e["s"][0]
                print("  %-12s %10.4f s (%.4f - %.4f)  %12.0f rows/s  %8.1f MB/s" % (
                    k, med, e["s"][1], e["s"][2], e["rows"] / med, e["bytes"] / med / 1e6))
        if args.run_steps:
            res["production"] = production(args.run_steps, args.run_walkers, tmp)
            print("run_mcmc_save:", {k: v for k, v in res["production"].items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
