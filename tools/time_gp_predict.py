"""Device timing of the GP posterior (lfg_gp_predict, lfg_gp_predict_tree)
against the two ways to the same numbers without it (recorded, not
asserted).

    python tools/time_gp_predict.py [--out profiles/gp_predict/time_gp_predict.json]

Three steps, each a child process under its own time limit; nothing follows
a step that failed:
  gpu    HIP events around single launches, 5 warm-ups, the median of
         `--launches` (20):
           predict_4096     lfg_gp_predict, W = 4096 vectors, N = 300 data +
                            M = 300 test points, 2 blocks, mean and variance
           predict_4096_mean  the same, mean only
           predict_1        W = 1: the plotting call
           tree_1024        lfg_gp_predict_tree, the shipped GP example (6
                            eclipses, 1413 points), W = 1024 walkers
           lnprob_1024      lfg_lnprob alone on the same walkers: the part of
                            tree_1024 that is the tree's own front
  cpu    lfg_cpu_gp_predict (the same device text on the host, g++ -O3
         -march=native, 16 OpenMP threads) on predict_4096's inputs, the
         median of 5 calls; its results are compared with the GPU's
  dense  the dense numpy conditional (tests/gp_smoother.dense_predict) on 8 of
         those vectors, the median per vector, times 4096
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W_BIG, N, M = 4096, 300, 300


def inputs():
    import numpy as np
    rng = np.random.default_rng(0)
    x = np.sort(rng.uniform(-0.2, 0.3, N))
    t = np.linspace(-0.25, 0.35, M)
    ye = rng.uniform(0.003, 0.006, N)
    res = 0.004 * rng.standard_normal((W_BIG, N))
    hyp = np.stack([np.exp(rng.uniform(-11, -8, W_BIG)), np.exp(rng.uniform(-11, -8, W_BIG)),
                    np.exp(rng.uniform(-6.9, -2, W_BIG))], axis=1)
    d = rng.uniform(0.01, 0.05, W_BIG)
    blocks = np.stack([np.stack([-1 + d, -d], 1), np.stack([d, 1 - d], 1)], axis=1)
    return x, ye, res, hyp, blocks, t


def step_gpu(args):
    import ctypes
    import numpy as np
    import torch
    from lfit_python_amd import _native, batch, cvmodel, gp

    dev = torch.device("cuda", 0)
    L = _native.lib()
    _native.verify()
    vp = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = _native.stream_ptr(dev)

    def timed(launch):
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return {"median_us": 1e3 * statistics.median(ms), "min_us": 1e3 * min(ms), "max_us": 1e3 * max(ms)}

    x, ye, res, hyp, blocks, t = inputs()
    out = {}
    keep = None
    for name, W, want_var in (("predict_4096", W_BIG, True), ("predict_4096_mean", W_BIG, False),
                              ("predict_1", 1, True)):
        g = gp._Merged(x, ye, res[:W], hyp[:W], blocks[:W], t, dev)
        mean = torch.empty((W, g.n), dtype=torch.float64, device=dev)
        var = torch.empty((W, g.n), dtype=torch.float64, device=dev)
        nbytes = L.lfg_gp_predict_workspace_size(W, g.n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def launch():
            rc = L.lfg_gp_predict(*g.head(), vp(mean), vp(var) if want_var else None, vp(g.status), vp(ws), nbytes,
                                  stream)
            assert rc == 0
        out[name] = timed(launch)
        out[name].update(W=W, n=g.n, workspace_bytes=nbytes)
        assert int(g.status.abs().sum().item()) == 0
        if name == "predict_4096":
            keep = (mean[:, g.it_dev].cpu().numpy(), var[:, g.it_dev].cpu().numpy())
    np.savez(args.scratch, mean=keep[0], var=keep[1])

    m = cvmodel.construct_model(os.path.join(ROOT, "tests", "golden", "ref_test_data", "mcmc_input.dat"))
    tree = batch.compile_tree(m)
    ev = batch.LnProbEvaluator(tree, device=dev)
    W = 1024
    p0 = np.array(m.dynasty_par_vals)
    walkers = torch.as_tensor(p0 * (1.0 + 1e-4 * np.random.default_rng(1).standard_normal((W, p0.size))), device=dev)
    r = ev.predict(walkers)
    ok = int((r["status"] == 0).sum().item())
    nbytes = L.lfg_gp_predict_tree_workspace_size(W, ctypes.byref(ev.ctree))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def launch_tree():
        rc = L.lfg_gp_predict_tree(vp(walkers), W, ctypes.byref(ev.ctree), vp(r["flux"]), vp(r["gp_mean"]),
                                   vp(r["gp_var"]), vp(r["status"]), vp(ws), nbytes, stream)
        assert rc == 0
    out["tree_1024"] = timed(launch_tree)
    out["tree_1024"].update(W=W, E=tree.E, points=int(tree.offsets[-1]), walkers_with_a_posterior=ok,
                            workspace_bytes=nbytes, layout=L.lfg_version().decode())
    lnp = torch.empty(W, dtype=torch.float64, device=dev)
    out["lnprob_1024"] = timed(lambda: ev(walkers, out=lnp))
    return out


def step_cpu(args):
    import numpy as np
    from cpu_baseline import cpu
    from tests import gp_smoother as gs
    x, ye, res, hyp, blocks, t = inputs()
    lib = cpu.build(out=os.path.join(tempfile.gettempdir(), "liblfg_cpu_gp_%d.so" % os.getpid()), march="native")
    port = cpu.CpuPort(lib)
    os.remove(lib)  # loaded: the mapping stays
    xm, obs, ix, it = gs.merge(x, t)
    rm = np.zeros((W_BIG, xm.size))
    rm[:, ix] = res
    yem = np.zeros(xm.size)
    yem[ix] = ye
    sec = []
    for _ in range(6):
        t0 = time.perf_counter()
        mean, var, st = port.gp_predict(xm, yem, obs, rm, hyp, blocks, nthreads=16)
        sec.append(time.perf_counter() - t0)
    out = {"cpu_twin_16_threads": {"median_us": 1e6 * statistics.median(sec[1:]), "min_us": 1e6 * min(sec[1:]),
                                   "W": W_BIG}}
    if os.path.exists(args.scratch):
        g = np.load(args.scratch)
        s = (hyp[:, 0] + hyp[:, 1])[:, None]
        out["gpu_vs_cpu_twin"] = {"mean_err_of_scale": float(np.max(np.abs(g["mean"] - mean[:, it]) / np.sqrt(s))),
                                  "var_err_of_scale": float(np.max(np.abs(g["var"] - var[:, it]) / s))}
    return out


def step_dense(args):
    import numpy as np
    from tests import gp_smoother as gs
    x, ye, res, hyp, blocks, t = inputs()
    sec = []
    err = 0.0
    g = np.load(args.scratch) if os.path.exists(args.scratch) else None
    for w in range(8):
        t0 = time.perf_counter()
        mu, cov = gs.dense_predict(x, ye, res[w], *hyp[w], blocks[w], t)
        sec.append(time.perf_counter() - t0)
        if g is not None:
            err = max(err, float(np.max(np.abs(g["mean"][w] - mu)) / np.sqrt(hyp[w, 0] + hyp[w, 1])))
    per = statistics.median(sec)
    return {"dense_numpy": {"per_vector_us": 1e6 * per, "times_4096_us": 1e6 * per * W_BIG,
                            "note": "8 vectors measured, the median per vector scaled to 4096; full covariance"},
            "gpu_vs_dense_mean_err_of_scale": err if g is not None else None}


STEPS = {"gpu": (step_gpu, 600), "cpu": (step_cpu, 300), "dense": (step_dense, 120)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_predict", "time_gp_predict.json"))
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--scratch", default=os.path.join(tempfile.gettempdir(), "gp_predict_gpu_%d.npz" % os.getpid()))
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(STEPS[args.step][0](args)))
        return 0
    result = {}
    try:
        for name in ("gpu", "cpu", "dense"):
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--launches", str(args.launches),
                   "--scratch", args.scratch]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEPS[name][1])
            except subprocess.TimeoutExpired:
                print("step %s ran past its %d s: stopping" % (name, STEPS[name][1]))
                return 1
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                print("step %s failed with %d: stopping" % (name, p.returncode))
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            result.update(json.loads(line[7:]))
    finally:
        if os.path.exists(args.scratch):
            os.remove(args.scratch)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
