#!/usr/bin/env python3
"""Timings of the white-dwarf atmosphere fit (report only; bench.py is the
project's benchmark and does not know this workload).

    python tools/wd_bench.py [--out FILE.json]

On one GPU, timed with HIP events after a warm-up, median and spread
(min .. max) of 11 repeats; a repeat is a window of 400 calls or 5000 sampler
steps (a tenth of a second or more), and the sampler paths take turns
inside every repeat:
  lnprob     lfg_wd_lnprob over 2^22 rows, rows/s
  fused      EnsembleSampler steps/s at W = 200 through lfg_wd_step_half
  three      the same through propose -> lfg_wd_lnprob -> accept
  graph      the same three launches replayed as a HIP graph
and on the host: lfg_cpu_wd_lnprob on 16 threads and the scipy double of
tests/wd_double.py on one core, rows/s.  The model is the tests' own: five
bands, g and r colour-corrected, the shipped input's priors.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 11


def stats(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return {"median": float(np.median(v)), "min": float(v[0]), "max": float(v[-1])}


def gpu_time(fn, repeats=REPEATS, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def main():
    import torch
    from cpu_baseline import cpu
    from lfit_python_amd import sampler, wdparams
    from tests import wd_double as wdd
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=5000, help="sampler steps per timed window")
    ap.add_argument("--calls", type=int, default=400, help="lfg_wd_lnprob calls per timed window")
    args = ap.parse_args()

    model = wdd.build_model("A", True)
    ev = wdparams.WDEvaluator(model)
    rng = np.random.default_rng(1)
    n = args.rows
    theta = np.column_stack([rng.uniform(5500, 80000, n), rng.uniform(7.1, 9.4, n), rng.uniform(1.5, 3.3, n),
                             rng.uniform(0.0005, 0.013, n)])
    x = torch.as_tensor(theta, device=ev.device)
    out = torch.empty(n, dtype=torch.float64, device=ev.device)
    res = {"rows": n, "steps": args.steps, "W": 200, "device": torch.cuda.get_device_name(ev.device)}

    def calls():
        for _ in range(args.calls):
            ev(x, out=out)
    t = gpu_time(calls, warm=1)
    res["lnprob_rows_per_s"] = stats([n * args.calls / s for s in t])

    # the three sampler paths take turns inside every repeat
    W = 200
    f = lambda p: ev(torch.as_tensor(p, dtype=torch.float64, device=ev.device)).cpu().numpy()
    p0 = sampler.initialise_walkers(np.array([13000.0, 8.2, 2.4, 0.006]), 0.05, W, f, seed=1)
    paths = {}
    for name in ("fused", "three", "graph"):
        S = sampler.EnsembleSampler(W, 4, ev, seed=3)
        S.fuse = name == "fused"
        S.use_graph = name == "graph"
        S.set_state(p0)
        for _ in range(50):
            S.step()
        paths[name] = S
    times = {name: [] for name in paths}
    for _ in range(REPEATS):
        for name, S in paths.items():
            def run():
                for _ in range(args.steps):
                    S.step()
            times[name] += gpu_time(run, repeats=1, warm=0)
    for name, t in times.items():
        res[name + "_steps_per_s"] = stats([args.steps / s for s in t])

    if not os.path.exists(cpu.LIB_PATH):
        cpu.build()
    P = cpu.CpuPort()
    m = min(n, 1 << 20)
    t = []
    for _ in range(REPEATS + 1):
        t0 = time.perf_counter()
        P.wd_lnprob(theta[:m], model, nthreads=16)
        t.append(time.perf_counter() - t0)
    res["twin_16_threads_rows_per_s"] = stats([m / s for s in t[1:]])
    D = wdd.Double("A", True)
    k = 20000
    t = []
    for _ in range(REPEATS + 1):
        t0 = time.perf_counter()
        D.run(theta[:k])
        t.append(time.perf_counter() - t0)
    res["scipy_double_one_core_rows_per_s"] = stats([k / s for s in t[1:]])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
