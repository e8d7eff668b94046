#!/usr/bin/env python3
"""Rows per second of lfg_physpar on the GPU, of its host twin and of the
numpy / scipy double (report only: profiles/physpar/README.md).

    python tools/physpar_bench.py [--rows 4194304] [--repeats 11] [--out FILE.md]

Two clouds of 2^22 rows:
  posterior   normals around the shipped example's fitted q = 0.1037,
              dphi = 0.0392, rwd = 0.0187 (2 %, 0.5 % and 4 % wide), with
              twd = 15 000 +/- 500 K and p = 0.07 +/- 1e-5 d: one branch
  mixed       the fixed batch of tests/physpar_double.py tiled: every branch
              and status, lanes of a wave in different models
GPU: tables resident, inputs and outputs resident and allocated beforehand,
three warm-up launches, then `repeats` launches each between two HIP events;
the median and the spread (min, max) are reported.  A run without a GPU
fails.  The host twin runs on 16 threads (median of 3), the double on one core
over 512 rows of the cloud.  The branch populations of each cloud come from
the GPU's own model / status output.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds(rows, oracle):
    from tests import physpar_double as ppd
    rng = np.random.default_rng(2)
    post = {"q": rng.normal(0.1037, 0.02 * 0.1037, rows), "dphi": rng.normal(0.0392, 0.005 * 0.0392, rows),
            "rw": rng.normal(0.0187, 0.04 * 0.0187, rows), "T": rng.normal(15000.0, 500.0, rows),
            "P": rng.normal(0.07, 1e-5, rows)}
    b = ppd.fixed_batch(oracle)
    reps = -(-rows // len(b["q"]))
    mixed = {k: np.tile(b[k], reps)[:rows] for k in ("q", "dphi", "rw", "T", "P")}
    return {"posterior": post, "mixed": mixed}


def main():
    import torch
    from cpu_baseline import cpu
    from lfit_python_amd import _native, physpar
    from oracle.oracle import Oracle
    from tests import physpar_double as ppd
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--dir", default=ppd.WD_MODELS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _native.require_gpu()
    _native.verify()
    dev = torch.device("cuda", 0)
    oracle = Oracle()
    tables = physpar.load_mr_tables(args.dir)
    tables.device_struct(dev)
    port = cpu.CpuPort()
    D = ppd.Double(args.dir, oracle.xl1, oracle.findi)
    n = args.rows
    lines = ["| cloud | rows | GPU ms (median, min - max of %d) | GPU rows/s | host twin, 16 threads rows/s | "
             "numpy double, 1 core rows/s | wood / panei / hamada / no solution / other status |" % args.repeats,
             "|---|---|---|---|---|---|---|"]
    for name, c in clouds(n, oracle).items():
        t = {k: torch.as_tensor(v, device=dev) for k, v in c.items()}
        out = torch.empty((10, n), dtype=torch.float64, device=dev)
        model = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)

        def launch():
            physpar._launch(t["q"], t["dphi"], t["rw"], 1, t["T"], t["P"], n, tables, out, model, status, dev)
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        mo, st = model.cpu().numpy(), status.cpu().numpy()
        pops = [np.mean(mo == k) for k in (0, 1, 2)] + [np.mean(st == 6), np.mean((st != 0) & (st != 6))]
        tw = []
        for _ in range(3):
            t0 = time.perf_counter()
            port.physpar(c["q"], c["dphi"], c["rw"], c["T"], c["P"], tables, nthreads=16)
            tw.append(time.perf_counter() - t0)
        k = 512
        t0 = time.perf_counter()
        D.run({key: v[:k] for key, v in c.items()}, tight=False)
        dbl = time.perf_counter() - t0
        lines.append("| %s | %d | %.3f (%.3f - %.3f) | %.3e | %.3e | %.3e | %s |" % (
            name, n, med, min(ms), max(ms), n / (med * 1e-3), n / statistics.median(tw), k / dbl,
            " / ".join("%.1f %%" % (100 * p) for p in pops)))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
