#!/usr/bin/env python3
"""Rows per second of lfg_limbdark on the GPU and of its host twin (report
only: profiles/limbdark/README.md; nothing is asserted).

    python tools/ld_profile.py [--out profiles/limbdark/README.md] [--resources FILE] [--note FILE]

Two clouds at 10^4, 10^6 and 10^7 rows:
  posterior   normals about logg = 8.1 +/- 0.05, teff = 14 300 +/- 300 K, what
              a white-dwarf chain looks like: the lanes of a wave read one or
              two cells of the tables
  scattered   uniform over [4.5, 10] x [3000, 35000]: every lane in a cell of
              its own, a third of the rows clamped
GPU: tables resident, inputs and outputs resident and allocated beforehand,
five warm-up launches per shape, then nine blocks of back-to-back launches,
each block between two HIP events and long enough to take tens of
milliseconds; the per-launch time of a block is its time over its launches,
and the median and the spread (min, max) of the nine are reported.  The
implied store bandwidth is 200 bytes per row over that time, against the
8.0 TB/s HBM3E peak and the 6.3 TB/s a copy reaches.  A run without a GPU
fails.  The host twin runs 10^6 rows on 16 threads (median of 3).  The
kernel's resource figures come from the compiler's kernel-resource-usage
remarks (tools/kernel_resources.sh prints the same), or from --resources.
--note appends a file (what bounds the kernel, from a counter run of its own).
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((10 ** 4, 400), (10 ** 6, 100), (10 ** 7, 20))     # rows, launches per timed block
BLOCKS = 9
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12
ROW_BYTES = 200


def cloud(name, n, rng):
    if name == "posterior":
        return rng.normal(8.1, 0.05, n), rng.normal(14300.0, 300.0, n)
    return rng.uniform(4.5, 10.0, n), rng.uniform(3000.0, 35000.0, n)


def resources():
    """the compiler's remarks for lfg_limbdark.hip's kernels"""
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
           "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage",
           os.path.join(ROOT, "lfit_python_amd", "csrc", "lfg_limbdark.hip")]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    keep = re.findall(r"remark: +((?:Function Name|VGPRs|AGPRs|ScratchSize|Occupancy|LDS Size|TotalSGPRs|"
                      r"SGPRs Spill|VGPRs Spill)[^\n]*?) *\[-Rpass-analysis", err)
    return "\n".join(k.strip() for k in keep)


def main():
    import torch
    from cpu_baseline import cpu
    from lfit_python_amd import _native, limbdark
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=os.path.join(ROOT, "tests", "golden", "ld_coeffs"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None, help="a file with the kernel's resource figures (default: compile)")
    ap.add_argument("--note", default=None, help="a file appended to the report")
    args = ap.parse_args()
    _native.require_gpu()
    _native.verify()
    dev = torch.device("cuda", 0)
    tables = limbdark.load_ld_tables(args.dir)
    tables.device_struct(dev)
    rng = np.random.default_rng(5)
    lines = ["| cloud | rows | launches per block | ms per launch (median, min - max of %d blocks) | rows/s | "
             "store bandwidth | of the 8.0 TB/s peak | of the 6.3 TB/s a copy reaches | clamped |" % BLOCKS,
             "|---|---|---|---|---|---|---|---|---|"]
    host = {}
    for name in ("posterior", "scattered"):
        for n, launches in SIZES:
            g, t = cloud(name, n, rng)
            lg, tf = torch.as_tensor(g, device=dev), torch.as_tensor(t, device=dev)
            out = torch.empty((n, 25), dtype=torch.float64, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)

            def launch():
                limbdark._launch(lg, tf, 1, n, tables, out, status, dev)
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            ms = []
            for _ in range(BLOCKS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    launch()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / launches)
            med = statistics.median(ms)
            bw = n * ROW_BYTES / (med * 1e-3)
            clamped = float((status == limbdark.ST_CLAMPED).double().mean())
            lines.append("| %s | %d | %d | %.4f (%.4f - %.4f) | %.3e | %.3f TB/s | %.1f %% | %.1f %% | %.1f %% |" % (
                name, n, launches, med, min(ms), max(ms), n / (med * 1e-3), bw / 1e12, 100 * bw / HBM_PEAK,
                100 * bw / HBM_COPY, 100 * clamped))
            print(lines[-1], flush=True)
            if n == 10 ** 6:
                port = cpu.CpuPort()
                tw = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    port.limbdark(g, t, tables, nthreads=16)
                    tw.append(time.perf_counter() - t0)
                host[name] = n / statistics.median(tw)
            del lg, tf, out, status
    text = "# lfg_limbdark on an MI355X\n\nWritten by `tools/ld_profile.py` (its docstring says how each number is taken).\n\n"
    text += "\n".join(lines) + "\n\n"
    text += "Host twin (`lfg_cpu_limbdark`, 16 threads, 10^6 rows, median of 3): " + ", ".join(
        "%s %.3e rows/s" % (k, v) for k, v in host.items()) + ".\n\n"
    res = open(args.resources).read().strip() if args.resources else resources()
    text += "Kernel resources (gfx950, the compiler's remarks; the LDS is dynamic: 151 480 bytes on the shipped " \
            "tables, knots + tile + 25 surfaces):\n\n```\n" + res + "\n```\n"
    if args.note:
        text += "\n" + open(args.note).read()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
