"""The measurements of profiles/corner/README.md: lfg_corner_hist and
lfg_corner_levels on a spread and on a collapsed posterior, and the host
route they replace.

    python profiles/corner/bench_corner.py [--steps 611] [--walkers 16384] [--k 18] [--bins 50] [--host-rows 1000000]

HIP events around each call, one warm-up and five repeats, median (min - max).
Prints a table and one JSON line.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def timed(fn, repeats=5):
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
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=611)
    ap.add_argument("--walkers", type=int, default=16384)
    ap.add_argument("--k", type=int, default=18)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--host-rows", type=int, default=1000000)
    args = ap.parse_args(argv)
    import torch
    from lfit_python_amd import _native, chainstats, corner
    L = _native.lib()
    K, nb, steps, W = args.k, args.bins, args.steps, args.walkers
    rows, P = steps * W, args.k * (args.k - 1) // 2
    dev = torch.device("cuda", torch.cuda.current_device())
    fr = np.array(corner.DEFAULT_LEVELS)
    cols = (ctypes.c_int * K)(*range(K))
    h1 = torch.empty((K, nb), dtype=torch.int64, device=dev)
    h2 = torch.empty((P, nb, nb), dtype=torch.int64, device=dev)
    flag = torch.empty(K, dtype=torch.int32, device=dev)
    lev = torch.empty((P, fr.size), dtype=torch.int64, device=dev)
    nbytes = L.lfg_corner_workspace_size(steps, W, K, nb)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    st = _native.stream_ptr(dev)
    tile = L.lfg_corner_pair_tile(nb)
    ntile = max(1, -(-P // tile))
    read = ntile * rows * K * 8
    out = {"rows": rows, "K": K, "bins": nb, "pairs": P, "pair_tile": tile, "pair_tiles": ntile,
           "chain_GB": rows * K * 8 / 1e9, "read_GB_per_call": read / 1e9}

    def hist(chain, rng):
        def go():
            rc = L.lfg_corner_hist(ctypes.c_void_p(chain.data_ptr()), steps, W, K, W * K, K, cols, K,
                                   ctypes.c_void_p(rng.data_ptr()), nb, ctypes.c_void_p(h1.data_ptr()),
                                   ctypes.c_void_p(h2.data_ptr()), ctypes.c_void_p(flag.data_ptr()),
                                   ctypes.c_void_p(ws.data_ptr()), nbytes, st)
            assert rc == 0
        return go

    def levels():
        rc = L.lfg_corner_levels(ctypes.c_void_p(h2.data_ptr()), P, nb, fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 fr.size, ctypes.c_void_p(lev.data_ptr()), st)
        assert rc == 0

    # (a) a spread cloud: correlated normals, the range from the device's min and max
    torch.manual_seed(1)
    chain = torch.randn((steps, W, K), dtype=torch.float64, device=dev)
    chain[:, :, 1:] += 0.5 * chain[:, :, :-1]
    v = chainstats._View(chain)
    r = chainstats._run(v, np.empty(0))
    rng = torch.stack([r["min"], r["max"]], dim=1).contiguous()
    out["a_hist_ms"] = timed(hist(chain, rng))
    out["a_levels_ms"] = timed(levels)
    out["a_GBps"] = read / 1e9 / (out["a_hist_ms"][0] / 1e3)
    assert int(h2[0].sum()) == rows and int(h1.sum()) == rows * K
    out["a_range_ms"] = timed(lambda: chainstats._run(v, np.empty(0)))
    # the sweep lfg_chain.hip's k_hist makes over the same rows, for comparison: 8 radix passes
    with_q = timed(lambda: chainstats._run(v, np.array([0.5])))
    out["chain_k_hist_pass_ms"] = (with_q[0] - out["a_range_ms"][0]) / 8.0
    out["chain_k_hist_GBps"] = rows * K * 8 / 1e9 / (out["chain_k_hist_pass_ms"] / 1e3)

    # (c) the host route on the same data: the copy, then np.histogram2d over the pairs of host_rows rows
    t0 = time.perf_counter()
    host = chain.cpu().numpy()
    out["c_copy_s"] = time.perf_counter() - t0
    flat = host.reshape(-1, K)[: args.host_rows]
    lohi = rng.cpu().numpy()
    t0 = time.perf_counter()
    for a in range(K):
        for b in range(a + 1, K):
            np.histogram2d(flat[:, a], flat[:, b], bins=nb, range=(tuple(lohi[a]), tuple(lohi[b])))
    out["c_hist2d_s"], out["c_rows"] = time.perf_counter() - t0, int(flat.shape[0])
    if flat.shape[0] == rows:   # (the whole chain on the host: the counts must be the device's)
        assert np.array_equal(np.histogram2d(flat[:, 0], flat[:, 1], bins=nb, range=(tuple(lohi[0]), tuple(lohi[1])))[0],
                              h2[0].cpu().numpy())
    del host, flat

    # (b) every row in one bin
    chain.fill_(0.25)
    one = torch.tensor([[0.0, 1.0]] * K, dtype=torch.float64, device=dev)
    out["b_hist_ms"] = timed(hist(chain, one))
    out["b_levels_ms"] = timed(levels)
    assert int(h2[-1, nb // 4, nb // 4]) == rows
    out["b_over_a"] = out["b_hist_ms"][0] / out["a_hist_ms"][0]

    def f(t):
        return "%.3f (%.3f - %.3f)" % t
    print("rows %d, K %d, bins %d: %d pairs in %d tiles of %d; chain %.2f GB, read %.2f GB per call" %
          (rows, K, nb, P, ntile, tile, out["chain_GB"], out["read_GB_per_call"]))
    print("(a) spread     lfg_corner_hist %s ms = %.0f GB/s; lfg_corner_levels %s ms; min/max sweep %s ms" %
          (f(out["a_hist_ms"]), out["a_GBps"], f(out["a_levels_ms"]), f(out["a_range_ms"])))
    print("    lfg_chain's radix pass on the same rows: %.3f ms = %.0f GB/s" %
          (out["chain_k_hist_pass_ms"], out["chain_k_hist_GBps"]))
    print("(b) one bin    lfg_corner_hist %s ms = %.2f x (a); lfg_corner_levels %s ms" %
          (f(out["b_hist_ms"]), out["b_over_a"], f(out["b_levels_ms"])))
    print("(c) host       copy of the chain %.3f s; np.histogram2d over %d pairs of %d rows %.3f s" %
          (out["c_copy_s"], P, out["c_rows"], out["c_hist2d_s"]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
