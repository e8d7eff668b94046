"""Diagnostic: why LONG points are not quiet (sub_point_quiet) at config 5,
or on a case of tests/test_gpu_long_edges.py.
Needs a build with -DLFG_COUNT_ITERS -DLFG_COUNT_QUIET (tools/build_exp.sh),
loaded with LFG_DIAGNOSTIC=1 LFG_LIB=...

    python tools/quiet_count.py [walkers] [points] [sub-bins]
    python tools/quiet_count.py <case>      (spot_dense, beam_dark, wrap_sub, ...:
                                             one evaluation of the test's 48 walkers)
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lfit_python_amd import _native, batch, sampler, synthetic  # noqa: E402
from lfit_python_amd.lfit import flux_batch  # noqa: E402

dev = torch.device("cuda", 0)
CASE = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else None
W = int(sys.argv[1]) if len(sys.argv) > 1 and not CASE else 1024
NPTS = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
NSUB = int(sys.argv[3]) if len(sys.argv) > 3 else 5
L = _native.lib()
c = (ctypes.c_ulonglong * 64)()


def flux_fn(pars, x, w, nsub):
    f, st = flux_batch(np.asarray(pars)[None, :], x, w, nsub=nsub, device=dev)
    return f[0].cpu().numpy()


if CASE:
    from oracle.oracle import Oracle
    from tests.test_gpu_long_edges import build_case, case_walkers
    model, NSUB = build_case(Oracle(), CASE)
    tree = batch.compile_tree(model, nsub=NSUB)
    walk = case_walkers(model)
    ev = batch.LnProbEvaluator(tree, device=dev, max_walkers=len(walk))
    L.lfg_diag_iters(c)  # clear
    lnp = ev(torch.as_tensor(walk, device=dev))
    torch.cuda.synchronize()
    print("%s: %d points, S = %d, %d walkers (%d finite)" % (CASE, tree.max_n, NSUB, len(walk),
                                                              int(torch.isfinite(lnp).sum())))
else:
    model = synthetic.config_single(npts=NPTS, flux_fn=flux_fn, nsub=NSUB)
    tree = batch.compile_tree(model, nsub=NSUB)
    ev = batch.LnProbEvaluator(tree, device=dev, max_walkers=W)
    p0 = np.array(model.dynasty_par_vals)
    init = sampler.initialise_walkers(p0, sampler.comp_scatter(model.dynasty_par_names, 0.1), W,
                                      lambda p: ev(torch.as_tensor(p, device=dev)).cpu().numpy(), seed=5)
    S = sampler.EnsembleSampler(W, tree.ndim, ev, seed=5)
    S.set_state(init)
    S.step()
    L.lfg_diag_iters(c)  # clear
    for _ in range(3):
        S.step()
    torch.cuda.synchronize()
L.lfg_diag_iters(c)
v = np.array(c[56:63], dtype=np.float64)
names = ["points", "zero/NaN width", "wraps", "spot hull", "beaming sign change", "donor entry inside", "quiet"]
for n, x in zip(names, v):
    print("%-22s %12d  (%.1f %%)" % (n, x, 100.0 * x / max(v[0], 1)))
if CASE:
    # the same windows by tests/long_windows.py's classes, summed over the
    # walkers (it tests the spot's entries before the beaming zeros and the
    # donor; the kernel's in-hull entry test, counted as "spot hull", comes last)
    from tests import long_windows
    leaf = model.leaves()[0]
    keys = ("zero", "wrap", "spot_edge", "beam_cross", "donor", "quiet", "borderline", "quiet_offspot",
            "quiet_partial", "quiet_full", "quiet_lit", "quiet_dark")
    tot, npt = dict.fromkeys(keys, 0), 0
    for k in np.flatnonzero(torch.isfinite(lnp).cpu().numpy()):
        model.dynasty_par_vals = walk[k]
        cl = long_windows.classify(Oracle(), np.array(leaf.cv_parlist), leaf.lc.x, leaf.lc.w, NSUB)
        npt += leaf.lc.x.size
        for key in keys:
            tot[key] += int(cl[key].sum())
    print("classifier, the %d points of the walkers with a finite ln_prob:" % npt)
    for key in keys:
        print("%-22s %12d  (%.1f %%)" % (key, tot[key], 100.0 * tot[key] / max(npt, 1)))
