"""GPU: k_pair's likelihood phase with the run scan (LFG_PAIR_RUNSCAN) against
the oracle.

After the phase barrier wave i < 6 scans difference array i in place, lane l
owning the run [l R, min((l + 1) R, m)) with R = ceil(m / 64), and a wave whose
first thread lies past the last point does nothing but reach the barriers
(lfg_k_lnlike.hpp: run_scan; lfg_k_pair.hpp: k_pair).  The point counts below are where that code
changes its shape:

    n = 2            R = 1, 62 empty lanes, seven idle waves
    n = 63, 64, 65   the first wave boundary; 65: R = 2 and a short last run
    n = 300          config 2: R = 5, waves 5-7 idle
    n = 448, 449     R = 7 -> 8; wave 7 (the housekeeping wave) gains a point
    n = 511, 512     a short last lane; the full tile, no idle wave

Each case: 8 walkers from the 1 % ball, ln_prob and the per-eclipse ln_like
through lfg_lnprob on both kernel layouts (the two-kernel layout keeps
block_scan), against oracle.lnprob_batch at LNP_RTOL.  The reference of a case
is computed once and shared by the layouts."""
import numpy as np
import pytest

from tests.test_gpu_lnprob import LAYOUTS, LNP_RTOL, _same, layout  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

W = 8
SIZES = [2, 63, 64, 65, 300, 448, 449, 511, 512]
RAGGED = (65, 300, 512)
_CASES = {}


def _set_lc(leaf, x, w, oracle, rng):
    from lfit_python_amd.synthetic import NOISE
    leaf.lc.x, leaf.lc.w = x, w
    leaf.lc.ye = NOISE * np.ones_like(x)
    st, f = oracle.flux(leaf.cv_parlist, x, w)
    assert st == 0
    leaf.lc.y = f + NOISE * rng.standard_normal(f.shape)


def _build(key, oracle):
    """(tree, walkers, rejected mask, oracle ln_prob, oracle ln_like per eclipse) of a case"""
    from lfit_python_amd import batch, synthetic
    from lfit_python_amd.synthetic import phase_grid
    kind, n = key
    rng = np.random.default_rng(3)
    if kind == "ragged":
        m = synthetic.config_tree(1, 300)      # 3 bands x 1 eclipse
        for lf, k in zip(m.leaves(), RAGGED):
            _set_lc(lf, *phase_grid(k), oracle, rng)
    else:
        m = synthetic.config_single(300)
        x, w = phase_grid(n)
        if kind == "shuffled":                 # a file in arbitrary order: the tile goes point-major
            p = np.random.default_rng(17).permutation(n)
            x, w = x[p], w[p]
        _set_lc(m.leaves()[0], x, w, oracle, rng)
    t = batch.compile_tree(m)
    p0 = np.array(m.dynasty_par_vals)
    walk = p0 * (1.0 + 0.01 * np.random.default_rng(23).standard_normal((W, p0.size)))
    bad = np.zeros(W, bool)
    if kind == "rejected":
        names = m.dynasty_par_names
        walk[2, [i for i, s in enumerate(names) if s.startswith("exp2")][0]] = 3e-3  # prior uniform(0.5, 5): out
        walk[5, 0] = np.nan
        bad[[2, 5]] = True
    ref, rlle, _ = oracle.lnprob_batch(walk, t)
    return t, walk, bad, ref, rlle


def _case(key, oracle):
    if key not in _CASES:
        _CASES[key] = _build(key, oracle)
    return _CASES[key]


def _check(key, oracle, layout):
    import ctypes
    import torch
    from lfit_python_amd import _native, batch
    t, walk, bad, ref, rlle = _case(key, oracle)
    assert np.all(np.isfinite(ref[~bad])) and np.all(np.isneginf(ref[bad]))
    ev = batch.LnProbEvaluator(t)
    assert _native.lib().lfg_layout(ctypes.byref(ev.ctree)) == layout   # the tree takes the layout under test
    lle = torch.empty((W, t.E), dtype=torch.float64, device="cuda")
    got = ev(torch.as_tensor(walk, device="cuda"), lnlike_e=lle).cpu().numpy()
    _same(got, ref, LNP_RTOL)
    _same(lle.cpu().numpy()[~bad], rlle[~bad], LNP_RTOL)


@LAYOUTS
@pytest.mark.parametrize("n", SIZES)
def test_one_eclipse_of_n_points(oracle, n, layout):
    _check(("grid", n), oracle, layout)


@LAYOUTS
def test_three_eclipse_tree_with_ragged_lengths(oracle, layout):
    """m differs per workgroup (the off[] path): 65, 300 and 512 points"""
    _check(("ragged", 0), oracle, layout)


@LAYOUTS
def test_point_major_tile_with_idle_waves(oracle, layout):
    """a shuffled 65-point file: the dir path, six waves without a point"""
    _check(("shuffled", 65), oracle, layout)


@LAYOUTS
def test_rejected_walkers_with_idle_waves(oracle, layout):
    """a prior-rejected and a NaN-coordinate walker among the 8, 65 points:
    the st != ST_OK exit with idle waves present"""
    _check(("rejected", 65), oracle, layout)
