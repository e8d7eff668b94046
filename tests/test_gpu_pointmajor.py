"""GPU: k_pair's point-major branch against the oracle.

A tile goes point-major when any of its exposure windows is out of order
(lo, hi or phase below its predecessor's) or has a negative or NaN width
(lfg_k_pair.hpp: k_pair's prologue, the sortedness flags); the element phase then writes
its tables into LDS and every point scans them (pair_direct_wd_disc,
direct_spot, direct_donor).  The reference accepts such light curves:
Lightcurve.from_calib keeps the file's order and sets w = mean(diff(x))/2,
negative for a descending file (/root/reference/CVModel.py:51-64), and a
phi0 shift or a phase range past 0.5 wraps points through +-0.5.

Every case runs through lfg_lnprob (a compiled one-eclipse tree and a
three-eclipse tree with one such eclipse) and lfg_lnlike on both kernel
layouts, against oracle.lnprob_batch at LNP_RTOL.  MODEL_SPEC 3 fixes the
semantics the oracle states: a negative width at S = 1 is point evaluation at
the centre, and a NaN width gives a NaN flux at that point (chi^2 = inf,
CVModel.py:161-171)."""
import numpy as np
import pytest

from tests.test_gpu_lnprob import LAYOUTS, LNP_RTOL, _same, layout  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CASES = ["shuffled", "descending", "wrap", "ragged_unsorted_hi", "nan_width"]


def _lightcurve(kind):
    """(x, w) of a <= 512-point, S = 1 light curve that sends k_pair's tile
    point-major, and whether the tile really is out of order"""
    from lfit_python_amd.synthetic import phase_grid
    rng = np.random.default_rng(17)
    if kind == "shuffled":            # a calib file in arbitrary order
        x, w = phase_grid(300)
        p = rng.permutation(x.size)
        x, w = x[p], w[p]
    elif kind == "descending":        # a descending file: w = mean(diff(x))/2 < 0
        x = np.linspace(0.3, -0.3, 300)
        w = np.mean(np.diff(x)) * np.ones_like(x) / 2.0
        assert np.all(w < 0)
    elif kind == "wrap":              # phases run past 0.5: wrap to -0.5 mid-file
        x, w = phase_grid(400, 0.45, 1.1)
    elif kind == "ragged_unsorted_hi":  # sorted centres, ragged widths: hi out of order
        x = np.sort(rng.uniform(-0.25, 0.25, 350))
        w = rng.uniform(1e-4, 4e-3, x.size)
        hi = x + w
        assert np.any(np.diff(hi) < 0)
    else:                             # one NaN width (the point's flux is NaN)
        x, w = phase_grid(300)
        w = w.copy()
        w[137] = np.nan
    return x, w


def _model(kind, oracle, E=1):
    """a tree whose eclipse 0 (of E) carries the point-major light curve;
    y is the oracle's model flux at the truth plus noise (the NaN-width
    point's y from its neighbour's width)"""
    from lfit_python_amd import synthetic
    from lfit_python_amd.synthetic import NOISE
    if E == 1:
        m = synthetic.config_single(300)
    else:
        m = synthetic.config_tree(1, 300)      # 3 bands x 1 eclipse
    leaf = m.leaves()[0]
    x, w = _lightcurve(kind)
    wy = np.where(np.isnan(w), np.nanmean(w), w)
    rng = np.random.default_rng(3)
    for k, lf in enumerate(m.leaves()):
        if k == 0:
            lf.lc.x, lf.lc.w = x, w
            lf.lc.ye = NOISE * np.ones_like(x)
            st, f = oracle.flux(lf.cv_parlist, x, wy)
        else:
            st, f = oracle.flux(lf.cv_parlist, lf.lc.x, lf.lc.w)
        assert st == 0
        lf.lc.y = f + NOISE * rng.standard_normal(f.shape)
    assert leaf.lc.x.size <= 512
    return m


def _walkers(m, W, seed=23):
    rng = np.random.default_rng(seed)
    p0 = np.array(m.dynasty_par_vals)
    return p0 * (1.0 + 0.01 * rng.standard_normal((W, p0.size)))


@LAYOUTS
@pytest.mark.parametrize("kind", CASES)
def test_lnprob_point_major_matches_oracle(oracle, kind, layout):
    import ctypes
    import torch
    from lfit_python_amd import _native, batch
    m = _model(kind, oracle)
    t = batch.compile_tree(m)
    ev = batch.LnProbEvaluator(t)
    assert _native.lib().lfg_layout(ctypes.byref(ev.ctree)) == layout   # the tree takes the layout under test
    W = 64
    walk = _walkers(m, W)
    lle = torch.empty((W, 1), dtype=torch.float64, device="cuda")
    got = ev(torch.as_tensor(walk, device="cuda"), lnlike_e=lle).cpu().numpy()
    ref, rlle, _ = oracle.lnprob_batch(walk, t)
    if kind == "nan_width":
        # every walker meets the NaN point: ln_like = -inf, so ln_prob = -inf
        assert np.all(np.isneginf(got)) and np.all(np.isneginf(ref))
        assert np.all(np.isneginf(lle.cpu().numpy()))
    else:
        assert np.isfinite(ref).sum() >= W // 2
        fin = np.isfinite(ref)
        _same(lle.cpu().numpy()[fin], rlle[fin], LNP_RTOL)
    _same(got, ref, LNP_RTOL)


@LAYOUTS
@pytest.mark.parametrize("kind", ["shuffled", "descending", "wrap"])
def test_lnprob_point_major_in_a_three_eclipse_tree(oracle, kind, layout):
    """eclipse 0 point-major, eclipses 1-2 sorted: the per-eclipse tiles
    decide their pass independently (k_pair's offsets path, E > 1)"""
    import torch
    from lfit_python_amd import batch
    m = _model(kind, oracle, E=3)
    t = batch.compile_tree(m)
    assert t.E == 3
    W = 32
    walk = _walkers(m, W, seed=5)
    ev = batch.LnProbEvaluator(t)
    lle = torch.empty((W, 3), dtype=torch.float64, device="cuda")
    got = ev(torch.as_tensor(walk, device="cuda"), lnlike_e=lle).cpu().numpy()
    ref, rlle, _ = oracle.lnprob_batch(walk, t)
    assert np.isfinite(ref).sum() >= W // 2
    _same(got, ref, LNP_RTOL)
    fin = np.isfinite(ref)
    _same(lle.cpu().numpy()[fin], rlle[fin], LNP_RTOL)


@LAYOUTS
@pytest.mark.parametrize("kind", CASES)
def test_lnlike_point_major_matches_oracle(oracle, kind, layout):
    """lfg_lnlike (no tree, no priors) on the same light curves: each
    parameter set's ln_like against the oracle's flux -> chi^2"""
    from lfit_python_amd.lfit import lnlike_batch
    m = _model(kind, oracle)
    leaf = m.leaves()[0]
    W = 48
    walk = _walkers(m, W, seed=9)
    pars = np.empty((W, 18))
    for i in range(W):
        m.dynasty_par_vals = walk[i]
        pars[i] = leaf.cv_parlist
    lc = leaf.lc
    got, st = lnlike_batch(pars, lc.x, lc.y, lc.ye, width=lc.w)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    ref = np.empty(W)
    for i in range(W):
        s, f = oracle.flux(pars[i], lc.x, lc.w)
        assert s == st[i]
        ref[i] = -np.inf if (s != 0 or np.any(np.isnan(f))) else -0.5 * np.sum(((lc.y - f) / lc.ye) ** 2)
    if kind == "nan_width":
        assert np.all(np.isneginf(got))
    else:
        assert np.isfinite(ref).sum() >= W // 2
    _same(got, ref, LNP_RTOL)


@pytest.mark.parametrize("kind", CASES)
def test_point_major_flux_matches_oracle(oracle, kind):
    """lfg_flux (the two-kernel k_lnlike<0>) on the same light curves, S = 1
    and S = 3: the flux itself, NaN exactly where the width is NaN"""
    from lfit_python_amd.lfit import flux_batch
    from tests.helpers import random_pars
    x, w = _lightcurve(kind)
    pars = random_pars(6, complex_bs=True, seed=13)
    for nsub in (1, 3):
        flux, status = flux_batch(pars, x, w, nsub=nsub)
        flux, status = flux.cpu().numpy(), status.cpu().numpy()
        n_ok = 0
        for i, p in enumerate(pars):
            st, f = oracle.flux(p, x, w, nsub=nsub)
            assert status[i] == st
            if st != 0:
                continue
            n_ok += 1
            assert np.array_equal(np.isnan(flux[i]), np.isnan(f))
            ok = ~np.isnan(f)
            scale = np.max(np.abs(f[ok]))
            assert np.max(np.abs(flux[i][ok] - f[ok])) / scale < 1e-6
        assert n_ok >= 4
