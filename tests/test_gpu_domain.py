"""GPU: the device against the oracle over the whole parameter domain
(tests/domain_cases.py), as tests/test_domain_sweep.py compares the host
build of the same algorithm: element tables, flux with components and the
fused likelihood on 96 sets that reach eclipses out to +-0.2 in phase, and
the status rules of MODEL_SPEC 6 at their edges through every entry point.

The flux bound is the derived one of tests/test_domain_sweep.py: a contact
phase may differ by PHASE_ATOL, which one sub-bin of width 2h/nsub turns into
PHASE_ATOL / (2h / nsub) of the flux scale at the most.  The oracle's results
are computed once per module and left unchanged."""
import ctypes
import functools

import numpy as np
import pytest

from tests import domain_cases as dc
from tests.helpers import ECL1, TRUTH18
from tests.test_gpu_lnprob import LAYOUTS, layout  # noqa: F401 (layout: a fixture)
from tests.test_gpu_parity import PHASE_ATOL, _elements_gpu, _grazing_sets, assert_geo_matches
from tests.test_gpu_tab_start import WIDE

pytestmark = pytest.mark.gpu

FLIP_WIDTH = 1e-6     # test_element_tables_grazing's rule
N, H = 301, 1e-3
N_LONG, H_LONG = 700, 5e-4
YE = 0.01


def flux_bound(h, nsub):
    return PHASE_ATOL / (2.0 * h / nsub)


def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def sets96():
    """[96, 18]: 40 wide_box and 40 prior_box sets that are status-OK, the 4
    disputed sets and 12 of the existing wide-eclipse and grazing sets"""
    O = _oracle()

    def ok(p):
        return O.flux(p, np.zeros(1), np.zeros(1))[0] == 0
    wide = [p for p in dc.wide_box(96) if ok(p)][:40]
    prior = [p for p in dc.prior_box(96) if ok(p)][:40]
    extra = []
    for base in (TRUTH18, ECL1):
        for q, dphi, rdisc in WIDE:
            p = np.array(base, dtype=float)
            p[4], p[5], p[6] = q, dphi, rdisc
            extra.append(p)
    extra += _grazing_sets()
    out = np.array(wide + prior + [np.array(d) for d in dc.DISPUTED] + extra)
    assert out.shape == (96, 18)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_elements():
    O = _oracle()
    return tuple(O.elements(p) for p in sets96())


def _grid(n, h):
    x = (np.arange(n) - 0.5 * (n - 1)) * (2.0 * h)   # contiguous exposures of half-width h about phase 0
    return x, np.full(n, h)


@functools.lru_cache(maxsize=None)
def oracle_flux(n, h, nsub):
    """(status [96], [96, 5, n]: total, wd, disc, spot, donor)"""
    O = _oracle()
    x, w = _grid(n, h)
    st = np.empty(96, dtype=np.int32)
    fl = np.empty((96, 5, n))
    for i, p in enumerate(sets96()):
        st[i], comps = O.flux(p, x, w, nsub=nsub, components=True)
        fl[i] = comps
    fl.setflags(write=False)
    return st, fl


def test_element_tables_over_the_domain():
    pars = sets96()
    st, a, b, wg, don, geo = _elements_gpu(pars)
    ref = oracle_elements()
    worst = {"a": 0.0, "b": 0.0}
    flips = 0
    reach = 0.0
    for i in range(96):
        ost, oa, ob, ow, odon, ogeo = ref[i]
        assert st[i] == ost == 0, (i, st[i], ost)
        g, o = a[i] < b[i], oa < ob
        both = g & o
        only = g ^ o
        if only.any():   # a class may differ only on a vanishing chord
            width = np.where(g, b[i] - a[i], ob - oa)[only]
            assert np.max(width) < FLIP_WIDTH, (i, np.flatnonzero(only), width)
            flips += int(only.sum())
        if both.any():
            worst["a"] = max(worst["a"], float(np.max(np.abs(a[i][both] - oa[both]))))
            worst["b"] = max(worst["b"], float(np.max(np.abs(b[i][both] - ob[both]))))
            reach = max(reach, float(np.max(np.abs(np.concatenate([oa[both], ob[both]])))))
    print("96 sets: worst |da| %.2e |db| %.2e, %d class flips on vanishing chords, contacts out to %.3f in phase"
          % (worst["a"], worst["b"], flips, reach))
    assert reach > 0.15
    assert flips <= 0.01 * 96 * 1500
    for i in range(96):
        ost, oa, ob, ow, odon, ogeo = ref[i]
        both = (a[i] < b[i]) & (oa < ob)
        assert np.max(np.abs(a[i][both] - oa[both]), initial=0.0) <= PHASE_ATOL, i
        assert np.max(np.abs(b[i][both] - ob[both]), initial=0.0) <= PHASE_ATOL, i
        np.testing.assert_allclose(wg[i], ow, rtol=1e-12, err_msg=str(i))
        np.testing.assert_allclose(don[i], odon, rtol=1e-9, atol=1e-14, err_msg=str(i))
    bad = []
    for i in range(96):
        try:
            assert_geo_matches(geo[i], ref[i][5], label=str(i))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("nsub", [1, 3])
def test_flux_components_over_the_domain(nsub):
    from lfit_python_amd.lfit import flux_batch
    x, w = _grid(N, H)
    flux, status, comps = flux_batch(sets96(), x, w, nsub=nsub, components=True)
    flux, status, comps = flux.cpu().numpy(), status.cpu().numpy(), comps.cpu().numpy()
    ost, ofl = oracle_flux(N, H, nsub)
    assert np.array_equal(status, ost) and np.all(ost == 0)
    assert np.array_equal(np.isfinite(flux), np.isfinite(ofl[:, 0]))
    scale = np.max(np.abs(ofl[:, 0]), axis=1)
    err = np.max(np.abs(flux - ofl[:, 0]), axis=1) / scale
    cerr = np.max(np.abs(comps.transpose(1, 0, 2) - ofl[:, 1:]), axis=(1, 2)) / scale
    print("nsub %d: worst flux difference %.2e of the scale (set %d), worst component %.2e (set %d); bound %.1e"
          % (nsub, err.max(), int(err.argmax()), cerr.max(), int(cerr.argmax()), flux_bound(H, nsub)))
    assert err.max() <= flux_bound(H, nsub), np.flatnonzero(err > flux_bound(H, nsub))
    assert cerr.max() <= flux_bound(H, nsub), np.flatnonzero(cerr > flux_bound(H, nsub))
    np.testing.assert_allclose(comps.sum(0), flux, rtol=1e-12, atol=1e-15)


def _lnlike_reference(n, h, nsub):
    """y, ye, the reference -1/2 sum ((y - f) / ye)^2 in longdouble from the
    oracle's flux, and the tolerance of each set.  With |df| <= B S (B the
    flux bound, S the set's flux scale), d(ln_like) = sum r df / ye - 1/2
    sum (df / ye)^2 is at most B S sum |y - f| / ye^2 + N (B S / ye)^2 / 2;
    the sums' own rounding (N terms in FP64) is allowed 1e-12 of |ln_like|."""
    st, fl = oracle_flux(n, h, nsub)
    f = fl[:, 0]
    rng = np.random.default_rng(17)
    y = f[40] + YE * rng.standard_normal(n)      # data drawn from the first prior_box set
    ye = np.full(n, YE)
    r = (y[None, :].astype(np.longdouble) - f.astype(np.longdouble)) / np.longdouble(YE)
    ref = np.asarray(-0.5 * np.sum(r * r, axis=1), dtype=np.float64)
    B = flux_bound(h, nsub)
    S = np.max(np.abs(f), axis=1)
    tol = B * S * np.sum(np.abs(y[None, :] - f), axis=1) / YE ** 2 + 0.5 * n * (B * S / YE) ** 2 + 1e-12 * np.abs(ref)
    return y, ye, ref, tol


@LAYOUTS
@pytest.mark.parametrize("n,h,nsub", [(N, H, 1), (N, H, 3), (N_LONG, H_LONG, 1)], ids=["n301", "n301_nsub3", "long700"])
def test_lnlike_over_the_domain(n, h, nsub, layout):
    from lfit_python_amd.lfit import lnlike_batch
    x, w = _grid(n, h)
    y, ye, ref, tol = _lnlike_reference(n, h, nsub)
    got, st = lnlike_batch(sets96(), x, y, ye, width=w, nsub=nsub)
    got, st = got.cpu().numpy(), st.cpu().numpy()
    assert np.all(st == 0) and np.all(np.isfinite(got))
    d = np.abs(got - ref)
    k = int(np.argmax(d / tol))
    print("layout %d n %d nsub %d: worst |d ln_like| / tolerance %.2e (set %d: %.3e of %.3e, ln_like %.6e)"
          % (layout, n, nsub, d[k] / tol[k], k, d[k], tol[k], ref[k]))
    assert np.all(d <= tol), [(int(i), float(d[i]), float(tol[i])) for i in np.flatnonzero(d > tol)]


# ------------------------------------------------------------ status edges
def _edge_sets(npar):
    edges = [e for e in dc.status_edges() if npar == 18 or not e[3]]
    pars = np.array([e[1] for e in edges])
    return edges, np.ascontiguousarray(pars if npar == 18 else dc.simple(pars))


def _edge_data():
    x, w = _grid(N, H)
    rng = np.random.default_rng(2)
    return x, w, 0.1 + YE * rng.standard_normal(N), np.full(N, YE)


def _one_eclipse_tree(npar):
    """a one-eclipse tree whose walker is the CV parameter vector itself: no
    Roche priors, and (LnProbEvaluator.ctree.prior_type = None) no priors"""
    from lfit_python_amd import batch
    x, w, y, ye = _edge_data()
    gather = np.arange(18, dtype=np.int32)[None, :].copy()
    gather[0, npar:] = gather[0, 0]
    return batch.CompiledTree(
        E=1, ndim=npar, names=["p%d" % k for k in range(npar)], gather=gather, npars=np.array([npar], np.int32),
        consts=np.zeros(0), offsets=np.array([0, N], np.int32), x=x, y=y, ye=ye, w=w,
        prior_type=np.full(npar, 2, np.int32), prior_p1=np.full(npar, -1e300), prior_p2=np.full(npar, 1e300),
        prior_norm=np.ones(npar), roche_priors=False)


def _same_rows(full, part, keep, label):
    """rows `keep` of the call with the failing sets equal the call without them, bit for bit"""
    assert np.array_equal(np.asarray(full)[keep], np.asarray(part), equal_nan=True), label


@pytest.mark.parametrize("npar", [18, 14])
def test_status_edges_flux_and_elements(npar):
    from lfit_python_amd.lfit import flux_batch
    edges, pars = _edge_sets(npar)
    want = np.array([e[2] for e in edges])
    keep = np.flatnonzero(want == 0)
    assert len(keep) >= 8 and set(want.tolist()) == {0, 1, 2, 3, 4, 5}
    x, w = _grid(N, H)
    flux, st = flux_batch(pars, x, w)
    flux, st = flux.cpu().numpy(), st.cpu().numpy()
    wrong = np.flatnonzero(st != want)
    assert wrong.size == 0, [(edges[k][0], int(st[k]), int(want[k])) for k in wrong]
    assert np.all(np.isnan(flux[want != 0])) and np.all(np.isfinite(flux[keep]))
    f2, st2 = flux_batch(pars[keep], x, w)
    assert np.all(st2.cpu().numpy() == 0)
    _same_rows(flux, f2.cpu().numpy(), keep, "lfg_flux")
    est, a, b, wg, don, geo = _elements_gpu(pars)
    wrong = np.flatnonzero(est != want)
    assert wrong.size == 0, [(edges[k][0], int(est[k]), int(want[k])) for k in wrong]
    est2, a2, b2, wg2, don2, geo2 = _elements_gpu(pars[keep])
    assert np.all(est2 == 0)
    for full, part, name in ((a, a2, "a"), (b, b2, "b"), (wg, wg2, "wgt"), (don, don2, "donor")):
        _same_rows(full, part, keep, "lfg_elements " + name)


@LAYOUTS
@pytest.mark.parametrize("npar", [18, 14])
def test_status_edges_lnlike_and_lnprob(npar, layout):
    import torch
    from lfit_python_amd import batch
    from lfit_python_amd.lfit import lnlike_batch
    edges, pars = _edge_sets(npar)
    want = np.array([e[2] for e in edges])
    keep = np.flatnonzero(want == 0)
    x, w, y, ye = _edge_data()
    ll, st = lnlike_batch(pars, x, y, ye, width=w)
    ll, st = ll.cpu().numpy(), st.cpu().numpy()
    wrong = np.flatnonzero(st != want)
    assert wrong.size == 0, [(edges[k][0], int(st[k]), int(want[k])) for k in wrong]
    assert np.all(np.isneginf(ll[want != 0])) and np.all(np.isfinite(ll[keep]))
    ll2, st2 = lnlike_batch(pars[keep], x, y, ye, width=w)
    assert np.all(st2.cpu().numpy() == 0)
    _same_rows(ll, ll2.cpu().numpy(), keep, "lfg_lnlike")
    # lfg_lnprob: W = the number of edge cases, the walker is the CV vector
    t = _one_eclipse_tree(npar)
    ev = batch.LnProbEvaluator(t)
    ev.ctree.prior_type = None
    ev.ctree.prior_c = None
    assert _layout_of(ev) == layout
    lnp = ev(torch.as_tensor(pars, device="cuda")).cpu().numpy()
    assert np.all(np.isneginf(lnp[want != 0])), [edges[k][0] for k in np.flatnonzero((want != 0) & ~np.isneginf(lnp))]
    assert np.all(np.isfinite(lnp[keep])), [edges[k][0] for k in keep[~np.isfinite(lnp[keep])]]
    np.testing.assert_allclose(lnp[keep], ll[keep], rtol=1e-12, atol=1e-9)   # no priors: ln_prob is the ln_like
    lnp2 = ev(torch.as_tensor(pars[keep], device="cuda")).cpu().numpy()
    _same_rows(lnp, lnp2, keep, "lfg_lnprob")


def _layout_of(ev):
    from lfit_python_amd import _native
    return _native.lib().lfg_layout(ctypes.byref(ev.ctree))
