"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Bar (BASELINE.json north_star): flux within 1e-6 relative of the oracle on
identical (pars, phase, width).  The kernels and the oracle solve the same
converged root-finding problems, so the observed agreement is ~1e-12; the
tolerances below are the contract, not the observation.
"""
import numpy as np
import pytest

from tests.helpers import TRUTH14, TRUTH18, ECL1, random_pars, phase_grid

pytestmark = pytest.mark.gpu

FLUX_RTOL = 1e-6      # north_star contract, relative to the flux scale
PHASE_ATOL = 1e-10    # eclipse contact phases (the tangency Newton stops at |dth| <= 1e-6: ~1e-12 in phase)


def _rel(a, b, scale):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / scale


def test_roche_primitives(oracle):
    from lfit_python_amd import roche
    qs = np.array([0.05, 0.1037, 0.2, 0.5, 1.0, 2.0])
    np.testing.assert_allclose(roche.xl1(qs), [oracle.xl1(q) for q in qs], rtol=1e-13)
    assert abs(roche.xl1(1.0) - 0.5) < 1e-14
    for q in qs:
        for inc in (84.0, 86.9, 90.0):
            assert abs(roche.findphi(q, inc) - oracle.findphi(q, inc)) < 1e-11
        dphi = oracle.findphi(q, 85.0)
        assert abs(roche.findi(q, dphi) - 85.0) < 1e-8
        assert abs(roche.findi(q, dphi) - oracle.findi(q, dphi)) < 1e-9
        x1 = oracle.xl1(q)
        for rad in (0.35 * x1, 0.55 * x1):
            np.testing.assert_allclose(roche.bspot(q, rad), oracle.bspot(q, rad), rtol=1e-9, atol=1e-11)


def test_stream_table_matches_oracle(oracle):
    """bspot over the stream table's whole domain (MODEL_SPEC 4.5): random
    (q, s) with s near periastron and toward the start point, and q outside
    the table (the fine RK4).  Kernels and oracle evaluate the same
    coefficients, so they agree to rounding."""
    from lfit_python_amd import roche
    rng = np.random.default_rng(31)
    qs = np.concatenate([np.exp(rng.uniform(np.log(0.002), np.log(5.0), 24)), [0.0015, 6.0]])
    for q in qs:
        x1 = oracle.xl1(q)
        grid = x1 * np.arange(1, 400) / 400.0
        ok = []
        for r in grid:
            try:
                oracle.bspot(q, r)
                ok.append(r)
            except ValueError:
                pass
        assert ok, q
        r_lo, r_hi = min(ok), max(ok)  # within a grid step of r_min and r0
        rads = np.concatenate([r_lo + (r_hi - r_lo) * np.array([0.0, 1e-4, 0.01, 0.3, 0.7, 0.99, 1.0]),
                               [0.5 * r_lo, r_hi + 0.5 * (x1 - r_hi)]])
        for rad in rads:
            try:
                ref = oracle.bspot(q, rad)
            except ValueError:
                with pytest.raises(roche.RocheError):
                    roche.bspot(q, rad)
                continue
            got = roche.bspot(q, rad)
            np.testing.assert_allclose(got[:2], ref[:2], rtol=0, atol=1e-12)
            np.testing.assert_allclose(got[2:], ref[2:], rtol=0, atol=1e-10)


def test_roche_errors():
    from lfit_python_amd import roche
    with pytest.raises(roche.RocheError):
        roche.xl1(-1.0)
    with pytest.raises(roche.RocheError):
        roche.findi(0.1, 0.3)          # wider than any inclination allows
    with pytest.raises(roche.RocheError):
        roche.bspot(0.1, 0.01)         # inside the stream's periastron
    with pytest.raises(roche.RocheError):
        roche.findphi(0.05, 80.0)      # the WD centre is never eclipsed


def _elements_gpu(pars):
    import ctypes
    import torch
    from lfit_python_amd import _native
    L = _native.lib()
    P = torch.as_tensor(np.atleast_2d(pars), dtype=torch.float64, device="cuda").contiguous()
    W, npar = P.shape
    a = torch.empty((W, _native.NEL), dtype=torch.float64, device="cuda")
    b, wg = torch.empty_like(a), torch.empty_like(a)
    don = torch.empty((W, _native.NDONOR, 3), dtype=torch.float64, device="cuda")
    geo = torch.empty((W, _native.NGEO), dtype=torch.float64, device="cuda")
    st = torch.empty(W, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lfg_workspace_size(W, 1), dtype=torch.uint8, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.lfg_elements(vp(P), W, npar, vp(a), vp(b), vp(wg), vp(don), vp(geo), vp(st),
                        vp(ws), ws.numel(), _native.stream_ptr())
    assert rc == 0
    return [t.cpu().numpy() for t in (st, a, b, wg, don, geo)]


# what the oracle's geo record (lfo_elements) and the device's (lfg_device.hpp
# enum Geo) both hold: oracle slot -> device slot.  The oracle's stream
# velocity and donor norm have no device counterpart (the element kernels
# compute neither), and the device's other slots are inputs or derived
# (sin i, cos i, the strip's direction, the beaming normal).
GEO_PAIRS = {"xl1": (0, 4), "pl1": (1, 5), "inc": (2, 10), "rwd_a": (3, 11), "rdisc_a": (4, 12), "bs_x": (5, 16),
             "bs_y": (6, 17), "upk": (9, 21), "umax": (10, 22), "l": (11, 20), "bden": (12, 31), "reff": (14, 13),
             "lnpk": (15, 23)}
GEO_TOL = 1e-12


def assert_geo_matches(geo, ogeo, label=""):
    """the geometry both sides export (x_L1, Phi(L1), inclination, radii, the
    stream's impact point, the strip's profile constants, the beaming
    denominator) to GEO_TOL, relative, or absolute for values below 1.

    The inclination alone has a second rule.  The eclipse is symmetric in
    cos i, so dphi fixes cos^2 i, and next to 90 degrees the inclination
    itself only as well as d(cos^2 i) / (2 cos i): two solves of the egress
    phase to 1e-13 rad differ by 2e-9 degrees at i = 89.965.  There the
    comparison is on cos^2 i, at GEO_TOL / 10 (which is the tighter rule
    wherever cos i > 0.05).
    The beaming denominator is fis + (1 - fis) max(0, |sin t| sin i + cos t
    cos i): it follows cos i with a slope of at most 1 + cot i < 2 (i > 45
    degrees wherever the WD is eclipsed), so it may differ by twice the two
    sides' difference in cos i beside GEO_TOL."""
    bad = []
    ci = [np.cos(np.radians(g[k])) for g, k in ((geo, GEO_PAIRS["inc"][1]), (ogeo, GEO_PAIRS["inc"][0]))]
    for name, (ko, kd) in GEO_PAIRS.items():
        ok = abs(geo[kd] - ogeo[ko]) <= GEO_TOL * max(1.0, abs(ogeo[ko]))
        if name == "inc" and not ok:
            ok = abs(ci[0] ** 2 - ci[1] ** 2) <= 0.1 * GEO_TOL
        if name == "bden" and not ok:
            ok = abs(geo[kd] - ogeo[ko]) <= GEO_TOL + 2.0 * abs(ci[0] - ci[1])
        if not ok:
            bad.append((name, float(geo[kd]), float(ogeo[ko])))
    assert not bad, (label, bad)


@pytest.mark.parametrize("pars", [TRUTH18, ECL1, TRUTH14])
def test_element_tables(oracle, pars):
    st, a, b, wg, don, geo = _elements_gpu(pars)
    ost, oa, ob, ow, odon, ogeo = oracle.elements(pars)
    assert st[0] == ost == 0
    ecl = oa < ob
    assert np.array_equal(a[0] < b[0], ecl)
    assert np.max(np.abs(a[0][ecl] - oa[ecl])) < PHASE_ATOL
    assert np.max(np.abs(b[0][ecl] - ob[ecl])) < PHASE_ATOL
    np.testing.assert_allclose(wg[0], ow, rtol=1e-12)
    np.testing.assert_allclose(don[0], odon, rtol=1e-9, atol=1e-14)
    assert_geo_matches(geo[0], ogeo)


def _grazing_sets():
    """parameter sets whose eclipse chords graze the WD and the disc: small
    dphi (inclination near the lowest that eclipses the WD centre) and a
    large disc, where the tangency equation's slope g' is small and the
    Newton stop rule (|dth| <= 1e-6, ~|dth|^2 g''/2g' after the step) is
    weakest"""
    out = []
    for q, dphi, rdisc in ((0.1037, 0.006, 0.45), (0.1037, 0.012, 0.6), (0.3, 0.008, 0.5), (0.05, 0.004, 0.4)):
        p = np.array(TRUTH18, dtype=float)
        p[4], p[5], p[6] = q, dphi, rdisc
        out.append(p)
    return out


@pytest.mark.parametrize("k", range(4))
def test_element_tables_grazing(oracle, k):
    """near-grazing contacts against the oracle's nested solver: every
    interval both find within PHASE_ATOL; an element one solver finds
    eclipsed and the other not must be a vanishing chord (< 1e-6 phase)"""
    pars = _grazing_sets()[k]
    st, a, b, wg, don, geo = _elements_gpu(pars)
    ost, oa, ob, ow, odon, ogeo = oracle.elements(pars)
    assert st[0] == ost == 0
    g, o = a[0] < b[0], oa < ob
    both = g & o
    assert both.sum() > 50
    assert np.max(np.abs(a[0][both] - oa[both])) < PHASE_ATOL
    assert np.max(np.abs(b[0][both] - ob[both])) < PHASE_ATOL
    only = g ^ o
    if only.any():
        width = np.where(g, b[0] - a[0], ob - oa)[only]
        assert np.max(width) < 1e-6, width


@pytest.mark.parametrize("complex_bs", [True, False])
@pytest.mark.parametrize("nsub", [1, 5])
def test_flux_matches_oracle(oracle, complex_bs, nsub):
    from lfit_python_amd.lfit import flux_batch
    pars = random_pars(24, complex_bs=complex_bs, seed=11 + nsub)
    x, w = phase_grid(300)
    flux, status, comps = flux_batch(pars, x, w, nsub=nsub, components=True)
    flux, status, comps = flux.cpu().numpy(), status.cpu().numpy(), comps.cpu().numpy()
    n_ok = 0
    for i, p in enumerate(pars):
        st, (f, ywd, yd, ys, yrs) = oracle.flux(p, x, w, nsub=nsub, components=True)
        assert status[i] == st
        if st != 0:
            assert np.all(np.isnan(flux[i]))
            continue
        n_ok += 1
        scale = np.max(np.abs(f))
        assert _rel(flux[i], f, scale) < FLUX_RTOL
        for k, ref in enumerate((ywd, yd, ys, yrs)):
            assert _rel(comps[k, i], ref, scale) < FLUX_RTOL
        np.testing.assert_allclose(comps[:, i].sum(0), flux[i], rtol=1e-12, atol=1e-15)
    assert n_ok >= 18


def test_absurd_geometry_matches(oracle):
    """lfg_flux has no prior to reject with: a bright-spot exponent exp2 ->
    0 places the strip at ~1e270 (bs_umax), and such elements must leave
    both solvers at once as uneclipsed (the !(cos D < 1) test) instead of
    iterating on non-finite geometry -- on the GPU and in the oracle alike."""
    from lfit_python_amd.lfit import flux_batch
    pars = np.array(random_pars(16, complex_bs=True, seed=5))
    pars[::2, 15] = 3e-3          # exp2 (cv_parlist slot 15)
    pars[1::4, 14] = 1e-3         # and a tiny exp1 beside it
    x, w = phase_grid(300)
    flux, status = flux_batch(pars, x, w)
    flux, status = flux.cpu().numpy(), status.cpu().numpy()
    for i, p in enumerate(pars):
        st, f = oracle.flux(p, x, w)
        assert status[i] == st
        # the spot's weights over- or underflow at such a strip: the flux is
        # then NaN in both (the reference's chisq maps NaN to inf)
        ok = np.isfinite(f)
        assert np.array_equal(np.isfinite(flux[i]), ok)
        if ok.any():
            assert _rel(flux[i][ok], f[ok], np.max(np.abs(f[ok]))) < FLUX_RTOL


@pytest.mark.perf
def test_absurd_geometry_stays_fast():
    """The wall-clock side of test_absurd_geometry_matches (perf marker: a
    shared box can slow it for other reasons): absurd strips leave the
    solvers at once instead of iterating on non-finite geometry."""
    import time
    import torch
    from lfit_python_amd.lfit import flux_batch
    pars = np.array(random_pars(16, complex_bs=True, seed=5))
    pars[::2, 15] = 3e-3
    pars[1::4, 14] = 1e-3
    x, w = phase_grid(300)
    flux_batch(pars, x, w)        # warm
    times = []
    for _ in range(3):   # the fastest of three: a host stall cannot decide it
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flux_batch(pars, x, w)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert min(times) < 0.05, "flux_batch calls (s): %s" % np.round(times, 4)


def test_cv_object_api(oracle):
    """lfit.CV(pars).calcFlux(pars, x, w) and the ywd/yd/ys/yrs attributes."""
    from lfit_python_amd.lfit import CV, LfitError
    x, w = phase_grid(300)
    cv = CV(TRUTH18)
    f = cv.calcFlux(TRUTH18, x, w)
    _, (of, ywd, yd, ys, yrs) = oracle.flux(TRUTH18, x, w, components=True)
    assert _rel(f, of, of.max()) < FLUX_RTOL
    for got, ref in ((cv.ywd, ywd), (cv.yd, yd), (cv.ys, ys), (cv.yrs, yrs)):
        assert _rel(got, ref, of.max()) < FLUX_RTOL
    # width inferred from the data when absent (README.md:63, CVModel.py:30)
    np.testing.assert_allclose(cv(TRUTH18, x), f, rtol=0, atol=0)
    bad = list(TRUTH18)
    bad[5] = 0.4  # dphi impossible
    with pytest.raises(LfitError):
        cv.calcFlux(bad, x, w)


def test_point_evaluation_and_edges(oracle):
    from lfit_python_amd.lfit import flux_batch
    x = np.linspace(-0.5, 0.5, 257)
    f, st = flux_batch(np.array([TRUTH18]), x, np.zeros_like(x))
    st0, of = oracle.flux(TRUTH18, x, np.zeros_like(x))
    assert st[0].item() == st0 == 0
    assert _rel(f.cpu().numpy()[0], of, of.max()) < FLUX_RTOL
    # out of eclipse the components sum to their maximum-light fluxes
    f, st, c = flux_batch(np.array([TRUTH18]), np.array([0.45]), np.array([0.0]), components=True)
    c = c.cpu().numpy()[:, 0, 0]
    assert abs(c[0] - TRUTH18[0]) < 1e-14 and abs(c[1] - TRUTH18[1]) < 1e-14
    # empty phase array
    f, st = flux_batch(np.array([TRUTH18]), np.zeros(0), np.zeros(0))
    assert f.shape == (1, 0)


def _grid_case(kind):
    rng = np.random.default_rng(5)
    if kind == "multi_tile":       # 3 sweep tiles, the last one ragged
        x, w = phase_grid(1300, -0.25, 0.25)
    elif kind == "shuffled":       # unsorted phases: the ring-scan path
        x, w = phase_grid(300)
        perm = rng.permutation(len(x))
        x, w = x[perm], w[perm]
    elif kind == "wide_exposures":  # exposures overlap many neighbours
        x, w = phase_grid(200, -0.15, 0.15)
        w = w * 9.0
    elif kind == "ragged_widths":  # sorted lo/hi with varying widths
        x = np.sort(rng.uniform(-0.2, 0.2, 400))
        w = np.full_like(x, 4e-4)
    else:                          # phases wrap through +-0.5 inside the data
        x, w = phase_grid(300, 0.2, 0.8)
    return x, w


@pytest.mark.parametrize("kind", ["multi_tile", "shuffled", "wide_exposures", "ragged_widths", "wrap"])
def test_flux_phase_layouts(oracle, kind):
    """Sweep (sorted tiles) and ring-scan (unsorted) paths both match the oracle."""
    from lfit_python_amd.lfit import flux_batch
    x, w = _grid_case(kind)
    pars = random_pars(6, complex_bs=True, seed=3)
    flux, status = flux_batch(pars, x, w, nsub=3)
    flux, status = flux.cpu().numpy(), status.cpu().numpy()
    n_ok = 0
    for i, p in enumerate(pars):
        st, f = oracle.flux(p, x, w, nsub=3)
        assert status[i] == st
        if st == 0:
            n_ok += 1
            assert _rel(flux[i], f, np.max(np.abs(f))) < FLUX_RTOL
    assert n_ok >= 4
