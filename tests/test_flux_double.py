"""CPU: the oracle and the host twins against the flux double
(tests/flux_double.py), an independent numpy reading of MODEL_SPEC 1-5.

The double's slow parts (the arbiter's intervals, the inclination, the
stream's impact point) are read from tests/golden/flux_double.npz
(tools/make_flux_golden.py); the first tests show that the file is the
double's.  Then, for every recorded parameter set:
  oracle.elements   mask, intervals, weights, donor vectors, geometry;
  oracle.flux       with components, on the grids of KINDS, nsub 1, 3, 5;
  oracle.component  default grids for every set, caller-chosen ones for the first;
  cpu_baseline      lfg_cpu_flux and lfg_cpu_lnlike (the host port that
                    tests/test_abi_host.py drives) on the same grids.

Tolerance (bound(), derived, not tuned).  Each component is compared relative
to its own flux parameter.  A contact may differ by PHASE_ATOL (the project's
contract for contact phases), so an element's overlap with a sub-bin of width
2h/nsub differs by at most 2 PHASE_ATOL, a fraction 2 PHASE_ATOL / (2h/nsub)
of it; the weights are normalised, so that is the bound of the component.  A
floor of 1e-12 covers 1 500 weighted terms summed in another order.  Never
above FLUX_RTOL.  Every window here has h >= 1e-3, so the bound stays below
1e-6 up to nsub = 5.  A point evaluation has no window: the floor alone
applies, and the test first asserts on the file alone that each such point
lies 1e-9 or more from every recorded contact.

Teeth.  Every `mutate` value of the double must miss the unmutated double by
100 times that bound at some point of some case, in the component it touches.
"""
import json
import os

import numpy as np
import pytest

from tests import contact_double as cd
from tests import flux_double as fd
from tests.helpers import ECL1, TRUTH14, TRUTH18, phase_grid

PHASE_ATOL = 1e-10    # tests/test_gpu_parity.py
FLUX_RTOL = 1e-6      # tests/test_gpu_parity.py
GEO_TOL = 1e-12       # tests/test_gpu_parity.py
FLOOR = 1e-12
POINT_CLEARANCE = 1e-9
GOLD = os.path.join(os.path.dirname(__file__), "golden", "flux_double.npz")
DISC_GRIDS = {250: (10, 25), 777: (18, 43)}      # MODEL_SPEC 5.6's rule
DONOR_GRIDS = {250: (16, 16), 777: (28, 28)}

_cache = {}


def records():
    """{name: record} of the fixture, in its order"""
    if "rec" not in _cache:
        d = np.load(GOLD)
        out = {}
        for name in d["names"]:
            pre = str(name) + "/"
            out[str(name)] = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
        _cache["rec"] = out
    return _cache["rec"]


NAMES = ["truth18", "ecl1", "truth14", "q_above_1", "q_small", "grazing"]


def the_model(name, mutate=None):
    key = (name, mutate)
    if key not in _cache:
        rec = records()[name]
        _cache[key] = fd.model(rec["pars"], record=rec, mutate=mutate)
    return _cache[key]


def double_curve(name, kind, N, nsub):
    """the double's light curve of a recorded set on a case's grid, computed once"""
    key = (name, kind, N, nsub)
    if key not in _cache:
        x, w = grid(kind, N)
        _cache[key] = fd.light_curve(the_model(name), x, w, nsub)
    return _cache[key]


# ------------------------------------------------------------------ grids
def grid(kind, N=300):
    """(x, w) of a case.  Every window has h >= 1e-3."""
    rng = np.random.default_rng(4 + N)
    if N == 1:
        x, w = np.array([0.0031]), np.array([2e-3])
        if kind in ("points", "tiny", "edges"):
            w = np.array([0.0 if kind == "points" else 1e-300])
        return x, w
    if kind == "regular":
        x, w = phase_grid(N, -0.3, 0.3)
        w = np.maximum(w, 1e-3)
    elif kind == "wrap":          # through +1/2 and on through the eclipse at 1
        x = np.linspace(0.3, 1.3, N)
        w = np.full(N, max(0.5 / (N - 1), 1e-3))
    elif kind == "ragged":
        x = np.sort(rng.uniform(-0.2, 0.2, N))
        w = rng.uniform(1e-3, 4e-3, N)
    elif kind == "unsorted":
        x, w = phase_grid(N, -0.3, 0.3)
        w = np.maximum(w, 1e-3) * rng.uniform(1.0, 2.0, N)
        perm = rng.permutation(N)
        x, w = x[perm], w[perm]
    elif kind == "points":        # w = 0 everywhere
        x = np.linspace(-0.25, 0.25, N) + 1.7e-5
        w = np.zeros(N)
    elif kind == "tiny":          # widths below the spacing of the doubles everywhere: sorted, so no direct pass
        x = np.linspace(-0.25, 0.25, N) + 0.9e-5
        w = np.full(N, 1e-300)
    elif kind == "edges":         # zero, negative, sub-spacing and NaN widths among windows
        x = np.linspace(-0.25, 0.25, N) + 2.3e-5
        w = np.full(N, 1.5e-3)
        w[0::4] = 0.0
        w[1::4] = -1e-3
        w[2::4] = 1e-300
        w[N // 2 | 3] = np.nan
    else:
        raise KeyError(kind)
    return x, w


KINDS = ["regular", "wrap", "ragged", "unsorted", "points", "tiny", "edges"]


def is_point(x, w):
    """where MODEL_SPEC 3 evaluates at a point: w <= 0, or no window left"""
    return ~np.isnan(w) & ((w <= 0.0) | ~(x + w > x - w))


def bound(x, w, nsub):
    """per point, relative to the component's flux parameter"""
    h = np.where(is_point(x, w) | np.isnan(w), 1.0, w)
    b = np.minimum(FLUX_RTOL, 2.0 * PHASE_ATOL / (2.0 * h / nsub) + FLOOR)
    return np.where(is_point(x, w), FLOOR, b)


def assert_points_clear(rec, x, w, a=None, b=None):
    """on the fixture alone: a point evaluation decides by a comparison with
    the contacts, so it must not sit on one"""
    pt = is_point(x, w)
    if not pt.any():
        return
    ph = x[pt] - float(rec["pars"][13])
    ph = ph - np.floor(ph + 0.5)
    a = rec["a"] if a is None else a
    b = rec["b"] if b is None else b
    ecl = a < b
    c = np.concatenate([a[ecl], b[ecl]])
    assert np.min(np.abs(ph[:, None] - c[None, :])) >= POINT_CLEARANCE


def flux_params(rec):
    return [abs(float(v)) for v in rec["pars"][:4]]


def worst(got, ref, x, w, nsub, scale):
    """largest |got - ref| / scale in units of the bound, and plainly; NaN must match NaN"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isnan(ref), np.isnan(w))
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok]) / scale
    return float(np.max(err / bound(x, w, nsub)[ok], initial=0.0)), float(np.max(err, initial=0.0))


def assert_light_curve(label, got5, ref5, x, w, nsub, pars4):
    """the four components, each against its own flux parameter; the total
    against the sum of the four bounds"""
    for k in range(4):
        r, e = worst(got5[1 + k], ref5[1 + k], x, w, nsub, pars4[k])
        assert r <= 1.0, (label, "component %d" % k, e, r)
    r, e = worst(got5[0], ref5[0], x, w, nsub, sum(pars4))
    assert r <= 1.0, (label, "total", e, r)


def assert_geometry(label, m, xl1, inc, bs_x, bs_y, upk, umax, bden):
    """GEO_TOL, relative, or absolute below 1; the inclination also by the
    cos^2 i rule and the beaming denominator with its slope in cos i, as
    tests/test_gpu_parity.py: assert_geo_matches"""
    bad = []
    ci = (np.cos(np.radians(inc)), np.cos(np.radians(m.inc)))
    for name, got, ref in (("xl1", xl1, m.xl1), ("inc", inc, m.inc), ("bs_x", bs_x, m.bs[0]), ("bs_y", bs_y, m.bs[1]),
                           ("upk", upk, m.upk), ("umax", umax, m.umax), ("bden", bden, m.bden)):
        ok = abs(got - ref) <= GEO_TOL * max(1.0, abs(ref))
        if name == "inc" and not ok:
            ok = abs(ci[0] ** 2 - ci[1] ** 2) <= 0.1 * GEO_TOL
        if name == "bden" and not ok:
            ok = abs(got - ref) <= GEO_TOL + 2.0 * abs(ci[0] - ci[1])
        if not ok:
            bad.append((name, float(got), float(ref)))
    assert not bad, (label, bad)


def assert_elements(label, m, st, a, b, wg, don):
    """an implementation's element tables against the double's"""
    assert st == 0, label
    assert np.array_equal(a < b, m.ecl), (label, np.nonzero((a < b) != m.ecl)[0])
    da = np.max(np.abs(a[m.ecl] - m.a[m.ecl]), initial=0.0)
    db = np.max(np.abs(b[m.ecl] - m.b[m.ecl]), initial=0.0)
    assert da <= PHASE_ATOL and db <= PHASE_ATOL, (label, da, db)
    np.testing.assert_allclose(wg, m.w, rtol=1e-12, err_msg=label)
    np.testing.assert_allclose(don, m.donor, rtol=1e-9, atol=1e-14, err_msg=label)   # test_element_tables' rule
    return max(da, db)


def split(pars):
    """CV parameters -> (q, phi0, flux parameters, component parameters by kind)"""
    p = fd.full_pars(pars)
    wdf, df, sf, rsf, q, dphi, rdisc, ul, rwd, scale, az, fis, dexp, phi0, e1, e2, tilt, yaw = p
    return q, phi0, (wdf, df, sf, rsf), {0: [rwd, ul], 1: [rwd, rdisc, dexp],
                                         2: [rdisc, az, fis, scale, e1, e2, tilt, yaw], 3: []}


COMPONENT_GRIDS = {0: (0, 0), 1: (20, 50), 2: (100, 0), 3: (20, 20)}


def double_component(name, kind, x, w, n1=0, n2=0, ab=None):
    """the double's unit component of a recorded set at its inclination"""
    rec = records()[name]
    q, _, _, cps = split(rec["pars"])
    if ab is None and kind != 3:
        ab = (rec["a"][list(fd.SLICES.values())[kind]], rec["b"][list(fd.SLICES.values())[kind]])
    return fd.component(kind, cps[kind], q, float(rec["inc"]), x, w, n1, n2, ab=ab, bs=rec["bs"])


# ------------------------------------------------------ the file is the double's
def test_fixture_holds_the_sets_the_issue_names():
    rec = records()
    assert list(rec) == NAMES
    for name, pars in (("truth18", TRUTH18), ("ecl1", ECL1), ("truth14", TRUTH14)):
        assert np.array_equal(rec[name]["pars"], np.array(pars, dtype=float))
    p = {n: fd.full_pars(rec[n]["pars"]) for n in NAMES}
    assert p["q_above_1"][4] > 1.0 and float(rec["q_above_1"]["inc"]) > 85.0
    assert p["q_above_1"][11] == 0.0 and p["q_above_1"][16] > 90.0 and p["q_above_1"][17] < 0.0
    assert p["q_above_1"][12] == 2.0 and p["q_above_1"][7] == 0.0
    assert abs(p["q_small"][4] - 0.02) < 2e-3 and p["q_small"][11] == 1.0 and p["q_small"][7] == 1.0
    assert p["q_small"][12] == 1.9986 and p["q_small"][15] < 1.0
    assert p["grazing"][5] < 0.015 and p["grazing"][6] >= 0.55
    assert os.path.getsize(GOLD) < 198713     # tests/golden/physpar_ref.npz, the largest before it
    for r in rec.values():
        assert np.array_equal(r["ecl"], r["a"] < r["b"]) and r["a"].shape == (1500,)
    assert isinstance(json.loads(str(np.load(GOLD)["swaps"])), list)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_intervals_are_the_arbiters(name):
    rec = records()[name]
    m = fd.model(rec["pars"], record=rec, positions_only=True)
    rng = np.random.default_rng(NAMES.index(name))
    for k in rng.choice(1500, 16, replace=False):
        ecl, a, b = cd.interval(m.q, m.inc, m.P[k], m.R)
        assert ecl == bool(rec["ecl"][k])
        assert abs(a - rec["a"][k]) <= 1e-12 and abs(b - rec["b"][k]) <= 1e-12, (k, a, b)
        if ecl:   # the rejection rule of tools/make_flux_golden.py
            assert all(cd.resolved(m.q, m.inc, m.P[k], c, PHASE_ATOL, m.R) for c in (a, b))


def test_fixture_extras_are_the_arbiters():
    """the caller-chosen disc grids and the mutated elements of the first set"""
    rec = records()["truth18"]
    q, _, _, cps = split(rec["pars"])
    inc = float(rec["inc"])
    rng = np.random.default_rng(7)
    for npts, (nr, naz) in DISC_GRIDS.items():
        P, _ = fd.component_elements(1, cps[1], q, inc, nr, naz)
        assert len(P) == len(rec["disc%d_a" % npts])
        for k in rng.choice(len(P), 4, replace=False):
            _, a, b = cd.interval(q, inc, P[k])
            assert abs(a - rec["disc%d_a" % npts][k]) <= 1e-12 and abs(b - rec["disc%d_b" % npts][k]) <= 1e-12
    for name, parts in fd.MUT_MOVES.items():
        m = fd.model(rec["pars"], record=rec, mutate=name, positions_only=True)
        lo, hi = fd.SLICES[parts[0]].start, fd.SLICES[parts[-1]].stop
        for k in rng.choice(hi - lo, 3, replace=False):
            _, a, b = cd.interval(q, inc, m.P[lo + k], m.R)
            got = np.array([rec["mut_%s_a" % name][k], rec["mut_%s_b" % name][k]], dtype=float)
            assert np.max(np.abs(got - [a, b])) <= 1e-7      # kept in single precision


def test_fixture_inclination_and_stream_are_the_doubles():
    pytest.importorskip("scipy")
    rec = records()["ecl1"]
    p = fd.full_pars(rec["pars"])
    R = cd.Roche(p[4])
    assert fd.findi(p[4], p[5], R) == float(rec["inc"])
    bs = fd.bspot(p[4], p[6] * R.xl1, R.xl1)
    np.testing.assert_allclose(bs, rec["bs"], rtol=0, atol=1e-13)
    rec = records()["truth18"]
    np.testing.assert_allclose(fd.bspot(TRUTH18[4], TRUTH18[6]), rec["mut_rdisc_in_a_bs"], rtol=0, atol=1e-13)


def test_stream_without_scipy_agrees():
    """the RK4 fallback (step halved until the crossing moves by < 1e-12)"""
    rec = records()["truth18"]
    bs = fd.bspot(TRUTH18[4], TRUTH18[6] * cd.xl1(TRUTH18[4]), use_scipy=False)
    np.testing.assert_allclose(bs[:2], rec["bs"][:2], rtol=0, atol=1e-11)
    np.testing.assert_allclose(bs[2:], rec["bs"][2:], rtol=0, atol=1e-9)


# ------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", NAMES)
def test_oracle_elements(oracle, name):
    m = the_model(name)
    st, a, b, wg, don, geo = oracle.elements(records()[name]["pars"])
    assert_elements(name, m, st, a, b, wg, don)
    assert_geometry(name, m, geo[0], geo[2], geo[5], geo[6], geo[9], geo[10], geo[12])
    np.testing.assert_allclose(geo[7:9], m.bs[2:], rtol=0, atol=1e-11)    # the table's 4e-12 and an integration's
    np.testing.assert_allclose(geo[13], m.dnorm, rtol=1e-12)


@pytest.mark.parametrize("nsub", [1, 3, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_flux(oracle, kind, nsub):
    x, w = grid(kind, 300)
    for name in NAMES:
        rec = records()[name]
        assert_points_clear(rec, x, w)
        st, got = oracle.flux(rec["pars"], x, w, nsub=nsub, components=True)
        assert st == 0
        assert_light_curve((name, kind, nsub), got, double_curve(name, kind, 300, nsub), x, w, nsub, flux_params(rec))


def test_oracle_flux_one_point(oracle):
    for kind in ("regular", "points"):
        x, w = grid(kind, 1)
        for name in NAMES:
            rec = records()[name]
            assert_points_clear(rec, x, w)
            st, got = oracle.flux(rec["pars"], x, w, nsub=3, components=True)
            assert st == 0
            assert_light_curve((name, kind), got, fd.light_curve(the_model(name), x, w, 3), x, w, 3, flux_params(rec))


@pytest.mark.parametrize("kind", ["regular", "wrap", "edges"])
def test_oracle_components(oracle, kind):
    """the unit components at the set's inclination, phases as given"""
    x, w = grid(kind, 300)
    for name in NAMES:
        rec = records()[name]
        q, phi0, _, cps = split(rec["pars"])
        xs = x - phi0
        assert_points_clear(dict(rec, pars=np.zeros(14)), xs, w)
        for k in range(4):
            st, y = oracle.component(k, cps[k], q, float(rec["inc"]), xs, w, *COMPONENT_GRIDS[k])
            assert st == 0
            r, e = worst(y, double_component(name, k, xs, w), xs, w, 1, 1.0)
            assert r <= 1.0, (name, kind, k, e)


@pytest.mark.parametrize("npts", [250, 777])
def test_oracle_components_caller_grids(oracle, npts):
    rec = records()["truth18"]
    q, _, _, cps = split(rec["pars"])
    inc = float(rec["inc"])
    for kind in ("regular", "points"):
        x, w = grid(kind, 300)
        ab = (rec["disc%d_a" % npts], rec["disc%d_b" % npts])
        assert_points_clear(dict(rec, pars=np.zeros(14)), x, w, *ab)
        for k, n12, ab_k in ((1, DISC_GRIDS[npts], ab), (3, DONOR_GRIDS[npts], None)):
            st, y = oracle.component(k, cps[k], q, inc, x, w, *n12)
            assert st == 0
            r, e = worst(y, double_component("truth18", k, x, w, *n12, ab=ab_k), x, w, 1, 1.0)
            assert r <= 1.0, (npts, kind, k, e)


# ---------------------------------------------------------- the CPU twins
@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    return cpu.CpuPort(cpu.build(out=str(tmp_path_factory.mktemp("cpu") / "liblfg_cpu.so")))


def noisy(ref, seed):
    """data = the double's flux plus seeded noise, and its errors"""
    rng = np.random.default_rng(seed)
    ye = np.full(ref.shape, 2e-3)
    return ref + ye * rng.standard_normal(ref.shape), ye


def chisq_bound(y, ye, ref, x, w, nsub, pars4):
    """the flux bound through chi^2 = sum ((y - f) / ye)^2: sum 2 |r| / ye^2 df
    + df^2 / ye^2, and the rounding of the sum itself"""
    df = bound(x, w, nsub) * sum(pars4)
    r = np.abs(y - ref)
    return float(np.sum(2.0 * r / ye ** 2 * df + (df / ye) ** 2)) + 1e-12 * float(np.sum((r / ye) ** 2))


@pytest.mark.parametrize("nsub", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_host_twin_flux_and_lnlike(port, kind, nsub):
    x, w = grid(kind, 300)
    for name in NAMES:
        rec = records()[name]
        assert_points_clear(rec, x, w)
        ref = double_curve(name, kind, 300, nsub)[0]
        flux, st = port.flux(rec["pars"], x, w, nsub=nsub)
        assert st[0] == 0
        r, e = worst(flux[0], ref, x, w, nsub, sum(flux_params(rec)))
        assert r <= 1.0, (name, kind, nsub, e)
        ok = ~np.isnan(w)       # a NaN width makes chi^2 infinite: its own check below
        y, ye = noisy(ref[ok], 11)
        ll, st = port.lnlike(rec["pars"], x[ok], w[ok], y, ye, nsub=nsub)
        want = float(np.sum(((y - ref[ok]) / ye) ** 2))
        assert st[0] == 0 and abs(-2.0 * ll[0] - want) <= chisq_bound(y, ye, ref[ok], x[ok], w[ok], nsub,
                                                                      flux_params(rec)), (name, kind, nsub)
        if not ok.all():
            yy, yye = noisy(np.where(ok, ref, 0.0), 11)
            ll, _ = port.lnlike(rec["pars"], x, w, yy, yye, nsub=nsub)
            assert ll[0] == -np.inf


# -------------------------------------------------------------------- teeth
TOUCHES = {"strip_from_impact": 2, "strip_reversed": 2, "rdisc_in_a": 1, "yaw_sign": 2, "tilt_from_plane": 2,
           "rho_c_mean": 0, "disc_no_half_step": 1, "donor_norm_max": 3}


def miss(mutate, kind, nsub, N=300, ref=None):
    """how far the mutated double of the first set is from `ref` (default: the
    unmutated double), in units of the bound, in the component it touches"""
    x, w = grid(kind, N)
    k = TOUCHES[mutate]
    mut = fd.light_curve(the_model("truth18", mutate), x, w, nsub)[1 + k]
    ref = double_curve("truth18", kind, N, nsub)[1 + k] if ref is None else ref
    ok = ~np.isnan(w)
    return float(np.max(np.abs(mut - ref)[ok] / flux_params(records()["truth18"])[k] / bound(x, w, nsub)[ok]))


@pytest.mark.parametrize("mutate", fd.MUTATIONS)
def test_every_mutation_is_seen(mutate):
    assert set(TOUCHES) == set(fd.MUTATIONS)
    assert miss(mutate, "regular", 1) >= 100.0
