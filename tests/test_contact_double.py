"""The oracle's interval solver (lfo_point_interval, MODEL_SPEC 4.3) against
the arbiter of tests/contact_double.py, which shares none of its method:
dense chord samples, bracketing refinement and bisection.

Points A and B are the two contacts at which the oracle's 32-sample scan of a
chord that starts on rising Phi lost the donor's well (MODEL_SPEC 4.2): its
egress came out 6.1e-6 (A) and 5.1e-6 (B) early in phase.  The rest of the
population is where that can happen (chords that start next to L1, the
bright-spot strips of the four disputed sets of tests/domain_cases.py) plus
seeded points in and off the orbital plane over q in [0.003, 8]."""
import functools
import math

import numpy as np
import pytest

from tests import contact_double as cd
from tests.domain_cases import DISPUTED

PHASE_ATOL = 1e-10   # tests/test_gpu_parity.py
FLIP_WIDTH = 1e-6    # test_element_tables_grazing's rule: only a vanishing chord may change class
FLIP_SHARE = 0.01
SEED = 7

A = (0.3952685078111785, 88.89820650536046, (0.57166176, 0.03317, 0.0))
B = (4.030141437263729, 89.9341492609694, (0.27630458, 0.13801451, 0.0))


def spot_points(O, pars, every=1):
    """(q, inc, P) of the bright-spot elements of an 18-parameter set (MODEL_SPEC 5.3)"""
    q, dphi, rdisc, scale, az = pars[4], pars[5], pars[6], pars[9], pars[10]
    e1, e2 = pars[14], pars[15]
    x1 = O.xl1(q)
    inc = O.findi(q, dphi)
    bx, by = O.bspot(q, rdisc * x1)[:2]
    upk = (e1 / e2) ** (1.0 / e2)
    lnpk = e1 * math.log(upk) - upk ** e2
    lo, hi = upk, upk + 1.0          # u_max: ln S(u_pk) - ln S(u) = 16 on u > u_pk
    f = lambda u: lnpk - (e1 * math.log(u) - u ** e2) - 16.0  # noqa: E731
    while f(hi) < 0.0:
        hi *= 2.0
    for _ in range(200):
        m = 0.5 * (lo + hi)
        lo, hi = (m, hi) if f(m) < 0.0 else (lo, m)
    umax = 0.5 * (lo + hi)
    u = (np.arange(100) + 0.5) * umax / 100.0
    off = scale * x1 * (u - upk)
    ca, sa = math.cos(math.radians(az)), math.sin(math.radians(az))
    return [(q, inc, (bx + o * ca, by + o * sa, 0.0)) for o in off[::every]]


def seeded_points(O, n_plane, n_off, n_l1, seed=SEED):
    rng = np.random.default_rng(seed)
    out = []

    def draw_q_inc():
        q = math.exp(rng.uniform(math.log(0.003), math.log(8.0)))
        # findi's range: from the grazing eclipse of the WD centre up to 90 degrees
        x1 = O.xl1(q)
        imin = math.degrees(math.asin(min(1.0, math.sqrt(1.0 - (1.0 - x1) ** 2))))
        return q, x1, rng.uniform(imin, 90.0)

    while len(out) < n_plane:           # in the orbital plane, inside the primary's lobe radius
        q, x1, inc = draw_q_inc()
        r, al = x1 * rng.uniform(0.01, 0.99), rng.uniform(0, 2 * math.pi)
        out.append((q, inc, (r * math.cos(al), r * math.sin(al), 0.0)))
    while len(out) < n_plane + n_off:   # off the plane: the WD's surface and beyond
        q, x1, inc = draw_q_inc()
        r = x1 * rng.uniform(0.001, 0.3)
        v = rng.standard_normal(3)
        v *= r / np.linalg.norm(v)
        out.append((q, inc, tuple(v)))
    while len(out) < n_plane + n_off + n_l1:
        # a chord that starts within 0.05 R_s of L1: P just outside the sphere
        # |X - D| = R_s, within reach of L1, seen from where the ray runs on into the sphere
        q, x1, inc = draw_q_inc()
        inc = rng.uniform(max(inc, 80.0), 90.0)
        Rs = 1.0 - x1
        ang = rng.uniform(-0.12, 0.12)
        d = Rs * (1.0 + rng.uniform(1e-4, 0.05))
        out.append((q, inc, (1.0 - d * math.cos(ang), d * math.sin(ang), 0.0)))
    return out


N_POINTS = 400


@functools.lru_cache(maxsize=None)
def population():
    """(points, the arbiter's (eclipsed, a, b) of each, seeded candidates dropped).
    A seeded candidate is dropped, and the next one drawn, when FP64 cannot
    place one of its contacts within PHASE_ATOL (contact_double.resolved): no
    solver in double precision is right or wrong there.  The named points
    (A, B and the disputed sets' strips) are never dropped."""
    from oracle.oracle import Oracle
    O = Oracle()
    rc = {}

    def arb(pt):
        q, inc, P = pt
        if q not in rc:
            rc[q] = cd.Roche(q)
        return cd.interval(q, inc, P, rc[q])

    pts = [A, B]
    for d in DISPUTED:
        pts += spot_points(O, d, every=5)
    ref = [arb(pt) for pt in pts]
    dropped = 0
    for pt in seeded_points(O, 120, 80, 160):
        if len(pts) == N_POINTS:
            break
        r = arb(pt)
        if r[0] and not all(cd.resolved(pt[0], pt[1], pt[2], x, PHASE_ATOL, rc[pt[0]]) for x in r[1:]):
            dropped += 1
            continue
        pts.append(pt)
        ref.append(r)
    return tuple(pts), tuple(ref), dropped


def test_xl1(oracle):
    for q in (0.003, 0.1037, 1.0, 8.0):
        assert abs(cd.xl1(q) - oracle.xl1(q)) < 1e-15
    assert abs(cd.xl1(1.0) - 0.5) < 1e-16


@pytest.mark.parametrize("name,pt,b_true", [("A", A, 0.156627033), ("B", B, 0.162459473)])
def test_disputed_points(oracle, name, pt, b_true):
    """the two contacts of the issue's table: the arbiter reproduces the
    brute-force roots, and the oracle now agrees with it"""
    ecl, a, b = cd.interval(*pt)
    oe, oa, ob = oracle.point_interval(*pt)
    print("%s: arbiter (%.12f, %.12f)  oracle (%.12f, %.12f)" % (name, a, b, oa, ob))
    assert ecl and oe
    assert abs(b - b_true) < 2e-8   # the table's P has 8 digits: it moves the root by up to ~1e-8
    assert abs(oa - a) <= PHASE_ATOL and abs(ob - b) <= PHASE_ATOL


def test_point_interval_matches_arbiter(oracle):
    pts, ref, dropped = population()
    assert len(pts) == N_POINTS and dropped <= 0.05 * N_POINTS, (len(pts), dropped)
    n_ecl = sum(r[0] for r in ref)
    assert 0.3 * len(pts) < n_ecl < 0.97 * len(pts)      # both classes are populated
    # the share of chords that start next to L1 (within 0.05 R_s, measured on the arbiter's egress ray)
    near = 0
    for (q, inc, P), (ecl, a, b) in zip(pts, ref):
        if not ecl:
            continue
        R = cd.Roche(q)
        s, c = math.sin(math.radians(inc)), math.cos(math.radians(inc))
        th = 2 * math.pi * b
        e = (s * math.cos(th), -s * math.sin(th), c)
        ch = cd.chord(R, P, e)
        if ch is not None:
            X = [P[i] + ch[0] * e[i] for i in range(3)]
            near += math.dist(X, (R.xl1, 0.0, 0.0)) < 0.05 * R.Rs
    assert near >= 40, near
    flips, worst = [], (0.0, None)
    for k, ((q, inc, P), (ecl, a, b)) in enumerate(zip(pts, ref)):
        oe, oa, ob = oracle.point_interval(q, inc, P)
        if oe != ecl:
            width = (b - a) if ecl else (ob - oa)
            assert width < FLIP_WIDTH, (k, q, inc, P, (ecl, a, b), (oe, oa, ob))
            flips.append(k)
            continue
        if ecl:
            d = max(abs(oa - a), abs(ob - b))
            if d > worst[0]:
                worst = (d, k)
    print("%d points (%d candidates dropped as unresolvable in FP64), %d eclipsed, %d with the chord starting next to L1, %d class flips, worst contact difference "
          "%.2e (point %s)" % (len(pts), dropped, n_ecl, near, len(flips), worst[0], worst[1]))
    assert len(flips) <= FLIP_SHARE * len(pts)
    bad = []
    for k, ((q, inc, P), (ecl, a, b)) in enumerate(zip(pts, ref)):
        if ecl and k not in flips:
            oe, oa, ob = oracle.point_interval(q, inc, P)
            if not (abs(oa - a) <= PHASE_ATOL and abs(ob - b) <= PHASE_ATOL):
                bad.append((k, q, inc, P, oa - a, ob - b))
    assert not bad, bad
