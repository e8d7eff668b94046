"""An independent double of the GP changepoint distance: MODEL_SPEC 10.2 and
10.3 read literally.

    wdphases(q, inc, r1, ntheta) -> (phi3, phi4, eclipsed limb points) or None
    dist_cp(q, dphi, rwd)        -> (dphi + phi4 - phi3) / 2 or None
    tripped(base, q, dphi, rwd)  -> the 120 % cache rule
    blocks(base, q, dphi, rwd, phi0, ecl0, ecl1) -> [[lo, hi], ...] or None

The limb circle is written out as 10.2 states it; the WD-centre egress phase
and each limb point's egress phase are the contact arbiter's
(tests/contact_double.py: dense chord samples and bisection), the inclination
is the flux double's bisection on the arbiter's findphi.  Nothing here is
shared with oracle/, cpu_baseline/ or the kernels: no Newton iteration, no
envelope, no fast path, and the minimum and maximum are taken in a plain loop
over the points the arbiter calls eclipsed.

About 0.2 s per call at ntheta = 10, seconds per dist_cp (findi): the results
are recorded in tests/golden/wdphases_double.npz (tools/make_wdphases_golden.py).
"""
import math

from tests import contact_double as cd
from tests import flux_double as fd

NTHETA = 10          # CVModel.py:564
RULE = 1.2           # CVModel.py:540-548: |old - new| / new > 1.2

# MODEL_SPEC 6
ST_OK, ST_BAD_Q, ST_BAD_DPHI, ST_BAD_GEOMETRY = 0, 1, 2, 3


def limb_points(inc_deg, r1, ntheta, findphi):
    """10.2: r1 (cos psi_k u1 + sin psi_k u2) at theta_e = pi findphi"""
    s, c = math.sin(math.radians(inc_deg)), math.cos(math.radians(inc_deg))
    th = math.pi * findphi
    u1 = (math.sin(th), math.cos(th), 0.0)
    u2 = (-c * math.cos(th), c * math.sin(th), s)
    out = []
    for k in range(ntheta):
        psi = 2.0 * math.pi * k / ntheta
        out.append(tuple(r1 * (math.cos(psi) * a + math.sin(psi) * b) for a, b in zip(u1, u2)))
    return out


def solve(q, inc_deg, r1, ntheta=NTHETA, all_points=False):
    """(status, phi3, phi4, eclipsed count, P3, P4): P3 / P4 are the limb
    points whose egress is phi3 / phi4.  The status is MODEL_SPEC 6's, in the
    order q -> r1, ntheta -> the eclipse.  all_points: a deliberate slip for
    the tests, the extremes over every limb point (a point never eclipsed
    counts with the arbiter's empty interval's b = -1)."""
    fail = lambda st: (st, math.nan, math.nan, 0, None, None)  # noqa: E731
    if not (q > 0.0 and math.isfinite(q)):
        return fail(ST_BAD_Q)
    if not (r1 > 0.0) or ntheta < 1:
        return fail(ST_BAD_GEOMETRY)
    R = cd.Roche(q)
    width = cd.findphi(q, inc_deg, R)
    if width is None:
        return fail(ST_BAD_DPHI)
    lo = hi = None
    count = 0
    for P in limb_points(inc_deg, r1, ntheta, width):
        ecl, _, b = cd.interval(q, inc_deg, P, R)
        count += bool(ecl)
        if not ecl and not all_points:
            continue
        if lo is None or b < lo[0]:
            lo = (b, P)
        if hi is None or b > hi[0]:
            hi = (b, P)
    if count == 0:
        return fail(ST_BAD_DPHI)
    return ST_OK, lo[0], hi[0], count, lo[1], hi[1]


def wdphases(q, inc_deg, r1, ntheta=NTHETA):
    st, p3, p4, count, _, _ = solve(q, inc_deg, r1, ntheta)
    return (p3, p4, count) if st == ST_OK else None


def dist_cp(q, dphi, rwd, all_points=False):
    """10.3: (dphi + phi4 - phi3) / 2 at i = findi(q, dphi); rwd goes in as r1 unchanged"""
    if not (q > 0.0 and math.isfinite(q)):
        return None
    inc = fd.findi(q, dphi)
    if inc is None:
        return None
    st, p3, p4 = solve(q, inc, rwd, NTHETA, all_points)[:3]
    return (dphi + p4 - p3) / 2.0 if st == ST_OK else None


def tripped(base, q, dphi, rwd):
    """10.3's rule against the cache's (q, dphi, rwd)"""
    return (abs(base[1] - dphi) / dphi > RULE or abs(base[0] - q) / q > RULE or
            abs(base[2] - rwd) / rwd > RULE)


def blocks_of(dcp, phi0, ecl0, ecl1):
    """10.3: for every eclipse number e: [(e - 1) + dist_cp + phi0, (e - dist_cp) + phi0]"""
    return [[((e - 1) + dcp) + phi0, (e - dcp) + phi0] for e in range(ecl0, ecl1 + 1)]


def blocks(base, q, dphi, rwd, phi0, ecl0, ecl1, own=None):
    """base: the cache's (q, dphi, rwd, dist_cp).  A walker that trips the
    rule gets dist_cp from its own values (`own`, when the caller recorded
    it, else computed here); None when that fails."""
    if tripped(base, q, dphi, rwd):
        dcp = dist_cp(q, dphi, rwd) if own is None else own
    else:
        dcp = base[3]
    if dcp is None or not math.isfinite(dcp):
        return None
    return blocks_of(dcp, phi0, ecl0, ecl1)
