"""An arbiter for eclipse contacts: MODEL_SPEC 2, 4.2 and 4.3 read literally.

    interval(q, inc_deg, P) -> (eclipsed, a, b)

g(theta) is the minimum of Phi over the chord of the sphere |X - D| <= R_s,
minus Phi(L1): the chord is sampled densely, and the lowest sample (a chord
end included) is refined by a golden-section search between its neighbours.
A point is eclipsed iff the minimum of g over a theta grid across
|theta - theta_c| < Delta_max (refined the same way) is negative; the
contacts are bisections of g to 1e-12 in phase.  No Newton iteration, no
envelope derivative, no warm start: nothing here can creep, stop early or
keep a stale minimiser, which is how the oracle's and the kernels' solvers
can fail.  x_L1 is a bisection of dPhi/dx in longdouble.  numpy only, tens
of milliseconds per point."""
import math

import numpy as np

NCHORD = 4001        # samples of a chord
NTHETA = 257         # theta grid across the search range
PHASE_TOL = 1e-12    # bisection of the contacts, in phase
_GOLD = 0.5 * (3.0 - math.sqrt(5.0))
TWO_PI = 2.0 * math.pi


def xl1(q):
    """root in (0, 1) of dPhi/dx on the line of centres, bisected in longdouble"""
    q = np.longdouble(q)
    cA = 2 / (1 + q)
    cB = q * cA
    mu = q / (1 + q)
    lo, hi = np.longdouble(0), np.longdouble(1)
    for _ in range(80):
        x = (lo + hi) / 2
        f = cA / (x * x) - cB / ((1 - x) * (1 - x)) - 2 * (x - mu)
        if f > 0:
            lo = x
        else:
            hi = x
    return float((lo + hi) / 2)


class Roche:
    def __init__(self, q):
        self.q = float(q)
        self.cA = 2.0 / (1.0 + q)
        self.cB = q * self.cA
        self.mu = q / (1.0 + q)
        self.xl1 = xl1(q)
        self.Rs = 1.0 - self.xl1
        self.pl1 = float(self.pot(self.xl1, 0.0, 0.0))

    def pot(self, x, y, z):
        r1 = np.sqrt(x * x + y * y + z * z)
        r2 = np.sqrt((x - 1.0) * (x - 1.0) + y * y + z * z)
        return -self.cA / r1 - self.cB / r2 - (x - self.mu) ** 2 - y * y

    def pot1(self, x, y, z):
        """scalar Phi (math, not numpy: the golden-section loops call it)"""
        yz = y * y + z * z
        return (-self.cA / math.sqrt(x * x + yz) - self.cB / math.sqrt((x - 1.0) * (x - 1.0) + yz)
                - (x - self.mu) * (x - self.mu) - y * y)


def _golden(f, lo, hi, flo=None, fhi=None, iters=44):
    """minimum of f over [lo, hi], the ends included: (t, f(t))"""
    a, b = lo, hi
    fa = f(a) if flo is None else flo
    fb = f(b) if fhi is None else fhi
    x1 = a + _GOLD * (b - a)
    x2 = b - _GOLD * (b - a)
    f1, f2 = f(x1), f(x2)
    for _ in range(iters):
        if f1 < f2:
            b, x2, f2 = x2, x1, f1
            x1 = a + _GOLD * (b - a)
            f1 = f(x1)
        else:
            a, x1, f1 = x1, x2, f2
            x2 = b - _GOLD * (b - a)
            f2 = f(x2)
    best = min((fa, lo), (fb, hi), (f1, x1), (f2, x2))
    return best[1], best[0]


def chord(R, P, e):
    """(t_lo, t_hi) of the ray P + t e inside the sphere, or None (4.2)"""
    ux, uy, uz = 1.0 - P[0], -P[1], -P[2]
    tc = ux * e[0] + uy * e[1] + uz * e[2]
    b2 = ux * ux + uy * uy + uz * uz - tc * tc
    if b2 >= R.Rs * R.Rs:
        return None
    h = math.sqrt(R.Rs * R.Rs - b2)
    if tc + h <= 0.0:
        return None
    return max(0.0, tc - h), tc + h


def g(R, P, s, c, th, nchord=NCHORD):
    """min over the chord of Phi, minus Phi(L1); +1 for a missed ray (4.3)"""
    e = (s * math.cos(th), -s * math.sin(th), c)
    ch = chord(R, P, e)
    if ch is None:
        return 1.0
    t = np.linspace(ch[0], ch[1], nchord)
    f = R.pot(P[0] + t * e[0], P[1] + t * e[1], P[2] + t * e[2])
    k = int(np.argmin(f))
    k0, k1 = max(k - 1, 0), min(k + 1, nchord - 1)
    _, fm = _golden(lambda u: R.pot1(P[0] + u * e[0], P[1] + u * e[1], P[2] + u * e[2]),
                    float(t[k0]), float(t[k1]), float(f[k0]), float(f[k1]))
    return min(fm, float(f[k])) - R.pl1


def _bisect(fun, pos, neg):
    """root of fun between pos (fun >= 0) and neg (fun < 0), to PHASE_TOL in phase"""
    while abs(neg - pos) > PHASE_TOL * TWO_PI:
        m = 0.5 * (pos + neg)
        if fun(m) < 0.0:
            neg = m
        else:
            pos = m
    return 0.5 * (pos + neg)


def interval(q, inc_deg, P, R=None):
    """(eclipsed, a, b) of point P, in phase; (False, 1, -1) when never eclipsed"""
    R = R or Roche(q)
    P = tuple(float(v) for v in P)
    s, c = math.sin(math.radians(inc_deg)), math.cos(math.radians(inc_deg))
    ux, uy, uz = 1.0 - P[0], -P[1], -P[2]
    uxy = math.hypot(ux, uy)
    uu = ux * ux + uy * uy + uz * uz
    none = (False, 1.0, -1.0)
    if uu <= R.Rs * R.Rs or uxy <= 0.0 or s <= 0.0:
        return none
    thc = math.atan2(-uy, ux)
    cosD = (math.sqrt(uu - R.Rs * R.Rs) - c * uz) / (s * uxy)
    if not cosD < 1.0:
        return none
    Dm = math.pi if cosD <= -1.0 else math.acos(cosD)
    fun = lambda th: g(R, P, s, c, th)  # noqa: E731
    grid = np.linspace(thc - Dm, thc + Dm, NTHETA)
    gv = np.array([g(R, P, s, c, th, 801) for th in grid])
    k = int(np.argmin(gv))
    neg = np.nonzero(gv < 0.0)[0]
    if len(neg) == 0:
        # the eclipse, if any, is narrower than the grid: refine the minimum
        k0, k1 = max(k - 1, 0), min(k + 1, NTHETA - 1)
        thm, gm = _golden(fun, float(grid[k0]), float(grid[k1]))
        if not gm < 0.0:
            return none
        return True, _bisect(fun, float(grid[k0]), thm) / TWO_PI, _bisect(fun, float(grid[k1]), thm) / TWO_PI
    i0, i1 = int(neg[0]), int(neg[-1])
    # the grid's g uses a coarser chord: confirm the bracket ends with the fine one
    lo_in, hi_in = float(grid[i0]), float(grid[i1])
    if not fun(lo_in) < 0.0 or not fun(hi_in) < 0.0:
        thm, gm = _golden(fun, float(grid[max(i0 - 1, 0)]), float(grid[min(i1 + 1, NTHETA - 1)]))
        if not gm < 0.0:
            return none
        lo_in = hi_in = thm
    lo_out = float(grid[i0 - 1]) if i0 > 0 else thc - Dm
    hi_out = float(grid[i1 + 1]) if i1 < NTHETA - 1 else thc + Dm
    return True, _bisect(fun, lo_out, lo_in) / TWO_PI, _bisect(fun, hi_out, hi_in) / TWO_PI


def resolved(q, inc_deg, P, contact, tol, R=None):
    """whether FP64 can place this contact (a phase from `interval`) within
    `tol`: g must leave the rounding noise of Phi, 16 ulp of Phi(L1), within
    tol/2 on both sides of it.  Where a line of sight leaves the lobe next to
    L1, g'(theta) -> 0 (the lobe ends in a cone there) and one ulp of Phi can
    be 1e-9 in phase: no FP64 solver, this one included, pins such a contact."""
    R = R or Roche(q)
    P = tuple(float(v) for v in P)
    s, c = math.sin(math.radians(inc_deg)), math.cos(math.radians(inc_deg))
    floor = 16.0 * np.spacing(abs(R.pl1))
    th = TWO_PI * contact
    return all(abs(g(R, P, s, c, th + d)) > floor for d in (-0.5 * tol * TWO_PI, 0.5 * tol * TWO_PI))


def findphi(q, inc_deg, R=None):
    """full phase width of the eclipse of the WD centre (4.4); None when not eclipsed"""
    ecl, a, b = interval(q, inc_deg, (0.0, 0.0, 0.0), R)
    return 2.0 * b if ecl else None
