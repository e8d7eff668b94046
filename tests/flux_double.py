"""A double of the flux arithmetic: MODEL_SPEC 1-5 read literally, in numpy.

    m = model(pars, record=None, mutate=None)   the 1 500 elements, the donor, the geometry
    total, ywd, yd, ys, yrs = light_curve(m, x, w, nsub)
    y = component(kind, cp, q, inc, x, w, n1, n2, ab=None)    the unit components of 5.6

Nothing here is shared with oracle/, lfit_python_amd/ or cpu_baseline/: x_L1,
Phi and the eclipse intervals come from the contact arbiter
(tests/contact_double.py), the inclination is a bisection on the arbiter's
findphi, the stream is integrated here (scipy's DOP853, or RK4 with step
halving), every other root is a bisection, and the light curve is the plain
element x sub-bin x point array.  No mirror symmetry, no breakpoint table, no
closed-form sub-bin sum.

The arbiter costs tens of milliseconds per element, so `record` (one set of
tests/golden/flux_double.npz, tools/make_flux_golden.py) carries what is slow:
the intervals, the inclination and the stream's impact point.  Positions,
weights, the strip's constants, the beaming and the donor are recomputed here
every time.

`mutate` flips one convention (MUTATIONS); the tests use it to show that they
would notice.  A mutated model takes its intervals from record["mut_<name>"]
(kept in single precision: they only have to show a miss) or from the arbiter.
"""
import math

import numpy as np

from tests import contact_double as cd

NWD_RINGS, NWD = 10, 400
NDISC_R, NDISC_AZ = 20, 50
NBS = 100
NDONOR_T, NDONOR_P = 20, 20
BS_TAIL = 16.0
STREAM_DELTA = 1e-2
TWO_PI = 2.0 * math.pi

MUTATIONS = ("strip_from_impact", "strip_reversed", "rdisc_in_a", "yaw_sign", "tilt_from_plane",
             "rho_c_mean", "disc_no_half_step", "donor_norm_max")
# the elements whose position a mutation moves (slices of the element table);
# the others keep the record's intervals
MUT_MOVES = {"strip_from_impact": ("bs",), "strip_reversed": ("bs",), "rdisc_in_a": ("disc", "bs"),
             "rho_c_mean": ("wd",), "disc_no_half_step": ("disc",)}
SLICES = {"wd": slice(0, NWD), "disc": slice(NWD, NWD + NDISC_R * NDISC_AZ),
          "bs": slice(NWD + NDISC_R * NDISC_AZ, NWD + NDISC_R * NDISC_AZ + NBS)}


def full_pars(pars):
    """the 18 values; 14 select the simple spot (MODEL_SPEC 1)"""
    p = [float(v) for v in pars]
    if len(p) == 14:
        p += [2.0, 1.0, 90.0, 0.0]
    assert len(p) == 18
    return p


# ---------------------------------------------------------------- geometry
def grad_pot(R, x, y, z):
    """grad Phi of MODEL_SPEC 2 (arrays)"""
    r1 = np.sqrt(x * x + y * y + z * z) ** 3
    r2 = np.sqrt((x - 1.0) ** 2 + y * y + z * z) ** 3
    return (R.cA * x / r1 + R.cB * (x - 1.0) / r2 - 2.0 * (x - R.mu),
            R.cA * y / r1 + R.cB * y / r2 - 2.0 * y,
            R.cA * z / r1 + R.cB * z / r2)


def findphi_fine(q, inc_deg, R):
    """the arbiter's findphi, its egress then bisected on the arbiter's g
    down to the spacing of the doubles (the arbiter stops at 1e-12 in phase,
    which would leave cos^2 i known to 4e-13 only)"""
    ecl, _, b = cd.interval(q, inc_deg, (0.0, 0.0, 0.0), R)
    if not ecl:
        return 0.0
    s, c = math.sin(math.radians(inc_deg)), math.cos(math.radians(inc_deg))
    P = (0.0, 0.0, 0.0)
    d = 4.0 * cd.PHASE_TOL * TWO_PI
    inside, outside = TWO_PI * b - d, TWO_PI * b + d
    assert cd.g(R, P, s, c, inside) < 0.0 <= cd.g(R, P, s, c, outside)
    for _ in range(60):
        m = 0.5 * (inside + outside)
        if m == inside or m == outside:
            break
        if cd.g(R, P, s, c, m) < 0.0:
            inside = m
        else:
            outside = m
    return 2.0 * (0.5 * (inside + outside)) / TWO_PI


def findi(q, dphi, R=None):
    """the inclination (degrees) whose WD-centre eclipse is dphi wide
    (MODEL_SPEC 4.4), by bisection; None when no inclination gives it"""
    R = R or cd.Roche(q)
    if not (0.0 < dphi < 0.5) or dphi >= findphi_fine(q, 90.0, R):
        return None
    lo, hi = 0.0, 90.0      # findphi is 0 at lo (not eclipsed) and grows with the inclination
    for _ in range(200):
        m = 0.5 * (lo + hi)
        if m == lo or m == hi:
            break
        if findphi_fine(q, m, R) < dphi:
            lo = m
        else:
            hi = m
    return 0.5 * (lo + hi)


# ------------------------------------------------------------- stream (4.5)
def _stream_rhs(q):
    m1, m2 = 1.0 / (1.0 + q), q / (1.0 + q)

    def rhs(_t, s):
        x, y, vx, vy = s
        r1 = (x * x + y * y) ** 1.5
        r2 = ((x - 1.0) ** 2 + y * y) ** 1.5
        ux = m1 * x / r1 + m2 * (x - 1.0) / r2 - (x - m2)     # dU/dx, U = Phi/2
        uy = m1 * y / r1 + m2 * y / r2 - y
        return np.array([vx, vy, -ux + 2.0 * vy, -uy - 2.0 * vx])
    return rhs


def stream_start(q, x1):
    """X0 = L1 + d v + d^2 w on the unstable manifold (MODEL_SPEC 4.5): v the
    unstable eigenvector of the linearised flow at L1, of unit length in
    position and pointing at the WD; (2 lam I - A) w = N2(v)"""
    m1, m2 = 1.0 / (1.0 + q), q / (1.0 + q)
    K = m1 / x1 ** 3 + m2 / (1.0 - x1) ** 3
    uxx, uyy = -2.0 * K - 1.0, K - 1.0
    A = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0], [-uxx, 0.0, 0.0, 2.0], [0.0, -uyy, -2.0, 0.0]])
    ev, vec = np.linalg.eig(A)
    k = int(np.argmax(ev.real))
    assert abs(ev[k].imag) < 1e-12 and ev[k].real > 0.0
    lam = float(ev[k].real)
    v = vec[:, k].real
    v = v / math.hypot(v[0], v[1])
    if v[0] > 0.0:
        v = -v
    uxxx = 6.0 * m1 / x1 ** 4 - 6.0 * m2 / (1.0 - x1) ** 4
    uxyy = -0.5 * uxxx
    n2 = np.array([0.0, 0.0, -0.5 * (uxxx * v[0] ** 2 + uxyy * v[1] ** 2), -uxyy * v[0] * v[1]])
    w = np.linalg.solve(2.0 * lam * np.eye(4) - A, n2)
    return np.array([x1, 0.0, 0.0, 0.0]) + STREAM_DELTA * v + STREAM_DELTA ** 2 * w


def _rk4_step(rhs, s, h):
    k1 = rhs(0.0, s)
    k2 = rhs(0.0, s + 0.5 * h * k1)
    k3 = rhs(0.0, s + 0.5 * h * k2)
    k4 = rhs(0.0, s + h * k3)
    return s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def _bspot_rk4(rhs, s0, rad, dt):
    """RK4 at the fixed step dt; the crossing inside the last step by
    bisection on the length of a shortened step"""
    s, rmin = np.array(s0, dtype=float), math.inf
    for _ in range(int(60.0 / dt)):
        nxt = _rk4_step(rhs, s, dt)
        r = math.hypot(nxt[0], nxt[1])
        if r <= rad:
            lo, hi = 0.0, dt
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                t = _rk4_step(rhs, s, mid)
                if math.hypot(t[0], t[1]) > rad:
                    lo = mid
                else:
                    hi = mid
            return _rk4_step(rhs, s, 0.5 * (lo + hi))
        if r > rmin + 0.05:
            return None          # past the periastron and on its way out
        rmin, s = min(rmin, r), nxt
    return None


def bspot(q, rad, x1=None, use_scipy=True):
    """(x, y, vx, vy) where the stream first reaches radius rad; None when it
    does not (rad at or beyond the start, or inside the periastron)"""
    x1 = cd.xl1(q) if x1 is None else x1
    rhs = _stream_rhs(q)
    s0 = stream_start(q, x1)
    if not (0.0 < rad < x1) or not rad < math.hypot(s0[0], s0[1]):
        return None
    solve_ivp = None
    if use_scipy:
        try:
            from scipy.integrate import solve_ivp
        except ImportError:
            pass
    if solve_ivp is None:
        dt, last = 4e-3, None
        while True:
            s = _bspot_rk4(rhs, s0, rad, dt)
            if s is None:
                return None
            if last is not None and np.max(np.abs(s[:2] - last[:2])) < 1e-12:
                return tuple(float(v) for v in s)
            last, dt = s, 0.5 * dt
    kw = dict(method="DOP853", rtol=2.3e-14, atol=1e-18)

    def hit(_t, s):
        return math.hypot(s[0], s[1]) - rad
    hit.terminal, hit.direction = True, -1.0
    sol = solve_ivp(rhs, (0.0, 60.0), s0, events=hit, **kw)
    if len(sol.t_events[0]) == 0:
        return None
    # the crossing time by Newton on r(t) - rad, each state integrated afresh
    # from X0: no interpolant in the answer
    t = float(sol.t_events[0][0])
    for _ in range(6):
        s = solve_ivp(rhs, (0.0, t), s0, **kw).y[:, -1]
        r = math.hypot(s[0], s[1])
        step = (r - rad) * r / (s[0] * s[2] + s[1] * s[3])
        t -= step
        if abs(step) < 1e-15:
            break
    return tuple(float(v) for v in solve_ivp(rhs, (0.0, t), s0, **kw).y[:, -1])


# ------------------------------------------------------------ elements (5)
def wd_tiles(rwd_a, ulimb, s, c, mutate=None):
    """5.1: positions [400, 3] and weights [400], ring by ring from the centre"""
    P, W = [], []
    F = lambda rho: (1.0 - ulimb) * rho * rho / 2.0 - ulimb * (1.0 - rho * rho) ** 1.5 / 3.0   # noqa: E731
    for k in range(NWD_RINGS):
        r0, r1 = k / NWD_RINGS, (k + 1) / NWD_RINGS
        n = 4 * (2 * k + 1)
        rc = 0.5 * (r0 + r1) if mutate == "rho_c_mean" else math.sqrt((r0 * r0 + r1 * r1) / 2.0)
        z = math.sqrt(1.0 - rc * rc)
        for j in range(n):
            psi = TWO_PI * (j + 0.5) / n
            yh = rc * math.cos(psi)          # along y
            up = rc * math.sin(psi)          # along (-c, 0, s)
            P.append((rwd_a * (up * -c + z * s), rwd_a * yh, rwd_a * (up * s + z * c)))
            W.append((TWO_PI / n) * (F(r1) - F(r0)))
    return np.array(P), np.array(W)


def disc_elements(rwd_a, rdisc_a, dexp, nr=NDISC_R, naz=NDISC_AZ, mutate=None):
    """5.2: ring-major from the inner ring, azimuth ascending"""
    P, W = [], []
    ex = 2.0 - dexp
    for k in range(nr):
        r0 = rwd_a + (rdisc_a - rwd_a) * k / nr
        r1 = rwd_a + (rdisc_a - rwd_a) * (k + 1) / nr
        lr = math.log(r1 / r0)
        integral = lr if ex == 0.0 else r0 ** ex * math.expm1(ex * lr) / ex
        rm = 0.5 * (r0 + r1)
        for j in range(naz):
            al = TWO_PI * (j if mutate == "disc_no_half_step" else j + 0.5) / naz
            P.append((rm * math.cos(al), rm * math.sin(al), 0.0))
            W.append((TWO_PI / naz) * integral)
    return np.array(P), np.array(W)


def strip_profile(exp1, exp2):
    """u_pk, and u_max from ln S(u_pk) - ln S(u) = 16 on u > u_pk, bisected"""
    lnS = lambda u: exp1 * math.log(u) - u ** exp2     # noqa: E731
    upk = (exp1 / exp2) ** (1.0 / exp2)
    f = lambda u: lnS(upk) - lnS(u) - BS_TAIL          # noqa: E731
    lo, hi = upk, 2.0 * upk + 1.0
    while f(hi) < 0.0:
        hi *= 2.0
    for _ in range(300):
        m = 0.5 * (lo + hi)
        if m == lo or m == hi:
            break
        if f(m) < 0.0:
            lo = m
        else:
            hi = m
    return upk, 0.5 * (lo + hi)


def strip_elements(bs_xy, l, az_deg, exp1, exp2, n=NBS, mutate=None):
    """5.3: the strip through the impact point, its peak on it"""
    upk, umax = strip_profile(exp1, exp2)
    ca, sa = math.cos(math.radians(az_deg)), math.sin(math.radians(az_deg))
    P, W = [], []
    for k in range(n):
        u = (k + 0.5) * umax / n
        off = l * (u - upk)
        if mutate == "strip_from_impact":
            off = l * u
        elif mutate == "strip_reversed":
            off = -off
        P.append((bs_xy[0] + off * ca, bs_xy[1] + off * sa, 0.0))
        # S(u) / S(u_pk)
        W.append(math.exp(exp1 * math.log(u) - u ** exp2 - (exp1 * math.log(upk) - upk ** exp2)))
    return np.array(P), np.array(W), upk, umax


def beaming(az_deg, fis, tilt_deg, yaw_deg, s, c, mutate=None):
    """5.3: the beaming direction n and the denominator of B"""
    if mutate == "yaw_sign":
        yaw_deg = -yaw_deg
    if mutate == "tilt_from_plane":
        tilt_deg = 90.0 - tilt_deg
    t, psi = math.radians(tilt_deg), math.radians(az_deg - 90.0 + yaw_deg)
    n = (math.sin(t) * math.cos(psi), math.sin(t) * math.sin(psi), math.cos(t))
    den = fis + (1.0 - fis) * max(0.0, abs(math.sin(t)) * s + math.cos(t) * c)
    return n, den


def donor_tiles(R, nt=NDONOR_T, nph=NDONOR_P):
    """5.4: dA n of every tile, [nt * nph, 3], band-major from the band at L1.
    theta' runs from the direction of L1 in nt equal bands, phi' from +y
    towards +z in nph equal steps, a tile's centre at the middle of both."""
    V = []
    for it in range(nt):
        t0, t1 = math.pi * it / nt, math.pi * (it + 1) / nt
        tc = 0.5 * (t0 + t1)
        dom = (math.cos(t0) - math.cos(t1)) * TWO_PI / nph
        for ip in range(nph):
            ph = TWO_PI * (ip + 0.5) / nph
            d = (-math.cos(tc), math.sin(tc) * math.cos(ph), math.sin(tc) * math.sin(ph))
            lo, hi = 0.0, R.Rs       # Phi - Phi(L1) < 0 towards D, >= 0 at R_s
            for _ in range(200):
                m = 0.5 * (lo + hi)
                if m == lo or m == hi:
                    break
                if R.pot1(1.0 + m * d[0], m * d[1], m * d[2]) - R.pl1 < 0.0:
                    lo = m
                else:
                    hi = m
            r = 0.5 * (lo + hi)
            g = np.array([float(v) for v in grad_pot(R, 1.0 + r * d[0], r * d[1], r * d[2])])
            nrm = g / math.sqrt(float(g @ g))
            dA = r * r * dom / float(nrm @ np.array(d))
            V.append(dA * nrm)
    return np.array(V)


def line_of_sight(s, c, ph):
    th = TWO_PI * np.asarray(ph)
    return s * np.cos(th), -s * np.sin(th), c + 0.0 * th


def donor_light(V, s, c, ph):
    """sum over tiles of max(0, dA n . e) at phases ph"""
    e0, e1, e2 = line_of_sight(s, c, ph)
    v = V[:, 0, None] * e0[None, :] + V[:, 1, None] * e1[None, :] + V[:, 2, None] * e2[None, :]
    return np.sum(np.maximum(v, 0.0), axis=0)


def donor_norm(V, s, c, mutate=None):
    if mutate == "donor_norm_max":
        return float(np.max(donor_light(V, s, c, np.linspace(-0.5, 0.5, 2001))))
    return float(donor_light(V, s, c, np.array([0.25]))[0])


def intervals(q, inc, P, R=None):
    """the arbiter at every position: (a, b), (1, -1) where never eclipsed"""
    R = R or cd.Roche(q)
    a, b = np.ones(len(P)), -np.ones(len(P))
    for k, p in enumerate(P):
        ecl, ak, bk = cd.interval(q, inc, p, R)
        if ecl:
            a[k], b[k] = ak, bk
    return a, b


# ------------------------------------------------------------------- model
class Model:
    pass


def model(pars, record=None, mutate=None, positions_only=False):
    """the CV model of MODEL_SPEC 5 for 14 or 18 parameters.  `record` is a
    dict with inc, bs (x, y, vx, vy), a, b [1500] (and mut_<name>_a/_b,
    mut_rdisc_in_a_bs for mutated models); without it the arbiter and the
    stream integration run here."""
    assert mutate is None or mutate in MUTATIONS
    p = full_pars(pars)
    m = Model()
    m.pars = p
    (m.wdFlux, m.dFlux, m.sFlux, m.rsFlux, q, dphi, rdisc, ulimb, rwd, scale, az, fis, dexp, m.phi0,
     exp1, exp2, tilt, yaw) = p
    m.q, m.R = q, cd.Roche(q)
    m.xl1 = m.R.xl1
    m.inc = float(record["inc"]) if record is not None else findi(q, dphi, m.R)
    assert m.inc is not None, "no inclination for dphi"
    m.s, m.c = math.sin(math.radians(m.inc)), math.cos(math.radians(m.inc))
    m.rwd_a = rwd * m.xl1
    m.rdisc_a = rdisc if mutate == "rdisc_in_a" else rdisc * m.xl1
    m.l = scale * m.xl1
    if record is None:
        m.bs = bspot(q, m.rdisc_a, m.xl1)
    elif mutate == "rdisc_in_a":
        m.bs = tuple(float(v) for v in record["mut_rdisc_in_a_bs"])
    else:
        m.bs = tuple(float(v) for v in record["bs"])
    assert m.bs is not None, "the stream misses the disc"
    Pw, Ww = wd_tiles(m.rwd_a, ulimb, m.s, m.c, mutate)
    Pd, Wd = disc_elements(m.rwd_a, m.rdisc_a, dexp, mutate=mutate)
    Pb, Wb, m.upk, m.umax = strip_elements(m.bs[:2], m.l, az, exp1, exp2, mutate=mutate)
    m.P = np.vstack([Pw, Pd, Pb])
    m.w = np.concatenate([Ww, Wd, Wb])
    m.fis = fis
    m.nb, m.bden = beaming(az, fis, tilt, yaw, m.s, m.c, mutate)
    m.donor = donor_tiles(m.R)
    m.dnorm = donor_norm(m.donor, m.s, m.c, mutate)
    if positions_only:
        return m
    if record is None:
        m.a, m.b = intervals(q, m.inc, m.P, m.R)
    else:
        m.a, m.b = np.array(record["a"], dtype=float), np.array(record["b"], dtype=float)
        parts = MUT_MOVES.get(mutate, ())
        if parts:   # the moved elements are one stretch of the table
            lo, hi = SLICES[parts[0]].start, SLICES[parts[-1]].stop
            m.a[lo:hi] = record["mut_%s_a" % mutate]
            m.b[lo:hi] = record["mut_%s_b" % mutate]
    m.ecl = m.a < m.b
    return m


# ------------------------------------------------------------- light curve
def sub_bins(x, w, nsub):
    """sub-bin centres reduced to [-1/2, 1/2) and half-widths, [N, S]
    (MODEL_SPEC 3); a negative width is a zero one; NaN stays NaN"""
    x, w = np.asarray(x, dtype=float), np.asarray(w, dtype=float)
    w = np.where(w < 0.0, 0.0, w)
    h = w / nsub
    j = np.arange(nsub)
    ph = x[:, None] - w[:, None] + (2 * j[None, :] + 1) * h[:, None]
    ph = ph - np.floor(ph + 0.5)
    return ph, np.broadcast_to(h[:, None], ph.shape)


def visibility(a, b, ph, h):
    """1 - overlap([ph - h, ph + h], [a, b]) / 2h, element x sub-bin; a
    window with no extent (h = 0, or ph + h == ph - h) is a point evaluation"""
    a, b = a[:, None], b[:, None]
    ph, h = ph[None, :], h[None, :]
    lo, hi = ph - h, ph + h
    with np.errstate(invalid="ignore", divide="ignore"):
        ov = np.maximum(np.minimum(b, hi) - np.maximum(a, lo), 0.0)
        window = 1.0 - ov / (2.0 * h)
    point = np.where((ph > a) & (ph < b), 0.0, 1.0)
    return np.where((h > 0.0) & (hi > lo), window, point)


def _series(a, b, wgt, ph, h):
    """sum_i w_i vis_i / sum_i w_i over the sub-bins ph [N, S] -> [N, S]"""
    v = visibility(a, b, ph.reshape(-1), h.reshape(-1))
    return (wgt @ v / np.sum(wgt)).reshape(ph.shape)


def _beam(nb, bden, fis, s, c, ph):
    if not bden > 0.0:
        return np.zeros_like(ph)
    e0, e1, e2 = line_of_sight(s, c, ph)
    return (fis + (1.0 - fis) * np.maximum(0.0, nb[0] * e0 + nb[1] * e1 + nb[2] * e2)) / bden


def light_curve(m, x, w, nsub=1):
    """(total, ywd, yd, ys, yrs), the components scaled by their flux parameters"""
    x = np.asarray(x, dtype=float)
    w = np.zeros_like(x) if w is None else np.asarray(w, dtype=float)
    ph, h = sub_bins(x - m.phi0, w, nsub)
    out = []
    for part, flux in (("wd", m.wdFlux), ("disc", m.dFlux), ("bs", m.sFlux)):
        sl = SLICES[part]
        y = _series(m.a[sl], m.b[sl], m.w[sl], ph, h)
        if part == "bs":
            y = y * _beam(m.nb, m.bden, m.fis, m.s, m.c, ph)
        out.append(flux * np.mean(y, axis=1))
    yr = donor_light(m.donor, m.s, m.c, ph.reshape(-1)).reshape(ph.shape) / m.dnorm
    out.append(m.rsFlux * np.mean(yr, axis=1))
    nan = np.isnan(w)
    out = [np.where(nan, np.nan, y) for y in out]
    return [out[0] + out[1] + out[2] + out[3]] + out


def component_elements(kind, cp, q, inc, n1=0, n2=0, bs=None, R=None):
    """positions and weights of a unit component (5.6); kind 0 WD (rwd,
    ulimb), 1 disc (rwd, rdisc, dexp), 2 spot (rdisc, az, fis, scale, exp1,
    exp2, tilt, yaw; bs = the impact point)"""
    R = R or cd.Roche(q)
    s, c = math.sin(math.radians(inc)), math.cos(math.radians(inc))
    if kind == 0:
        return wd_tiles(cp[0] * R.xl1, cp[1], s, c)
    if kind == 1:
        return disc_elements(cp[0] * R.xl1, cp[1] * R.xl1, cp[2], n1 or NDISC_R, n2 or NDISC_AZ)
    bs = bs if bs is not None else bspot(q, cp[0] * R.xl1, R.xl1)
    P, W, _, _ = strip_elements(bs[:2], cp[3] * R.xl1, cp[1], cp[4], cp[5], n1 or NBS)
    return P, W


def component(kind, cp, q, inc, x, w=None, n1=0, n2=0, ab=None, bs=None):
    """the unit-normalised component of 5.6 at inclination inc (degrees),
    phases used as given, S = 1.  ab = (a, b) of its elements (else the
    arbiter runs); the donor (kind 3) has none."""
    R = cd.Roche(q)
    s, c = math.sin(math.radians(inc)), math.cos(math.radians(inc))
    x = np.asarray(x, dtype=float)
    w = np.zeros_like(x) if w is None else np.asarray(w, dtype=float)
    ph, h = sub_bins(x, w, 1)
    if kind == 3:
        V = donor_tiles(R, n1 or NDONOR_T, n2 or NDONOR_P)
        y = donor_light(V, s, c, ph[:, 0]) / donor_norm(V, s, c)
    else:
        P, W = component_elements(kind, cp, q, inc, n1, n2, bs, R)
        a, b = ab if ab is not None else intervals(q, inc, P, R)
        y = _series(np.asarray(a, dtype=float), np.asarray(b, dtype=float), W, ph, h)[:, 0]
        if kind == 2:
            nb, bden = beaming(cp[1], cp[2], cp[6], cp[7], s, c)
            y = y * _beam(nb, bden, cp[2], s, c, ph[:, 0])
    return np.where(np.isnan(w), np.nan, y)
