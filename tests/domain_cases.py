"""Parameter populations that cover the whole domain of the light-curve model
(tests/test_domain_sweep.py on the host port, tests/test_gpu_domain.py on the
device, tests/test_contact_double.py for the disputed sets' strips).  Seeded;
each population is built once per session and shared, and its arrays are
read-only.  Every set has 18 parameters in CV order (MODEL_SPEC 1); `simple`
cuts sets down to the 14-parameter form.

    wide_box(n, seed)   the widest box the model accepts
    prior_box(n, seed)  the same, inside what the Roche priors allow (MODEL_SPEC 8)
    DISPUTED            four sets on which the oracle's contacts were wrong
    status_edges()      named sets on either side of every rule of MODEL_SPEC 6
"""
import functools
import math

import numpy as np

from tests.helpers import TRUTH18

OK, BAD_Q, BAD_DPHI, BAD_GEOMETRY, BAD_STREAM, BAD_ARGS = 0, 1, 2, 3, 4, 5   # include/lfg.h LFG_ST_*

# Sets on which the oracle and the host build of the device algorithm differed
# by 2e-6 .. 5e-5 of the flux scale before the oracle's chord scan was mended
# (MODEL_SPEC 4.2): one bright-spot element each whose chord starts next to L1.
D1 = [0.0528,0.0707,0.0613,0.0131,0.3952685078111785,0.0947246919699271,0.9654888173670896,0.8297852952045203,0.01538535815638301,0.056857567738653914,94.24714310515178,0.07598848116007151,1.650282874251356,0.0328170233168711,0.37409526746360633,1.5512961374622176,51.021989746323555,-57.59266067109567]   # table row A, element 1418
D2 = [0.0528,0.0707,0.0613,0.0131,4.030141437263729,0.17033552372829766,0.5966906165798463,0.20134379645159273,0.041925404340279776,0.1629107203298122,53.32768005957503,0.7253639332902304,1.7509017873854313,0.04232767482499823,3.3888604488393814,1.2065836643080505,8.643136215222668,28.140805230587205]    # table row B, element 1429
D3 = [0.0528,0.0707,0.0613,0.0131,0.2827728605757874,0.08624746548857226,0.6832373980142445,0.746647137071686,0.02548921998798372,0.051437136684199414,84.17551211465613,0.6112601800079339,0.030245102046423167,-0.04640347521501456,0.16730586689856344,0.6277167643071249,132.1870750218314,56.6138096050706]   # inside the Roche priors, 2.0e-6
D4 = [0.0528,0.0707,0.0613,0.0131,1.7451494623753858,0.1406148644107974,0.903481183320631,0.6239212740515507,0.017258906082826174,0.03469659504081611,97.07304847257782,0.6544033859747176,0.4846930741022959,-0.026229123706397118,0.21038247849608233,0.7695277841201856,36.89252014055503,80.93510894347236]   # inside the Roche priors, 1.4e-5
DISPUTED = [D1, D2, D3, D4]

Q_LO, Q_HI = 0.003, 8.0
DISC_MAX_A, AZ_SLOPE, DPHI_TOL = 0.46, 80.0, 1e-6   # CVModel.py:217, :282, :452


def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def simple(pars):
    """the 14-parameter (simple bright spot) form of 18-parameter sets"""
    return np.ascontiguousarray(np.asarray(pars, dtype=float)[..., :14])


def _draw(rng, O, priors):
    p = np.array(TRUTH18, dtype=float)
    p[0:4] = rng.uniform(0.005, 0.2, 4)                              # component fluxes
    q = p[4] = math.exp(rng.uniform(math.log(Q_LO), math.log(Q_HI)))
    x1 = O.xl1(q)
    fmax = O.findphi(q, 90.0)
    p[5] = fmax * rng.uniform(1e-3, 1.0 - 1e-6)                      # dphi
    if priors:
        p[5] = min(p[5], fmax - DPHI_TOL)
    p[7] = rng.uniform(0.0, 1.0)                                     # ulimb
    p[8] = rng.uniform(1e-3, 0.1)                                    # rwd
    hi = min(0.99, DISC_MAX_A / x1) if priors else 0.99
    p[6] = rng.uniform(1.05 * p[8], hi)                              # rdisc
    if priors:
        p[9] = p[8] * rng.uniform(1.0 / 3.0, 3.0)                    # scale
    else:
        p[9] = p[8] * math.exp(rng.uniform(math.log(0.1), math.log(10.0)))
    p[10] = rng.uniform(0.0, 360.0)                                  # az
    p[11] = rng.uniform(0.0, 1.0)                                    # fis
    p[12] = rng.uniform(0.0, 2.5)                                    # dexp
    p[13] = rng.uniform(-0.05, 0.05)                                 # phi0
    p[14] = rng.uniform(0.1, 10.0)                                   # exp1
    p[15] = rng.uniform(0.3, 10.0)                                   # exp2
    p[16] = rng.uniform(0.0, 180.0)                                  # tilt
    p[17] = rng.uniform(-180.0, 180.0)                               # yaw
    if priors:
        try:
            x, y = O.bspot(q, p[6] * x1)[:2]
        except ValueError:
            return None                                              # the stream must hit the disc
        alpha = math.degrees(math.atan2(y, x))
        t = 90.0 + alpha if alpha >= 0.0 else 90.0 - alpha           # CVModel.py:276-281
        p[10] = rng.uniform(max(0.0, t - AZ_SLOPE), min(178.0, t + AZ_SLOPE))
    return p


def _box(n, seed, priors):
    O = _oracle()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = _draw(rng, O, priors)
        if p is not None:
            out.append(p)
    out = np.array(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wide_box(n, seed=101):
    """[n, 18]: q log-uniform in [0.003, 8]; dphi a fraction 1e-3 .. 1 - 1e-6
    of findphi(q, 90); rwd in [1e-3, 0.1]; rdisc up to 0.99; scale within a
    factor 10 of rwd; exp1 in [0.1, 10]; exp2 in [0.3, 10]; all angles.  The
    stream misses the disc (status 4) in a part of it."""
    return _box(n, seed, False)


@functools.lru_cache(maxsize=None)
def prior_box(n, seed=202):
    """[n, 18]: wide_box restricted to rdisc xl1 <= 0.46, rwd/3 <= scale <=
    3 rwd, a stream that hits the disc, az within 80 degrees of the tangent
    and dphi <= findphi(q, 90) - 1e-6"""
    return _box(n, seed, True)


def _stream_edges(O, q):
    """(r_min, r0) of the stream at q as the oracle's bspot decides them (units of a)"""
    x1 = O.xl1(q)

    def ok(r):
        try:
            O.bspot(q, r)
            return True
        except ValueError:
            return False
    grid = x1 * np.arange(1, 400) / 400.0
    good = [r for r in grid if ok(r)]
    edges = []
    for bad, inside in ((min(good) - x1 / 400.0, min(good)), (max(good) + x1 / 400.0, max(good))):
        for _ in range(80):
            m = 0.5 * (bad + inside)
            if ok(m):
                inside = m
            else:
                bad = m
        edges.append(0.5 * (bad + inside))
    return edges[0], edges[1]


@functools.lru_cache(maxsize=None)
def status_edges():
    """tuple of (name, pars [18], status MODEL_SPEC 6 demands, complex_only).
    complex_only: the rule is about exp1/exp2, which a 14-parameter set does
    not carry.  Solver-made boundaries (findphi(q, 90), r_min, r0) are taken
    from the oracle and straddled by a relative 1e-9."""
    O = _oracle()
    out = []

    def base(q=None):
        p = np.array(TRUTH18, dtype=float)
        if q is not None:      # a set that is valid at this q: half the widest eclipse, mid-stream disc
            p[4] = q
            p[5] = 0.5 * O.findphi(q, 90.0)
            rmin, r0 = _stream_edges(O, q)
            p[6] = 0.5 * (rmin + r0) / O.xl1(q)
        return p

    def add(name, status, complex_only=False, q=None, **slots):
        p = base(q)
        for k, v in slots.items():
            p[int(k[1:])] = v
        p.setflags(write=False)
        out.append((name, p, status, complex_only))

    add("valid", OK)
    # 1: q
    add("q=0", BAD_Q, s4=0.0)
    add("q=-1", BAD_Q, s4=-1.0)
    # 5: not finite, whichever slot (checked before anything else)
    add("q=nan", BAD_ARGS, s4=math.nan)
    add("q=inf", BAD_ARGS, s4=math.inf)
    add("wdFlux=nan", BAD_ARGS, s0=math.nan)
    add("rdisc=nan", BAD_ARGS, s6=math.nan)
    add("phi0=nan", BAD_ARGS, s13=math.nan)
    # 2: findi
    for q in (0.003, 0.1, 1.0, 6.0):
        f = O.findphi(q, 90.0)
        add("dphi=findphi(%g,90)(1-1e-9)" % q, OK, q=q, s5=f * (1.0 - 1e-9))
        add("dphi=findphi(%g,90)(1+1e-9)" % q, BAD_DPHI, q=q, s5=f * (1.0 + 1e-9))
    add("dphi=0", BAD_DPHI, s5=0.0)
    add("dphi=-0.01", BAD_DPHI, s5=-0.01)
    add("dphi=0.5", BAD_DPHI, s5=0.5)
    # 3: geometry
    rwd = TRUTH18[8]
    add("rwd=0", BAD_GEOMETRY, s8=0.0)
    add("rdisc=rwd(1-1e-12)", BAD_GEOMETRY, s6=rwd * (1.0 - 1e-12))
    add("rdisc=rwd(1+1e-12)", BAD_STREAM, s6=rwd * (1.0 + 1e-12))    # geometry passes; inside periastron
    add("rdisc=1-1e-12", BAD_STREAM, s6=1.0 - 1e-12)                 # geometry passes; beyond the stream's start
    add("rdisc=1+1e-12", BAD_GEOMETRY, s6=1.0 + 1e-12)
    add("scale=0", BAD_GEOMETRY, s9=0.0)
    add("exp1=0", BAD_GEOMETRY, True, s14=0.0)
    add("exp2=0", BAD_GEOMETRY, True, s15=0.0)
    add("exp2=-1", BAD_GEOMETRY, True, s15=-1.0)
    add("exp2=3e-3", BAD_GEOMETRY, True, s15=3e-3)                   # the profile overflows: after the stream
    # 4: the stream, inside the table (q = 0.1037) and on the RK4 path
    for q in (TRUTH18[4], 0.0015, 6.0):
        rmin, r0 = _stream_edges(O, q)
        x1 = O.xl1(q)
        add("q=%g rdisc=rmin(1-1e-9)" % q, BAD_STREAM, q=q, s6=rmin * (1.0 - 1e-9) / x1)
        add("q=%g rdisc=rmin(1+1e-9)" % q, OK, q=q, s6=rmin * (1.0 + 1e-9) / x1)
        add("q=%g rdisc=r0(1-1e-9)" % q, OK, q=q, s6=r0 * (1.0 - 1e-9) / x1)
        add("q=%g rdisc=r0(1+1e-9)" % q, BAD_STREAM, q=q, s6=r0 * (1.0 + 1e-9) / x1)
    # precedence q -> findi -> geometry -> stream -> profile: both rules of a pair fail, the earlier is reported
    add("q=0 & dphi=0.5", BAD_Q, s4=0.0, s5=0.5)
    add("dphi=0.5 & rwd=0", BAD_DPHI, s5=0.5, s8=0.0)
    add("scale=0 & rdisc inside periastron", BAD_GEOMETRY, s9=0.0, s6=rwd * 1.5)
    add("rdisc inside periastron & exp2=3e-3", BAD_STREAM, True, s6=rwd * 1.5, s15=3e-3)
    return tuple(out)
