#!/usr/bin/env python
"""tests/golden/wdphases_double.npz: the changepoint double
(tests/wdphases_double.py) on a seeded population, recorded once because a row
costs seconds (findi by bisection on the arbiter, then ten limb points).

    python tools/make_wdphases_golden.py [--seed 3] [--workers 16] [--out ...]

Rows (MODEL_SPEC 10.2, 10.3):
  seeded   N_SEEDED rows: q log-uniform in the domain sweep's [0.003, 8], dphi
           uniform in (0.002, 0.95 findphi(q, 90)), inc = findi(q, dphi), r1
           log-uniform in [1e-3, 0.1]
  edge     EDGES below: inc = 90 exactly, an inclination just below the
           grazing one (the centre is not eclipsed: failure), r1 = 0, r1 < 0,
           r1 = NaN, grazing geometries with phi3 < 0 and with part of the
           limb never eclipsed
  ntheta   the first N_NTHETA seeded rows and every finite edge row again at
           ntheta = 1, 2, 3, 7, 16 (N_SUBSET rows each)

Per row: q, inc, r1, ntheta, dphi (NaN where the row sets inc itself), the
double's status (MODEL_SPEC 6), phi3, phi4, the number of eclipsed limb
points, and contact_double.resolved at 1e-10 for the two contacts.  Under
rule_*: the double's dist_cp of the rows tests/gp_trees.py's rule family
designates (rule_values()).  Computes with the double, the arbiter and the
flux double's findi only.
"""
import argparse
import math
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import contact_double as cd      # noqa: E402
from tests import flux_double as fd         # noqa: E402
from tests import wdphases_double as wd     # noqa: E402

PHASE_ATOL = 1e-10
SEED = 3
N_SEEDED = 160
N_SUBSET = 24
NTHETAS = (1, 2, 3, 7, 16)
Q_RANGE = (0.003, 8.0)
R1_RANGE = (1e-3, 0.1)
BELOW_GRAZING = 1e-3     # degrees

# (name, q, dphi or None, inc or None / "below_grazing", r1)
EDGES = [
    ("inc_90", 0.1037, None, 90.0, 0.0187),
    ("inc_90_q_above_1", 2.5, None, 90.0, 0.05),
    ("below_grazing", 0.1037, None, "below_grazing", 0.03),
    ("below_grazing_q_above_1", 1.6, None, "below_grazing", 0.05),
    ("r1_zero", 0.1037, 0.0392, None, 0.0),
    ("r1_negative", 0.1037, 0.0392, None, -0.0187),
    ("r1_nan", 0.1037, 0.0392, None, math.nan),
    ("phi3_negative", 0.1037, 0.003, None, 0.03),
    ("partial_6", 0.1037, 0.0392 / 2.3, None, 0.0187),
    ("partial_5", 0.5, 0.004, None, 0.05),
    ("example", 0.1037, 0.0392, None, 0.0187),
]
N_NTHETA = N_SUBSET - sum(1 for e in EDGES if not (e[4] != e[4] or e[4] <= 0.0 or e[3] == "below_grazing"))


def grazing_inclination(q):
    """the inclination below which the WD centre is never eclipsed, bisected on the arbiter"""
    R = cd.Roche(q)
    lo, hi = 0.0, 90.0
    for _ in range(60):
        m = 0.5 * (lo + hi)
        if cd.findphi(q, m, R) is None:
            lo = m
        else:
            hi = m
    return lo


def _inputs(job):
    """(q, dphi or None, inc or None / "below_grazing", r1) -> (q, inc, r1, dphi)"""
    q, dphi, inc, r1 = job
    if inc == "below_grazing":
        return q, grazing_inclination(q) - BELOW_GRAZING, r1, math.nan
    if inc is None:
        inc = fd.findi(q, dphi)
        assert inc is not None, job
        return q, inc, r1, dphi
    return q, inc, r1, math.nan


def _row(job):
    q, inc, r1, ntheta = job
    st, p3, p4, count, P3, P4 = wd.solve(q, inc, r1, ntheta)
    ok3 = ok4 = True
    if st == wd.ST_OK:
        R = cd.Roche(q)
        ok3 = cd.resolved(q, inc, P3, p3, PHASE_ATOL, R)
        ok4 = cd.resolved(q, inc, P4, p4, PHASE_ATOL, R)
    return st, p3, p4, count, ok3, ok4


def seeded(seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N_SEEDED):
        q = math.exp(rng.uniform(math.log(Q_RANGE[0]), math.log(Q_RANGE[1])))
        top = fd.findphi_fine(q, 90.0, cd.Roche(q))
        dphi = rng.uniform(0.002, 0.95 * top)
        r1 = math.exp(rng.uniform(math.log(R1_RANGE[0]), math.log(R1_RANGE[1])))
        out.append((q, dphi, None, r1))
    return out


def _dcp(v):
    out = wd.dist_cp(*v)
    assert out is not None, v
    return out


def rule_rows(pool):
    """tests/gp_trees.py's rule family: the double's dist_cp of the cache's
    base, of the rows that trip the 120 % rule and of those just short of it"""
    from tests import gp_trees
    vals = gp_trees.rule_values()
    names = list(vals)
    v = np.array([vals[n] for n in names])
    return dict(rule_name=np.array(names), rule_q=v[:, 0], rule_dphi=v[:, 1], rule_rwd=v[:, 2],
                rule_dcp=np.array(pool.map(_dcp, [vals[n] for n in names], chunksize=1)))


def generate(seed, workers):
    jobs = seeded(seed) + [e[1:] for e in EDGES]
    names = ["seeded"] * N_SEEDED + [e[0] for e in EDGES]
    with multiprocessing.Pool(min(16, workers)) as pool:
        inp = pool.map(_inputs, jobs, chunksize=1)
        finite_edges = [k for k in range(N_SEEDED, len(jobs)) if inp[k][2] > 0.0 and jobs[k][2] != "below_grazing"]
        subset = list(range(N_NTHETA)) + finite_edges
        assert len(subset) == N_SUBSET
        rows = [(q, inc, r1, wd.NTHETA, dphi, names[k]) for k, (q, inc, r1, dphi) in enumerate(inp)]
        for nt in NTHETAS:
            rows += [(inp[k][0], inp[k][1], inp[k][2], nt, inp[k][3], names[k]) for k in subset]
        res = pool.map(_row, [r[:4] for r in rows], chunksize=1)
        rule = rule_rows(pool)
    col = lambda k, dt: np.array([r[k] for r in rows], dtype=dt)  # noqa: E731
    out = lambda k, dt: np.array([r[k] for r in res], dtype=dt)   # noqa: E731
    return dict(q=col(0, np.float64), inc=col(1, np.float64), r1=col(2, np.float64), ntheta=col(3, np.int32),
                dphi=col(4, np.float64), name=np.array([r[5] for r in rows]),
                status=out(0, np.int32), phi3=out(1, np.float64), phi4=out(2, np.float64),
                count=out(3, np.int32), resolved3=out(4, bool), resolved4=out(5, bool),
                seed=np.array(seed), phase_atol=np.array(PHASE_ATOL), **rule)


def report(d):
    main = d["ntheta"] == wd.NTHETA
    ok = d["status"] == 0
    part = ok & (d["count"] < d["ntheta"])
    unres = ok & ~(d["resolved3"] & d["resolved4"])
    print("rows %d (ntheta = 10: %d), failed %d" % (len(ok), main.sum(), (~ok).sum()))
    print("part of the limb eclipsed: %d of all rows (%.1f %%), %d of the ntheta = 10 rows (%.1f %%)" % (
        part.sum(), 100.0 * part.mean(), (part & main).sum(), 100.0 * (part & main).sum() / main.sum()))
    print("unresolved at 1e-10: %d (%.1f %%)" % (unres.sum(), 100.0 * unres.mean()))
    print("phi3 < 0: %d" % (ok & (d["phi3"] < 0.0)).sum())
    return part.mean() >= 0.10 and (part & main).sum() >= 0.10 * main.sum() and unres.mean() <= 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wdphases_double.npz"))
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    t0 = time.time()
    d = generate(args.seed, args.workers)
    good = report(d)
    print("wall time %.0f s" % (time.time() - t0))
    if not good:
        raise SystemExit("seed %d misses the population's conditions; nothing written" % args.seed)
    np.savez_compressed(args.out, **d)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
