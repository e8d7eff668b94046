#!/usr/bin/env python
"""tests/golden/flux_double.npz: what the flux double (tests/flux_double.py)
is too slow to recompute in a test.

    python tools/make_flux_golden.py [--out tests/golden/flux_double.npz] [--workers 16]
    python tools/make_flux_golden.py --check      # regenerate and compare with the committed file

Per parameter set: the arbiter's [a_i, b_i] of the 1 500 elements, the
eclipsed mask, the inclination, the stream's impact point and velocity.  For
the first set also the intervals of two caller-chosen disc grids (5.6) and,
in single precision, of the elements each `mutate` value of the double moves.

A set is accepted only if the arbiter resolves every contact of every
element to PHASE_ATOL (contact_double.resolved); one that does not is
replaced by its nearest neighbour that does (NEIGHBOURS), and the swap is
recorded in the file and printed.  Imports the double and the arbiter only.
"""
import argparse
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import contact_double as cd      # noqa: E402
from tests import flux_double as fd         # noqa: E402
from tests.helpers import ECL1, TRUTH14, TRUTH18   # noqa: E402

PHASE_ATOL = 1e-10
DISC_GRIDS = (250, 777)     # caller-chosen PyDisc sizes of the first set


def _edge(**kw):
    p = dict(zip("wdFlux dFlux sFlux rsFlux q dphi rdisc ulimb rwd scale az fis dexp phi0 exp1 exp2 tilt yaw".split(),
                 TRUTH18))
    p.update(kw)
    return list(p.values())


# name, parameters, inclination that sets dphi (or None: dphi as given)
SETS = [
    ("truth18", TRUTH18, None),
    ("ecl1", ECL1, None),
    ("truth14", TRUTH14, None),
    # q > 1 at high inclination; fis = 0; tilt > 90 with negative yaw; dexp = 2 exactly; ulimb = 0
    ("q_above_1", _edge(q=1.6, rdisc=0.45, ulimb=0.0, rwd=0.03, scale=0.04, az=130.0, fis=0.0, dexp=2.0,
                        phi0=0.002, exp1=1.5, exp2=2.0, tilt=120.0, yaw=-20.0), 86.0),
    # q ~ 0.02; fis = 1; ulimb = 1; dexp = 1.9986; a small exp2 with a long strip
    ("q_small", _edge(q=0.02, rdisc=0.7, ulimb=1.0, rwd=0.015, scale=0.01, az=110.0, fis=1.0, dexp=1.9986,
                      phi0=-0.003, exp1=0.5, exp2=0.6, tilt=60.0, yaw=10.0), 87.5),
    # a near-grazing dphi with a large disc
    ("grazing", _edge(dphi=0.012, rdisc=0.6), None),
]

# the k-th neighbour of a set that the rejection rule refuses: (q, rdisc) scaled
NEIGHBOURS = [(1.0, 1.0)] + [(1.0 + 0.002 * k * sgn, 1.0 - 0.003 * k) for k in range(1, 6) for sgn in (1, -1)]


def disc_grid(npts):
    """MODEL_SPEC 5.6's rule for PyDisc's npts"""
    nr = max(1, int(round(np.sqrt(npts / 2.5))))
    return nr, max(1, int(round(npts / nr)))


def _chunk(job):
    q, inc, P = job
    R = cd.Roche(q)
    out = []
    for p in P:
        ecl, a, b = cd.interval(q, inc, p, R)
        ok = (not ecl) or all(cd.resolved(q, inc, p, x, PHASE_ATOL, R) for x in (a, b))
        out.append((a, b, ok) if ecl else (1.0, -1.0, True))
    return out


def solve(pool, q, inc, P, n=12):
    jobs = [(q, inc, P[k:k + n]) for k in range(0, len(P), n)]
    res = [r for part in pool.map(_chunk, jobs) for r in part]
    a, b, ok = (np.array(v) for v in zip(*res))
    return a, b, ok.astype(bool)


def make_set(pool, pars, inc_for_dphi):
    pars = [float(v) for v in pars]
    R = cd.Roche(pars[4])
    if inc_for_dphi is not None:
        pars[5] = round(fd.findphi_fine(pars[4], inc_for_dphi, R), 6)
    inc = fd.findi(pars[4], pars[5], R)
    if inc is None:
        return None, "no inclination"
    rdisc_a = pars[6] * R.xl1
    bs = fd.bspot(pars[4], rdisc_a, R.xl1)
    if bs is None:
        return None, "the stream misses the disc"
    rec = {"pars": np.array(pars), "inc": inc, "bs": np.array(bs)}
    m = fd.model(pars, record=rec, positions_only=True)
    a, b, ok = solve(pool, m.q, inc, m.P)
    if not ok.all():
        return None, "%d unresolved contacts (elements %s...)" % ((~ok).sum(), np.nonzero(~ok)[0][:5])
    rec.update(a=a, b=b, ecl=a < b)
    return rec, None


def extras(pool, rec):
    """the first set's caller-chosen disc grids and mutated elements"""
    pars = list(rec["pars"])
    q, inc = pars[4], float(rec["inc"])
    out = {}
    for npts in DISC_GRIDS:
        nr, naz = disc_grid(npts)
        P, _ = fd.component_elements(1, [pars[8], pars[6], pars[12]], q, inc, nr, naz)
        a, b, ok = solve(pool, q, inc, P)
        assert ok.all(), "unresolved contact on the %d-element disc" % npts
        out["disc%d_a" % npts], out["disc%d_b" % npts] = a, b
    bs_mut = fd.bspot(q, pars[6])           # rdisc in units of a
    assert bs_mut is not None
    out["mut_rdisc_in_a_bs"] = np.array(bs_mut)
    tmp = dict(rec, **out)
    for name, parts in fd.MUT_MOVES.items():
        m = fd.model(pars, record=tmp, mutate=name, positions_only=True)
        lo, hi = fd.SLICES[parts[0]].start, fd.SLICES[parts[-1]].stop
        a, b, _ = solve(pool, q, inc, m.P[lo:hi])
        out["mut_%s_a" % name], out["mut_%s_b" % name] = a.astype(np.float32), b.astype(np.float32)
    return out


def generate(workers):
    t0 = time.time()
    data, names, swaps = {}, [], []
    with multiprocessing.Pool(min(16, workers)) as pool:
        for k, (name, pars, inc_t) in enumerate(SETS):
            for fq, fr in NEIGHBOURS:
                p = list(pars)
                p[4], p[6] = p[4] * fq, p[6] * fr
                rec, why = make_set(pool, p, inc_t)
                if rec is not None:
                    break
                print("%s x (q %.3f, rdisc %.3f): refused, %s" % (name, fq, fr, why), flush=True)
            else:
                raise SystemExit("no neighbour of %s passes the rejection rule" % name)
            if (fq, fr) != (1.0, 1.0):
                swaps.append({"set": name, "q_factor": fq, "rdisc_factor": fr, "why": why})
            if k == 0:
                rec.update(extras(pool, rec))
            names.append(name)
            for key, v in rec.items():
                data["%s/%s" % (name, key)] = v
            print("%-10s inc %.6f  eclipsed %4d / 1500   %.0f s" % (name, rec["inc"], rec["ecl"].sum(),
                                                                   time.time() - t0), flush=True)
    data["names"] = np.array(names)
    data["swaps"] = np.array(json.dumps(swaps))
    return data, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "flux_double.npz"))
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--check", action="store_true", help="compare a fresh run with --out instead of writing it")
    args = ap.parse_args()
    data, wall = generate(args.workers)
    print("wall time %.0f s" % wall)
    if args.check:
        old = np.load(args.out)
        worst = 0.0
        for key in data:
            if key.endswith("/a") or key.endswith("/b") or "/disc" in key:
                worst = max(worst, float(np.max(np.abs(old[key] - data[key]))))
        print("largest change of a committed interval: %.2e" % worst)
        sys.exit(0 if worst <= 1e-12 else 1)
    np.savez_compressed(args.out, **data)
    print("%s: %d bytes, swaps: %s" % (args.out, os.path.getsize(args.out), str(data["swaps"])))


if __name__ == "__main__":
    main()
