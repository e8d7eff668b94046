#!/usr/bin/env python3
"""Generate tests/golden/limbdark_ref.npz from the reference's own limbdark.py.

    python tools/make_ld_golden.py --reference REFERENCE_DIR [--check | --tables]

Runs only where a checkout of the reference is at hand: it imports
REFERENCE_DIR/limbdark.py (numpy and scipy are all that needs) and calls its
ld(band, logg, teff, law) for every band and law at every point below;
nothing of the reference travels, only the numbers it returns.  The tables
ld() reads, REFERENCE_DIR/Gianninas13/ld_coeffs_<band>.txt, are the files
under tests/golden/ld_coeffs/ with every data row cut after byte 47, the last
of the seven columns ld() reads (logg, teff, a, b, c, d, f; the eleven
columns of other laws behind them are never read); the header lines are whole.
--tables writes those copies, and every other run refuses to start unless
they are exactly that cut of the reference's files.

Points (logg, teff), `kind` in the file:
  0  all 627 nodes of the 19 x 33 grid
  1  the centre of each of the 18 x 32 grid cells: every knot interval of both
     axes, the double-width ones at the dropped nodes (5.25, 9.25, 4250,
     25000) included
  2  outside each of the four sides and the four corners
  3  exactly on each edge, off the nodes
  4  200 uniform points in [4.5, 10] x [3000, 35000], seed 20130

The file: logg, teff, kind [n]; table [n, 25], column band * 5 + coef with
bands u, g, r, i, z and coefficients linear, quad a, quad b, sqr d, sqr f.
--check regenerates and compares with the committed file bit for bit.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "limbdark_ref.npz")
TABLES = os.path.join(ROOT, "tests", "golden", "ld_coeffs", "Gianninas13")
BANDS = ("u", "g", "r", "i", "z")
sys.dont_write_bytecode = True


ROW_BYTES = 47  # bytes 1-47: logg, teff and the linear, quadratic and square-root coefficients


def cut_table(path):
    """the file's lines, data rows cut after ROW_BYTES bytes"""
    with open(path, "rb") as fh:
        return [l if l.startswith(b"#") else l[:ROW_BYTES].rstrip() + b"\n" for l in fh.read().splitlines(keepends=True)]


def points():
    g1 = np.array([5.0 + 0.25 * k for k in range(19)])
    t1 = np.loadtxt(os.path.join(TABLES, "ld_coeffs_u.txt"))[:33, 1]
    assert len(np.unique(t1)) == 33 and t1[0] == 4000.0 and t1[-1] == 30000.0
    sets = []
    G, T = np.meshgrid(g1, t1, indexing="ij")
    sets.append((G.ravel(), T.ravel()))
    G, T = np.meshgrid(0.5 * (g1[:-1] + g1[1:]), 0.5 * (t1[:-1] + t1[1:]), indexing="ij")
    sets.append((G.ravel(), T.ravel()))
    sets.append((np.array([4.7, 9.9, 8.0, 8.0, 4.7, 4.7, 9.9, 9.9]),
                 np.array([12000.0, 12000.0, 3500.0, 41000.0, 3500.0, 41000.0, 3500.0, 41000.0])))
    sets.append((np.array([5.0, 9.5, 7.77, 7.77]), np.array([12345.0, 12345.0, 4000.0, 30000.0])))
    rng = np.random.default_rng(20130)
    sets.append((rng.uniform(4.5, 10.0, 200), rng.uniform(3000.0, 35000.0, 200)))
    logg = np.concatenate([s[0] for s in sets])
    teff = np.concatenate([s[1] for s in sets])
    kind = np.concatenate([np.full(len(s[0]), k, dtype=np.int32) for k, s in enumerate(sets)])
    return logg, teff, kind


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="the directory that holds the reference's limbdark.py")
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed file, bit for bit")
    ap.add_argument("--tables", action="store_true", help="write the cut copies of the reference's five tables and stop")
    args = ap.parse_args()
    src = os.path.join(args.reference, "limbdark.py")
    if not os.path.isfile(src):
        sys.exit("%s: no limbdark.py there" % args.reference)
    for b in BANDS:
        name = "ld_coeffs_%s.txt" % b
        want = b"".join(cut_table(os.path.join(args.reference, "Gianninas13", name)))
        if args.tables:
            os.makedirs(TABLES, exist_ok=True)
            with open(os.path.join(TABLES, name), "wb") as fh:
                fh.write(want)
        elif open(os.path.join(TABLES, name), "rb").read() != want:
            sys.exit("%s is not the reference's table cut after byte %d" % (os.path.join(TABLES, name), ROW_BYTES))
    if args.tables:
        return
    spec = importlib.util.spec_from_file_location("ref_limbdark", src)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    logg, teff, kind = points()
    n = len(logg)
    table = np.empty((n, 25))
    for i in range(n):
        for b, band in enumerate(BANDS):
            a, c = ref.ld(band, logg[i], teff[i], law="quad")
            d, f = ref.ld(band, logg[i], teff[i], law="sqr")
            table[i, 5 * b: 5 * b + 5] = [ref.ld(band, logg[i], teff[i]), a, c, d, f]
        if i % 200 == 0:
            print("point %d of %d" % (i, n), flush=True)
    if args.check:
        old = np.load(OUT)
        for key, new in (("logg", logg), ("teff", teff), ("kind", kind), ("table", table)):
            if old[key].shape != new.shape or old[key].tobytes() != new.tobytes():
                sys.exit("%s: %r differs from what the reference gives now" % (OUT, key))
        print("%s: %d points x 25 columns, bit for bit what the reference gives" % (OUT, n))
        return
    np.savez_compressed(OUT, logg=logg, teff=teff, kind=kind, table=table)
    print("wrote %s: %d points x 25 columns" % (OUT, n))


if __name__ == "__main__":
    main()
