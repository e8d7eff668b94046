"""Test helper: an independent double of the limb-darkening surfaces
(MODEL_SPEC section 15) and what the limb-darkening tests share.

The double uses neither FITPACK's bivariate code nor physpar.eval_bispline:
it is the tensor product of 1-D not-a-knot cubic splines, which is what an
interpolating bicubic with not-a-knot knots is.  make_interp_spline(teff
nodes, Z, k=3, axis=1) interpolates every logg row along teff; at a point
the 19 values of those splines are interpolated along logg by one more
make_interp_spline.  It is defined inside the grid only (no clamp).

The golden file tests/golden/limbdark_ref.npz holds the reference's own ld()
at the points tools/make_ld_golden.py lists.  TOL is the issue's bound:
de Boor's recursion gives a basis value a relative error of about 9 eps, the
16-term sum of products has sum hx hy = 1 and |c| <= c_max, so the absolute
error is about 40 eps c_max; 64 eps c_max is used, c_max from the loaded
tables (1.8e-14 on the shipped ones).
"""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_DIR = os.path.join(ROOT, "tests", "golden", "ld_coeffs")
GOLDEN = os.path.join(ROOT, "tests", "golden", "limbdark_ref.npz")
ST_OK, ST_BAD_ARGS, ST_CLAMPED = 0, 5, 7


@functools.lru_cache(maxsize=None)
def tables():
    from lfit_python_amd import limbdark
    return limbdark.load_ld_tables(LD_DIR)


@functools.lru_cache(maxsize=None)
def golden():
    """the golden file's arrays (read-only) and the statuses its points must get"""
    g = dict(np.load(GOLDEN))
    for a in g.values():
        a.setflags(write=False)
    return g


def tol():
    return 64.0 * np.finfo(np.float64).eps * tables().c_max


def expected_status(logg, teff):
    """CLAMPED strictly outside [5, 9.5] x [4000, 30000], BAD_ARGS for a non-finite input, else OK"""
    logg, teff = np.broadcast_arrays(np.asarray(logg, dtype=np.float64), np.asarray(teff, dtype=np.float64))
    T = tables()
    out = np.zeros(logg.shape, dtype=np.int32)
    out[(logg < T.logg[0]) | (logg > T.logg[-1]) | (teff < T.teff[0]) | (teff > T.teff[-1])] = ST_CLAMPED
    out[~(np.isfinite(logg) & np.isfinite(teff))] = ST_BAD_ARGS
    return out


def tensor_double(logg, teff):
    """[n, 25] at points inside the grid: 1-D not-a-knot splines along teff, then along logg"""
    from scipy.interpolate import make_interp_spline
    T = tables()
    logg, teff = np.asarray(logg, dtype=np.float64), np.asarray(teff, dtype=np.float64)
    assert np.all((logg >= T.logg[0]) & (logg <= T.logg[-1]) & (teff >= T.teff[0]) & (teff <= T.teff[-1]))
    out = np.empty((len(logg), 25))
    for s in range(25):
        along_t = make_interp_spline(T.teff, T.values[s], k=3, axis=1)(teff)      # [ng, n]
        for i in range(len(logg)):
            out[i, s] = make_interp_spline(T.logg, along_t[:, i], k=3)(logg[i])
    return out


def mixed_rows(n=257, seed=4):
    """n (logg, teff) rows with all three statuses: golden points (every kind), shuffled, with
    NaN and infinities put into a few; returns (logg, teff, golden row index or -1)"""
    g = golden()
    rng = np.random.default_rng(seed)
    special = np.flatnonzero(g["kind"] >= 2)
    pick = np.concatenate([special[:40], rng.choice(np.flatnonzero(g["kind"] < 2), n - 40 - 6, replace=False)])
    logg, teff = g["logg"][pick].copy(), g["teff"][pick].copy()
    idx = pick.astype(np.int64)
    bad_l = np.array([np.nan, 8.0, np.inf, 8.0, -np.inf, np.nan])
    bad_t = np.array([12000.0, np.nan, 12000.0, -np.inf, np.inf, np.nan])
    logg, teff, idx = np.concatenate([logg, bad_l]), np.concatenate([teff, bad_t]), np.concatenate([idx, -np.ones(6, int)])
    order = rng.permutation(n)
    return logg[order], teff[order], idx[order]


def check_rows(table, status, logg, teff, idx, what=""):
    """every row against the golden values within tol(), NaN rows where the status says so, statuses exact"""
    g = golden()
    want_st = expected_status(logg, teff)
    assert np.array_equal(np.asarray(status), want_st), what
    table = np.asarray(table)
    bad = want_st == ST_BAD_ARGS
    assert np.all(np.isnan(table[bad])) and np.all(idx[bad] < 0) and np.all(idx[~bad] >= 0), what
    if (~bad).any():
        err = np.max(np.abs(table[~bad] - g["table"][idx[~bad]]))
        print("%s max abs error %.3e (tolerance %.3e)" % (what, err, tol()))
        assert err <= tol(), (what, err)
