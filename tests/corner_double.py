"""Test double of the corner-plot data (MODEL_SPEC section 16), in numpy:
np.histogram, np.histogram2d and the level rule; and the shared case list
(columns, sizes, layouts, column picks, bin counts, ranges) of the CPU,
host-program and GPU tests.  The chain's layouts and most value columns are
tests/chain_double.py's; three columns are added here.  Inputs come from
seeded generators; nothing here reads a file.
"""
import functools

import numpy as np

from tests import chain_double as cd

FRACS = tuple(1.0 - np.exp(-0.5 * np.arange(0.5, 2.1, 0.5) ** 2))     # corner's default levels
NBS = (1, 2, 4, 50, 64)
# values on, one ulp below and one ulp above every edge of this range, for every nb of NBS
ONEDGE_RANGE = (0.1, 0.7)
# a range 20 ulp wide: with more than 20 bins its edges repeat
NARROW_LO = 1.5
NARROW_RANGE = (NARROW_LO, NARROW_LO + 20 * np.spacing(NARROW_LO))
COLUMNS = cd.VALUE_COLUMNS + ("onedge", "same", "narrow")
TILE_ROWS = 256                          # lfg_corner_tile_rows() (the GPU test asserts it)
SIZES = ((1, 1), (2, 1), (1, 2), (TILE_ROWS + 1, 1), (37, 6), (64, 64))
LAYOUTS = cd.LAYOUTS
PAIR_TILE = {50: 13, 64: 8}              # lfg_corner_pair_tile(nb) (the GPU test asserts it)


def value_column(kind, rng, n):
    if kind == "onedge":
        pool = []
        for nb in NBS:
            e = np.linspace(ONEDGE_RANGE[0], ONEDGE_RANGE[1], nb + 1)
            pool += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
        pool = rng.permutation(np.concatenate(pool))
        return np.resize(pool, n)
    if kind == "same":
        return np.full(n, -3.25)
    if kind == "narrow":     # a few values just outside the range as well
        return NARROW_LO + rng.integers(-2, 23, n) * np.spacing(NARROW_LO)
    return cd.value_column(kind, rng, n)


@functools.lru_cache(maxsize=None)
def chain(steps, W, C):
    """[steps][W][C]: COLUMNS in turn; read-only, made once per shape"""
    rng = np.random.default_rng([16, steps, W, C])
    x = np.empty((steps, W, C))
    for c in range(C):
        x[:, :, c] = value_column(COLUMNS[c % len(COLUMNS)], rng, steps * W).reshape(steps, W)
    x.setflags(write=False)
    return x


def pick_cols(C, K):
    """K distinct columns of C, unsorted and not adjacent (K = 3 of 10: [5, 0, 3])"""
    if (C, K) == (10, 3):
        return (5, 0, 3)
    return tuple(int(c) for c in np.random.default_rng([C, K]).permutation(C)[:K])


def ranges(x, cols, mode="default"):
    """[K][2].  default: each column's finite minimum and maximum (NaN, NaN
    without a finite value); cut: a quarter of that width off either side, the
    onedge and narrow columns at their own ranges; immobile: as default, but
    the second column (lo == hi), and the last (a NaN bound) if there are
    three or more, do not move."""
    out = np.empty((len(cols), 2))
    for k, c in enumerate(cols):
        v = x[:, :, c].reshape(-1)
        v = v[np.isfinite(v)]
        lo, hi = (v.min(), v.max()) if v.size else (np.nan, np.nan)
        kind = COLUMNS[c % len(COLUMNS)]
        if mode == "cut":
            if kind == "onedge":
                lo, hi = ONEDGE_RANGE
            elif kind == "narrow":
                lo, hi = NARROW_RANGE
            else:
                lo, hi = lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo)
        out[k] = lo, hi
    if mode == "immobile" and len(cols) > 1:
        out[1] = 1.0, 1.0
        if len(cols) > 2:
            out[-1, 0] = np.nan
    return out


def mobile(lo, hi):
    with np.errstate(all="ignore"):
        return bool(np.isfinite(lo) and np.isfinite(hi) and hi > lo and np.isfinite(hi - lo))


def bin_rule(v, lo, hi, nb):
    """MODEL_SPEC 16's bin of every value of v (-1: not used): the largest
    i < nb with e[i] <= x, by a linear walk over np.linspace's edges"""
    e = np.linspace(lo, hi, nb + 1)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        used = np.isfinite(v) & (v >= lo) & (v <= hi)
        b = np.zeros(v.shape, dtype=np.int64)
        for i in range(1, nb):
            b[e[i] <= v] = i
    return np.where(used, b, -1)


def hist1d(v, lo, hi, nb):
    e = np.linspace(lo, hi, nb + 1)
    if np.all(np.diff(e) > 0):
        with np.errstate(invalid="ignore"):
            return np.histogram(v, bins=nb, range=(lo, hi))[0].astype(np.int64)
    b = bin_rule(v, lo, hi, nb)          # repeated edges: np.histogram's guess is not held to them
    return np.bincount(b[b >= 0], minlength=nb).astype(np.int64)


def hist2d(va, vb, ra, rb, nb):
    with np.errstate(invalid="ignore"):
        h = np.histogram2d(va, vb, bins=nb, range=(ra, rb))[0]
    assert np.all(h == np.floor(h))
    return h.astype(np.int64)


def levels(h, fracs=FRACS):
    """corner.hist2d's levels of one histogram, as counts"""
    c = np.sort(np.asarray(h, dtype=np.int64).reshape(-1))[::-1]
    sm = np.cumsum(c).astype(np.float64)
    with np.errstate(invalid="ignore"):
        sm /= sm[-1]
    out = np.empty(len(fracs), dtype=np.int64)
    for i, f in enumerate(fracs):
        inside = c[sm <= f]
        out[i] = inside[-1] if inside.size else c[0]
    return out


def pairs(K):
    return [(a, b) for a in range(K) for b in range(a + 1, K)]


def expected(x, cols, rng, nb, fracs=FRACS):
    """h1 [K][nb], h2 [P][nb][nb], flag [K], levels [P][nl] of x [steps][W][C]"""
    K = len(cols)
    v = [x[:, :, c].reshape(-1) for c in cols]
    mob = [mobile(lo, hi) for lo, hi in rng]
    h1 = np.zeros((K, nb), dtype=np.int64)
    for k in range(K):
        if mob[k]:
            h1[k] = hist1d(v[k], rng[k][0], rng[k][1], nb)
    h2 = np.zeros((len(pairs(K)), nb, nb), dtype=np.int64)
    for p, (a, b) in enumerate(pairs(K)):
        if mob[a] and mob[b]:
            h2[p] = hist2d(v[a], v[b], tuple(rng[a]), tuple(rng[b]), nb)
    lev = np.array([levels(h, fracs) for h in h2], dtype=np.int64).reshape(len(h2), len(fracs))
    return {"h1": h1, "h2": h2, "flag": np.array([0 if m else 1 for m in mob], dtype=np.int32), "levels": lev}


# (size, layout, C, K, nb, range mode).  C = 10 holds every column kind once.
def _cases():
    out = [(size, kind, 10, 3, 50, "default") for size in SIZES for kind in LAYOUTS]
    # K = 1: no pairs; K = 5 and 6 at nb = 50: 10 pairs fill one tile of 13, 15 are a tile and a
    # remainder; K = 18: 153 pairs, several tiles; the same at nb = 64 with K = 4 and 5
    out += [((37, 6), "chain_dev", 20, K, 50, "default") for K in (1, 2, 5, 6, 18)]
    out += [((37, 6), "padded", 10, K, 64, "cut") for K in (4, 5)]
    out += [((37, 6), "skipthin", 70, 64, 4, "default")]                 # 2 016 pairs
    out += [((37, 6), "walker_major", 10, 4, nb, mode) for nb in (1, 2) for mode in ("default", "cut")]
    # ranges: cut on both sides (with the edge, narrow, offset and non-finite columns), an immobile
    # column between mobile ones
    out += [((64, 64), "chain_dev", 10, 10, 50, mode) for mode in ("default", "cut")]
    out += [((64, 64), "skipthin", 10, 10, 64, "cut"), ((37, 6), "chain_dev", 10, 10, 50, "immobile"),
            ((64, 64), "padded", 10, 3, 50, "immobile")]
    return tuple(out)


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case(size, kind, C, K, nb, mode):
    """-> (x, cols, ranges, expected): made once and shared"""
    x = chain(size[0], size[1], C)
    cols = pick_cols(C, K)
    rng = ranges(x, cols, mode)
    return x, cols, rng, expected(x, cols, rng, nb)


def check(got, want, what=""):
    """every count equal, integer for integer"""
    for k in ("flag", "h1", "h2"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), (what, k, int((g != w).sum()) if g.shape == w.shape else g.shape)
    if "levels" in got:
        assert np.array_equal(got["levels"], want["levels"]), (what, "levels")


def run_case(backend, c, what=None):
    """backend(buf, offset, steps, W, row_len, step_ld, walker_ld, cols, ranges,
    nb) -> dict of h1, h2, flag (and levels); checked against the double"""
    size, kind, C, K, nb, mode = c
    x, cols, rng, want = case(*c)
    buf, off, sld, wld = cd.layout(x, kind)
    got = backend(buf, off, x.shape[0], x.shape[1], C, sld, wld, cols, rng, nb)
    check(got, want, what or c)
    return got, want


# ---- constructed level cases: (counts [nb][nb], fractions, expected levels) ----
def level_cases():
    one = np.zeros((4, 4), dtype=np.int64)
    one[2, 1] = 7                                    # a single occupied bin: cum / total = 1 from the start
    flat = np.full((3, 3), 5, dtype=np.int64)        # all equal: position m holds (m + 1) / 9
    empty = np.zeros((2, 2), dtype=np.int64)         # total = 0
    # counts 4, 2, 1, 1 (total 8): the running sums 4, 6, 7, 8 over 8 are exact in binary
    exact = np.array([[1, 4], [2, 1]], dtype=np.int64)
    return [(one, (0.0, 0.5, 0.999, 1.0), (7, 7, 7, 0)),
            (flat, (0.0, 1.0 / 9.0, 0.5, 1.0), (5, 5, 5, 5)),
            (empty, (0.0, 0.5, 1.0), (0, 0, 0)),
            (exact, (0.0, 0.5, 0.75, np.nextafter(0.75, 0.0), 0.875, 1.0), (4, 4, 2, 4, 1, 1))]
