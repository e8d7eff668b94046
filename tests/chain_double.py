"""Test double of the chain summary (MODEL_SPEC section 14), in numpy: sorted
order statistics, np.quantile, np.longdouble two-pass moments (about the
exactly rounded sum's mean), a vectorised
Gelman-Rubin, wdparams.sigma_clipped_stats for the clip; and the shared case
list (value columns, sizes, memory layouts) of the CPU, host-program and GPU
tests.  Inputs come from seeded generators; nothing here reads a file.
"""
import functools
import math

import numpy as np

FRACS = (0.16, 0.5, 0.84)
VALUE_COLUMNS = ("normal", "offset", "equal", "two", "lowbyte", "signs", "nonfinite")
# (steps, W): the smallest, one sweep tile plus one row (tile = 256 rows), odd, square
SIZES = ((1, 1), (2, 1), (1, 2), (257, 1), (37, 6), (64, 64))
LAYOUTS = ("chain_dev", "walker_major", "padded", "skipthin")


def value_column(kind, rng, n):
    if kind == "normal":
        return rng.normal(size=n)
    if kind == "offset":       # the column a sum-of-squares formula fails
        return 1e6 + 1e-3 * rng.normal(size=n)
    if kind == "equal":        # the reference's dev == 0 column
        return np.full(n, 0.1234567)
    if kind == "two":
        return np.where(rng.random(n) < 0.3, -2.5, 7.25)
    if kind == "lowbyte":      # keys that differ in their last byte only: the last radix pass decides
        base = np.float64(1.5).view(np.uint64)
        return (base + rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)
    if kind == "signs":        # the key transform: negatives, both zeros, denormals, huge
        pool = np.array([-1e300, -3.0, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1e-310, 3.0, 1e300, -1e-310, 1.0])
        return pool[rng.integers(0, pool.size, n)]
    if kind == "nonfinite":
        x = rng.normal(size=n)
        k = rng.random(n)
        x[k < 0.1] = np.nan
        x[(k >= 0.1) & (k < 0.15)] = np.inf
        x[(k >= 0.15) & (k < 0.2)] = -np.inf
        return x
    raise KeyError(kind)


def chain(steps, W, C, seed=0):
    """[steps][W][C]: the value columns in turn"""
    rng = np.random.default_rng([seed, steps, W, C])
    x = np.empty((steps, W, C))
    for c in range(C):
        x[:, :, c] = value_column(VALUE_COLUMNS[c % len(VALUE_COLUMNS)], rng, steps * W).reshape(steps, W)
    return x


def layout(x, kind):
    """The logical chain x [steps][W][C] in memory -> (buf, offset, step_ld,
    walker_ld): element (s, w, c) is buf[offset + s * step_ld + w * walker_ld + c]."""
    steps, W, C = x.shape
    if kind == "chain_dev":
        return x.reshape(-1).copy(), 0, W * C, C
    if kind == "walker_major":
        return np.array(x.transpose(1, 0, 2)).reshape(-1), 0, C, steps * C
    if kind == "padded":       # a row of C + 1 elements, the last NaN throughout and never read
        big = np.full((steps, W, C + 1), np.nan)
        big[:, :, :C] = x
        return big.reshape(-1), 0, W * (C + 1), C + 1
    if kind == "skipthin":     # nskip = 2, thin = 3 of a longer chain whose other steps are garbage
        total = 3 * steps + 1  # not a multiple of 3; big[2::3] has exactly `steps` steps
        big = np.full((total, W, C), 9e99)
        big[2::3] = x
        return big.reshape(-1), 2 * W * C, 3 * W * C, C
    raise KeyError(kind)


def ranks(f, n):
    pos = np.float64(f) * np.float64(n - 1)
    lo = int(np.floor(pos))
    return lo, min(lo + 1, n - 1)


def ulp(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.where(np.isfinite(x), np.spacing(np.maximum(x, np.finfo(np.float64).tiny)), np.inf)


def rhat_formula(ch, dtype):
    """Gelman-Rubin of ch [m walkers][n steps] (Gelman & Rubin 1992, as the
    reference evaluates it), in the given float type"""
    ch = ch.astype(dtype)
    m, n = ch.shape
    if m < 2 or n < 2:
        return np.float64(np.nan)
    with np.errstate(all="ignore"):
        grand = ch.mean()
        means = ch.mean(axis=1)
        between = ((means - grand) ** 2).sum() / (m - 1)
        within = ((ch - means[:, None]) ** 2).sum() / (m * (n - 1))
        sigma2 = (n - 1) / dtype(n) * within + between
        return np.float64((m + 1) * sigma2 / (m * within) - (n - 1) / dtype(m * n))


def column(vals, window=None, fracs=FRACS, walkers=None):
    """One column's expected results.  vals: every value in the view (any
    shape); walkers: [W][steps] for R-hat.  Entries: the exact ones (n, n_bad,
    min, max, ostat), quant from np.quantile, and for mean, m2 (and rhat) the
    np.longdouble evaluation with plain FP64 numpy's beside it ('*_np')."""
    v = np.asarray(vals, dtype=np.float64).reshape(-1)
    fin = np.isfinite(v)
    use = fin.copy()
    if window is not None:
        use &= (v >= window[0]) & (v <= window[1])
    u = v[use]
    n = int(u.size)
    out = {"n": n, "n_bad": int((~fin).sum())}
    nq = len(fracs)
    out["ostat"], out["quant"] = np.full((nq, 2), np.nan), np.full(nq, np.nan)
    if n == 0:
        for k in ("mean", "m2", "min", "max", "mean_np", "m2_np"):
            out[k] = np.nan
    else:
        s = np.sort(u)
        out["min"], out["max"] = s[0], s[-1]
        for i, f in enumerate(fracs):
            lo, hi = ranks(f, n)
            out["ostat"][i] = s[lo], s[hi]
            out["quant"][i] = np.quantile(u, f)
        with np.errstate(all="ignore"):
            ld = u.astype(np.longdouble)
            # (the sum from math.fsum, exact to its remainder: 64 mantissa bits
            # lose the small values of a column that also holds +-1e300)
            total = math.fsum(u)
            mean = (np.longdouble(total) + np.longdouble(math.fsum(list(u) + [-total]))) / n
            out["mean"] = np.float64(mean)
            d = ld - mean
            out["m2"] = np.float64((d ** 2).sum() - d.sum() ** 2 / n)
            out["mean_np"] = np.mean(u)
            out["m2_np"] = np.var(u) * n
    if walkers is not None:
        w = np.asarray(walkers, dtype=np.float64)
        if not np.isfinite(w).all():
            out["rhat"] = out["rhat_np"] = np.nan
        else:
            out["rhat"], out["rhat_np"] = rhat_formula(w, np.longdouble), rhat_formula(w, np.float64)
    return out


def expected(x, window=None, fracs=FRACS, rhat=False):
    """column() for every column of x [steps][W][C], stacked"""
    cols = [column(x[:, :, c], None if window is None else window[c], fracs, x[:, :, c].T if rhat else None)
            for c in range(x.shape[2])]
    return {k: np.array([c[k] for c in cols]) for k in cols[0]}


@functools.lru_cache(maxsize=None)
def shared(steps, W, C, rhat=False):
    """(chain, expected) computed once per shape and left unchanged"""
    x = chain(steps, W, C)
    x.setflags(write=False)
    return x, expected(x, rhat=rhat)


# ---- accuracy: profiles/chainstats/README.md ----
# mean, m2 and rhat are held to 8 times plain FP64 numpy's own deviation from
# the np.longdouble evaluation on the same column (both sum in FP64, in another
# order), with a floor of 8 ulp of the result.
ORDER_FACTOR = 8.0
ULP_FLOOR = 8.0


def moment_bound(ref, ref_np):
    with np.errstate(invalid="ignore"):
        return np.maximum(ORDER_FACTOR * np.abs(np.asarray(ref_np) - np.asarray(ref)), ULP_FLOOR * ulp(ref))


def check(got, want, what="", rhat=False, log=None):
    """got: n, n_bad, mean, m2, min, max, ostat, quant (and rhat) arrays per
    column.  Exact entries compare equal (-0.0 equals 0.0, NaN equals NaN);
    quant within 4 ulp of max(|a|, |b|); the moments within moment_bound."""
    for k in ("n", "n_bad", "min", "max", "ostat"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=k not in ("n", "n_bad")), (what, k)
    scale = np.max(np.abs(np.nan_to_num(want["ostat"])), axis=-1)
    q, wq = np.asarray(got["quant"]), want["quant"]
    assert np.array_equal(np.isnan(q), np.isnan(wq)), (what, "quant nan")
    ok = ~np.isnan(wq)
    with np.errstate(invalid="ignore"):
        assert np.all(np.abs(q[ok] - wq[ok]) <= 4 * ulp(scale[ok])), (what, "quant")
    for k in ("mean", "m2") + (("rhat",) if rhat else ()):
        g, w, w_np = np.asarray(got[k]), np.asarray(want[k]), np.asarray(want[k + "_np"])
        exact = ~np.isfinite(w)          # NaN (no values) and an overflowed m2 are reproduced as they are
        assert np.array_equal(g[exact], w[exact], equal_nan=True), (what, k, g[exact], w[exact])
        err, bound = np.abs(g[~exact] - w[~exact]), moment_bound(w[~exact], w_np[~exact])
        if log is not None:
            log.append((what, k, err, np.abs(w_np[~exact] - w[~exact]), bound))
        assert np.all(err <= bound), (what, k, err, bound)


def clip_no_intersection(x, sigma=3.0, maxiters=5):
    """survivors of a clip whose window is NOT intersected with the previous
    one: every round tests all finite values against the new bounds alone"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    x = x[np.isfinite(x)]
    keep = np.ones(x.size, dtype=bool)
    for _ in range(maxiters):
        med, std = np.median(x[keep]), np.std(x[keep])
        keep = (x >= med - sigma * std) & (x <= med + sigma * std)
    return int(keep.sum())


SKEW_SEED = 3


def skewed(seed=SKEW_SEED, n=4000):
    """the right-skewed column of the clip tests"""
    return np.random.default_rng(seed).lognormal(0.0, 1.0, n)


def run_case(backend, x, kind="chain_dev", window=None, fracs=FRACS, rhat=False, want=None, log=None, what=None):
    """backend(buf, offset, steps, W, C, step_ld, walker_ld, window, fracs,
    rhat) -> dict of arrays; checked against the double of x in layout `kind`"""
    buf, off, sld, wld = layout(x, kind)
    steps, W, C = x.shape
    got = backend(buf, off, steps, W, C, sld, wld, window, fracs, rhat)
    want = expected(x, window, fracs, rhat) if want is None else want
    check(got, want, what or (kind, x.shape), rhat, log)
    return got


def gapped(seed=1):
    """A column on which the intersection of successive windows matters: two
    tight clumps with the median at the edge of the upper one, a few high
    outliers and a few values just below the first round's lower bound.  The
    first round drops both groups; the median then falls into the gap between
    the clumps, and the second round's own lower bound would re-admit the low
    values.  (On a lognormal column the bounds only ever tighten: the two
    clips agree there for every seed tried.)"""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.normal(-1.0, 0.05, 1000), rng.normal(1.0, 0.05, 1000), np.full(7, 4.5),
                        np.array([-2.4, -2.45, -2.5])])
    return rng.permutation(v)


def clip_survivors(x, sigma=3.0, maxiters=5):
    """what astropy's successive subsetting keeps"""
    keep = np.asarray(x, dtype=np.float64).reshape(-1)
    keep = keep[np.isfinite(keep)]
    for _ in range(maxiters):
        m, s = np.median(keep), np.std(keep)
        keep = keep[(keep >= m - sigma * s) & (keep <= m + sigma * s)]
    return keep
