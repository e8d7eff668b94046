"""Host test double of the device stretch move (lfg_stretch_propose /
lfg_stretch_accept and every restatement of them: accept_regen, the verdict
kernels, make_prop, fold_rows, the PT and WD samplers): numpy Philox4x32-10
with the kernels' counter layout.  Used to check the HIP kernels
draw-for-draw and to exercise the sampler's sharding logic on CPU (gloo).

Two arithmetics.  The legacy one (exact=False: c - (c - s) z and
(a - 1) u + 1 with two roundings each) is what the CPU sharding tests run
on.  exact=True is the device's, bit for bit: rows fma(s - c, z, c) and
z = fma(a - 1, u, 1)^2 / a in exact rational arithmetic, one rounding each
(Z_CONTRACTED: the reading of (a - 1) u + 1 that include/lfg.h states).

`mutate` flips one convention (MUTATIONS); the tests use it to show that
they would notice."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)

Z_CONTRACTED = True   # the device forms (a - 1) u + 1 as one fma (include/lfg.h)
MUTATIONS = ("z_uncontracted", "partner_ns_minus_1", "step_hi_dropped", "half_purpose_swapped")
# (a, seed, step) at which a W = 10 ensemble tells every mutation in both halves
MUTATION_CASE = (2.5, 2**40 + 7, 2**33 + 26)


def philox(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    for _ in range(10):
        p0 = c0 * M0
        p1 = c2 * M1
        lo0, hi0 = p0 & MASK, p0 >> np.uint64(32)
        lo1, hi1 = p1 & MASK, p1 >> np.uint64(32)
        c0, c1, c2, c3 = (hi1 ^ c1 ^ k0) & MASK, lo1, (hi0 ^ c3 ^ k1) & MASK, lo0
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def u53(a, b):
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    return ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64) / 9007199254740992.0


def draw(seed, step, half, purpose, n, mutate=None, lo=0):
    """The draws of walkers lo .. lo + n - 1 of half `half`: counter =
    (walker, step lo, step hi, half * 2 + purpose), key = seed."""
    i = np.arange(lo, lo + n, dtype=np.uint64)
    hi = np.uint64(0) if mutate == "step_hi_dropped" else np.uint64(step) >> np.uint64(32)
    cw = purpose * 2 + half if mutate == "half_purpose_swapped" else half * 2 + purpose
    return philox(i, np.uint64(step) & MASK, hi, np.uint64(cw), np.uint64(seed) & MASK,
                  np.uint64(seed) >> np.uint64(32))


def _fma1(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # one rounding, as the device's fma


_fma = np.frompyfunc(_fma1, 3, 1)


def fma(a, b, c):
    """a b + c with one rounding, elementwise (exact rationals; slow)"""
    return np.asarray(_fma(a, b, c), dtype=np.float64)


def z_of(u, a, contracted):
    """z = ((a - 1) u + 1)^2 / a.  contracted: (a - 1) u + 1 as one fma (one
    rounding), else product and sum rounded in turn.  The two agree whenever
    (a - 1) u is exact (a - 1 a power of two: a = 2, 1.5) and differ in the
    last bit on a few per cent of the draws otherwise."""
    u = np.asarray(u, np.float64)
    zr = fma(a - 1.0, u, 1.0) if contracted else (a - 1.0) * u + 1.0
    return zr * zr / a


def stretch_draws(ns, half, a, seed, step, mutate=None, exact=True):
    """z [ns] and partner index [ns] of half `half`'s proposals"""
    r = draw(seed, step, half, 0, ns, mutate)
    u = u53(r[0], r[1])
    if exact:
        z = z_of(u, a, Z_CONTRACTED != (mutate == "z_uncontracted"))
    else:
        z = ((a - 1.0) * u + 1.0) ** 2 / a
    mul = ns - 1 if mutate == "partner_ns_minus_1" else ns
    j = ((r[2] * np.uint64(mul)) >> np.uint64(32)).astype(np.int64)
    return z, j


def propose(pos, half, a, seed, step, exact=False, mutate=None):
    """q [W/2, ndim], zfac [W/2] of half `half` (k_propose).  exact: the
    device's arithmetic bit for bit (module docstring); `log` alone is not
    correctly rounded on either side."""
    W, ndim = pos.shape
    ns = W // 2
    z, j = stretch_draws(ns, half, a, seed, step, mutate, exact)
    s = pos[half * ns:(half + 1) * ns]
    c = pos[(1 - half) * ns:(2 - half) * ns][j]
    q = fma(s - c, z[:, None], c) if exact else c - (c - s) * z[:, None]
    return q, (ndim - 1.0) * np.log(z)


def _decide(lu, zfac, lnp_new, lnp_old, log=None):
    """ln u < zfac + lnp_new - lnp_old; log: a chain()'s margin record"""
    with np.errstate(invalid="ignore"):
        diff = zfac + lnp_new - lnp_old
        acc = lu < diff
    if log is not None:
        fin = np.isfinite(diff) & np.isfinite(lu)
        if fin.any():
            log.margin = min(log.margin, float(np.min(np.abs(lu[fin] - diff[fin]))))
        for k in np.flatnonzero(~fin):
            log.nonfinite.append((float(lu[k]), float(zfac[k]), float(lnp_new[k]), float(lnp_old[k]), bool(acc[k])))
    return acc


def _lnu(seed, step, half, n, mutate=None, lo=0):
    r = draw(seed, step, half, 1, n, mutate, lo)
    with np.errstate(divide="ignore"):
        return np.log(u53(r[0], r[1]))


def accept(pos, lnp, half, q, zfac, lnp_new, seed, step, naccept, mutate=None, log=None):
    W = pos.shape[0]
    ns = W // 2
    sl = slice(half * ns, (half + 1) * ns)
    acc = _decide(_lnu(seed, step, half, ns, mutate), zfac, lnp_new, lnp[sl], log)
    pos[sl][acc] = q[acc]
    lnp[sl][acc] = lnp_new[acc]
    naccept[sl][acc] += 1
    return acc


def accept_regen(pos, lnp, half, a, lnp_new, seed, step, naccept, accflag=None, mutate=None):
    """k_accept_regen: the Metropolis step of the whole half with each
    accepted row re-formed in place from its draws, fma(p - c_j, z, c_j)"""
    W, ndim = pos.shape
    ns = W // 2
    z, j = stretch_draws(ns, half, a, seed, step, mutate)
    sl = slice(half * ns, (half + 1) * ns)
    acc = _decide(_lnu(seed, step, half, ns, mutate), (ndim - 1.0) * np.log(z), lnp_new, lnp[sl])
    c = pos[(1 - half) * ns:(2 - half) * ns][j]
    pos[sl][acc] = fma(pos[sl] - c, z[:, None], c)[acc]
    lnp[sl][acc] = lnp_new[acc]
    naccept[sl][acc] += 1
    if accflag is not None:
        accflag[:] = acc
    return acc


def verdict(lnp_new, lnp, zfac, lo, ns, half, seed, step, mutate=None):
    """k_verdict: walkers lo .. lo + n - 1 of the half; the new ln_prob where
    the move is accepted, NaN where it is not"""
    n = lnp_new.shape[0]
    acc = _decide(_lnu(seed, step, half, n, mutate, lo), zfac, lnp_new, lnp[half * ns + lo:half * ns + lo + n])
    return np.where(acc, lnp_new, np.nan)


def apply_verdicts(pos, lnp, half, a, v, seed, step, naccept, accflag=None, mutate=None):
    """k_apply_verdicts: half `half`'s gathered verdicts (NaN = rejected)
    applied, the rows re-formed as accept_regen re-forms them"""
    ns = pos.shape[0] // 2
    z, j = stretch_draws(ns, half, a, seed, step, mutate)
    sl = slice(half * ns, (half + 1) * ns)
    acc = ~np.isnan(v)
    c = pos[(1 - half) * ns:(2 - half) * ns][j]
    pos[sl][acc] = fma(pos[sl] - c, z[:, None], c)[acc]
    lnp[sl][acc] = v[acc]
    naccept[sl][acc] += 1
    if accflag is not None:
        accflag[:] = acc
    return acc


def chain(pos0, lnp0, lnprob_fn, a, seed, step0, iters):
    """The plain red/blue loop in the device's arithmetic: per iteration
    step0 + it, half 0 then half 1, propose (exact) -> lnprob_fn(q) -> accept.
    Returns pos [iters, W, ndim], lnp [iters, W], naccept [iters, W] (the
    running counters after each step), acc and lnp_new [iters, 2, W/2] (the
    decisions and the proposals' ln_prob), margin: the smallest |ln u - (zfac + lnp_new - lnp_old)| over the
    decisions whose two sides are finite, and nonfinite: (ln u, zfac, lnp_new,
    lnp_old, accepted) of every other decision (the comparison's operands: no
    margin exists)."""
    pos, lnp = np.array(pos0, np.float64), np.array(lnp0, np.float64)
    W = pos.shape[0]
    nacc = np.zeros(W, np.int64)
    out = SimpleNamespace(pos=[], lnp=[], naccept=[], acc=[], lnp_new=[], margin=np.inf, nonfinite=[])
    for it in range(iters):
        both, news = [], []
        for half in (0, 1):
            q, zfac = propose(pos, half, a, seed, step0 + it, exact=True)
            lnp_new = np.asarray(lnprob_fn(q), np.float64)
            both.append(accept(pos, lnp, half, q, zfac, lnp_new, seed, step0 + it, nacc, log=out))
            news.append(lnp_new)
        out.pos.append(pos.copy())
        out.lnp.append(lnp.copy())
        out.naccept.append(nacc.copy())
        out.acc.append(np.stack(both))
        out.lnp_new.append(np.stack(news))
    for k in ("pos", "lnp", "naccept", "acc", "lnp_new"):
        setattr(out, k, np.stack(getattr(out, k)))
    return out


class TorchCpuOps:
    """EnsembleSampler ops on CPU tensors, via the numpy double."""

    def propose(self, pos, half, a, seed, step, q, zfac):
        import torch
        qq, zz = propose(pos.numpy(), half, a, seed, step)
        q.copy_(torch.as_tensor(qq))
        zfac.copy_(torch.as_tensor(zz))

    def accept(self, pos, lnp, half, q, zfac, lnp_new, seed, step, naccept):
        p, l, n = pos.numpy(), lnp.numpy(), naccept.numpy()
        accept(p, l, half, q.numpy(), zfac.numpy(), lnp_new.numpy(), seed, step, n)
