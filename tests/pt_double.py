"""Host double of the parallel-tempered sampler (lfg_pt_propose /
lfg_pt_accept / lfg_pt_swap): a NumPy statement of the moves with the
kernels' exact Philox counter layout (include/lfg.h), built on
stretch_double's Philox.  Used to check the HIP kernels draw for draw and to
run sampler.PTSampler on CPU (TorchCpuPTOps)."""
import numpy as np

from tests.stretch_double import MASK, Z_CONTRACTED, _fma, draw, philox, u53, z_of


def propose(pos, half, a, seed, step, exact=False):
    """pos [T, W, ndim] -> q [T * W/2, ndim], zfac [T * W/2]; proposal
    g = t * W/2 + i is walker i of half `half` of level t.  exact: the
    kernel's fma(s - c, z, c) and fma(a - 1, u, 1) in exact rational
    arithmetic (bit-identical rows; slow), else c + (s - c) z and
    (a - 1) u + 1 with two roundings each."""
    T, W, ndim = pos.shape
    ns = W // 2
    r = draw(seed, step, half, 0, T * ns)
    u = u53(r[0], r[1])
    z = z_of(u, a, Z_CONTRACTED) if exact else ((a - 1.0) * u + 1.0) ** 2 / a
    j = ((r[2] * np.uint64(ns)) >> np.uint64(32)).astype(np.int64)
    t = np.repeat(np.arange(T), ns)
    s = pos[:, half * ns:(half + 1) * ns].reshape(T * ns, ndim)
    c = pos[t, (1 - half) * ns + j]
    if exact:
        q = _fma(s - c, z[:, None], c).astype(np.float64)
    else:
        q = c + (s - c) * z[:, None]
    return q, (ndim - 1.0) * np.log(z)


def accept(pos, lnl, lnpr, half, betas, q, zfac, lnp_new, lnlike_e, seed, step, naccept):
    """Tempered Metropolis step of half `half`, in place; returns the
    acceptances [T * W/2]."""
    T, W, _ = pos.shape
    ns = W // 2
    r = draw(seed, step, half, 1, T * ns)
    with np.errstate(divide="ignore"):
        lu = np.log(u53(r[0], r[1]))
    t = np.repeat(np.arange(T), ns)
    w = half * ns + np.tile(np.arange(ns), T)
    ll = np.zeros(T * ns)
    for e in range(lnlike_e.shape[1]):
        ll = ll + lnlike_e[:, e]
    with np.errstate(invalid="ignore"):
        lpr = lnp_new - ll
        diff = zfac + betas[t] * (ll - lnl[t, w]) + (lpr - lnpr[t, w])
        acc = np.isfinite(lnp_new) & (lu < diff)
    pos[t[acc], w[acc]] = q[acc]
    lnl[t[acc], w[acc]] = ll[acc]
    lnpr[t[acc], w[acc]] = lpr[acc]
    naccept[t[acc], w[acc]] += 1
    return acc


def swap_draws(W, seed, step, level):
    """The draws of pair (level, level - 1): permutations A (of level) and B
    (of level - 1), each the stable argsort of W 32-bit keys, and ln u_k."""
    k = np.arange(W, dtype=np.uint64)
    r = philox(k, np.uint64(step) & MASK, np.uint64(step) >> np.uint64(32), np.uint64(4 + level),
               np.uint64(seed) & MASK, np.uint64(seed) >> np.uint64(32))
    A = np.argsort((r[0] << np.uint64(32)) | k, kind="stable")
    B = np.argsort((r[1] << np.uint64(32)) | k, kind="stable")
    with np.errstate(divide="ignore"):
        lu = np.log(u53(r[2], r[3]))
    return A, B, lu


def swap(pos, lnl, lnpr, betas, seed, step, nswap):
    """The swaps of one iteration, in place, pair T-1 first; nswap [T, 2]
    += (proposed, accepted) of pair (i, i - 1) at row i.  Returns
    [(i, A, B, accepted [W])] in the order taken."""
    T, W, _ = pos.shape
    out = []
    for i in range(T - 1, 0, -1):
        A, B, lu = swap_draws(W, seed, step, i)
        acc = lu < (betas[i - 1] - betas[i]) * (lnl[i, A] - lnl[i - 1, B])
        a, b = A[acc], B[acc]
        for x in (pos, lnl, lnpr):
            up = x[i, a].copy()
            x[i, a] = x[i - 1, b]
            x[i - 1, b] = up
        nswap[i, 0] += W
        nswap[i, 1] += int(acc.sum())
        out.append((i, A, B, acc))
    return out


class TorchCpuPTOps:
    """PTSampler ops on CPU tensors, via the numpy double."""

    def __init__(self, exact=False):
        self.exact = exact

    def propose(self, pos, half, a, seed, step, q, zfac):
        import torch
        qq, zz = propose(pos.numpy(), half, a, seed, step, exact=self.exact)
        q.copy_(torch.as_tensor(qq))
        zfac.copy_(torch.as_tensor(zz))

    def accept(self, pos, lnl, lnpr, half, betas, q, zfac, lnp_new, lnlike_e, seed, step, naccept):
        accept(pos.numpy(), lnl.numpy(), lnpr.numpy(), half, betas.numpy(), q.numpy(), zfac.numpy(),
               lnp_new.numpy(), lnlike_e.numpy(), seed, step, naccept.numpy())

    def swap(self, pos, pos_out, lnl, lnpr, betas, seed, step, nswap):
        pos_out.copy_(pos)
        swap(pos_out.numpy(), lnl.numpy(), lnpr.numpy(), betas.numpy(), seed, step, nswap.numpy())


class GaussianTarget:
    """A torch evaluator with the LnProbEvaluator call signature, on any
    device: lnlike = -|x|^2 / 2 (one 'eclipse'), lnprior = -|x|^2 / (2 s^2)."""
    E = 1

    def __init__(self, device="cpu", prior_sigma=3.0):
        import torch
        self.device = torch.device(device)
        self.s2 = float(prior_sigma) ** 2

    def __call__(self, x, out=None, lnlike_e=None):
        r2 = (x * x).sum(1)
        ll = -0.5 * r2
        lnp = ll - r2 / (2.0 * self.s2)
        if lnlike_e is not None:
            lnlike_e.copy_(ll[:, None])
        if out is None:
            return lnp
        out.copy_(lnp)
        return out
