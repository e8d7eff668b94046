"""Device-resident parallel-tempered ensemble sampler.

Stands in for ptemcee.Sampler(nwalkers, ndim, logl, logp, ntemps=...) as the
reference drives it with usePT = 1 (mcmcfit.py:251-270, 319-329;
mcmc_utils.py:75-111, 186-239): T temperature levels of W walkers live in
HBM, level t samples betas[t] * ln_like + ln_prior, and one iteration is

  half 0, half 1:  propose every level (lfg_pt_propose) -> ONE batched
                   ln_prob of the T * W/2 proposals with its per-eclipse
                   ln_like -> tempered Metropolis step (lfg_pt_accept)
  swaps:           adjacent levels exchange walkers (lfg_pt_swap)

with no host synchronisation and no device -> host copy inside the loop
(include/lfg.h states the moves and the Philox counter of every draw).

Deliberately not the reference's: it hands ln_prob to ptemcee as the prior
term (mcmcfit.py:264-270), so its cold chain samples 2 ln_like + ln_prior
and every light curve is evaluated twice.  Here the prior is the prior: the
cold level samples the posterior of the non-PT path, one model evaluation
per proposal (ln_like = sum of lnlike_e, ln_prior = ln_prob - ln_like).
Adaptive ladders, evidence estimates and multi-rank PT are not provided.
"""
import ctypes

import numpy as np

from . import _native


def default_betas(ndim, ntemps=None, Tmax=None):
    """The geometric ladder betas[t] = r^-t.  r = 1 + 2 sqrt(ln 4) / sqrt(ndim)
    (the spacing at which adjacent levels of an ndim-dimensional Gaussian swap
    about 25 % of the time; ptemcee's large-ndim formula.  ptemcee tabulates
    slightly different steps for ndim <= 100; it is not available to this
    project, so those tabulated values are not reproduced).  As in ptemcee:
    Tmax alone fixes the number of levels (the first ladder reaching Tmax),
    ntemps and a finite Tmax together fix r = Tmax^(1 / (ntemps - 1)), and
    Tmax = inf makes the hottest level beta = 0."""
    if ndim < 1:
        raise ValueError("ndim must be >= 1")
    if ntemps is None and Tmax is None:
        raise ValueError("give ntemps, Tmax or an explicit ladder")
    if ntemps is not None and int(ntemps) < 1:
        raise ValueError("ntemps must be >= 1")
    if Tmax is not None and not Tmax > 1.0:
        raise ValueError("Tmax must be > 1")
    r = 1.0 + 2.0 * np.sqrt(np.log(4.0)) / np.sqrt(ndim)
    hot = Tmax is not None and np.isinf(Tmax)
    if hot:
        if ntemps is None:
            raise ValueError("Tmax = inf needs ntemps")
        n = int(ntemps) - 1
    elif ntemps is None:
        n = int(np.log(Tmax) / np.log(r) + 2)
    else:
        n = int(ntemps)
        if Tmax is not None and n > 1:
            r = float(Tmax) ** (1.0 / (n - 1))
    betas = r ** -np.arange(n, dtype=np.float64)
    return np.concatenate([betas, [0.0]]) if hot else betas


def _host(t):
    return t.cpu().numpy() if t.device.type != "cpu" else t.numpy().copy()


class HipPTOps:
    """The parallel-tempering kernels (include/lfg.h, lfg_pt_*)."""

    def __init__(self, device):
        self.L = _native.lib()
        self.device = device
        self._ws = None

    @staticmethod
    def _vp(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def propose(self, pos, half, a, seed, step, q, zfac):
        T, W, ndim = pos.shape
        rc = self.L.lfg_pt_propose(self._vp(pos), T, W, ndim, half, a, seed, step, self._vp(q), self._vp(zfac),
                                   _native.stream_ptr(self.device))
        _native.check(rc, "lfg_pt_propose")

    def accept(self, pos, lnl, lnpr, half, betas, q, zfac, lnp_new, lnlike_e, seed, step, naccept):
        T, W, ndim = pos.shape
        rc = self.L.lfg_pt_accept(self._vp(pos), self._vp(lnl), self._vp(lnpr), T, W, ndim, half, self._vp(betas),
                                  self._vp(q), self._vp(zfac), self._vp(lnp_new), self._vp(lnlike_e),
                                  lnlike_e.shape[1], seed, step, self._vp(naccept), _native.stream_ptr(self.device))
        _native.check(rc, "lfg_pt_accept")

    def workspace(self, T, W):
        """the swap phase's scratch (int32; holds the permutations afterwards)"""
        import torch
        n = self.L.lfg_pt_workspace_size(T, W)
        if n == 0:
            raise RuntimeError("lfg_pt_workspace_size refuses T = %d, W = %d" % (T, W))
        if self._ws is None or self._ws.numel() * 4 < n:
            self._ws = torch.empty(n // 4, dtype=torch.int32, device=self.device)
        return self._ws

    def swap(self, pos, pos_out, lnl, lnpr, betas, seed, step, nswap):
        """swaps of one iteration: lnl / lnpr in place, the rows into pos_out"""
        T, W, ndim = pos.shape
        ws = self.workspace(T, W)
        rc = self.L.lfg_pt_swap(self._vp(pos), self._vp(pos_out), self._vp(lnl), self._vp(lnpr), T, W, ndim,
                                self._vp(betas), seed, step, self._vp(nswap), self._vp(ws), ws.numel() * 4,
                                _native.stream_ptr(self.device))
        _native.check(rc, "lfg_pt_swap")


class PTSampler:
    """ptemcee.Sampler's surface over T x W walkers on the device.

    evaluator(x [n, ndim], out=lnp [n], lnlike_e=[n, E]) on evaluator.device
    (batch.LnProbEvaluator, or any callable with that signature, a torch one
    included; E from evaluator.E or evaluator.tree.E).  It must satisfy
    ln_prob = ln_prior + sum_e lnlike_e wherever ln_prob is finite.
    ntemps / betas / Tmax: the ladder (default_betas; betas = any explicit
    one, betas[0] = 1, strictly decreasing, >= 0).
    ops: the move implementation (HipPTOps by default; CPU tests inject a
    host double).  cold_only: the stored chain keeps level 0 alone."""

    def __init__(self, nwalkers, ndim, evaluator, ntemps=None, betas=None, Tmax=None, a=2.0, seed=0, ops=None,
                 cold_only=False):
        import torch
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("the parallel-tempered sampler runs on one rank: its levels are not sharded "
                                      "over torch.distributed ranks (run usePT = 1 as a single process)")
        if nwalkers % 2 or nwalkers < 4:
            raise ValueError("nwalkers must be even and >= 4")
        self.W, self.ndim, self.a = int(nwalkers), int(ndim), float(a)
        if betas is None:
            betas = default_betas(self.ndim, ntemps, Tmax)
        betas = np.array(betas, dtype=np.float64).reshape(-1)
        if ntemps is not None and len(betas) != int(ntemps):
            raise ValueError("the ladder has %d levels, ntemps = %d" % (len(betas), int(ntemps)))
        if len(betas) < 1 or betas[0] != 1.0 or np.any(np.diff(betas) >= 0) or betas[-1] < 0:
            raise ValueError("betas must start at 1 and decrease strictly, none below 0")
        self.T = len(betas)
        self.ev = evaluator
        self.dev = evaluator.device
        self.E = int(getattr(evaluator, "E", 0) or evaluator.tree.E)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.ops = ops if ops is not None else HipPTOps(self.dev)
        self.cold_only = bool(cold_only)
        T, W, n = self.T, self.W, self.T * (self.W // 2)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self._betas = torch.as_tensor(betas, **f64)
        self._pos = torch.empty((T, W, self.ndim), **f64)
        self._alt = torch.empty((T, W, self.ndim), **f64)   # the swap phase gathers into it (ping-pong)
        self._lnl = torch.empty((T, W), **f64)
        self._lnpr = torch.empty((T, W), **f64)
        self.q = torch.empty((n, self.ndim), **f64)
        self.zfac = torch.empty(n, **f64)
        self.lnp_new = torch.empty(n, **f64)
        self.lle = torch.empty((n, self.E), **f64)
        self._naccept = torch.zeros((T, W), dtype=torch.int32, device=self.dev)
        self._nswap = torch.zeros((T, 2), dtype=torch.int64, device=self.dev)  # per pair (t, t-1): proposed, accepted
        self.iteration = 0
        self.rng_step = 0   # Philox step counter: monotone over the sampler's life (kept across reset())
        self._chunks = []   # stored runs: (chain [n, Ts, W, ndim], logpost [n, Ts, W], loglike [n, Ts, W])
        self._last = None
        self._started = False

    # ---- state
    @property
    def betas(self):
        return _host(self._betas)

    @property
    def ntemps(self):
        return self.T

    @property
    def nwalkers(self):
        return self.W

    @property
    def pos(self):
        return self._pos

    @property
    def loglike(self):
        return self._lnl

    @property
    def logprior(self):
        return self._lnpr

    @property
    def has_state(self):
        """True once a start was given (set_state, or p0 of sample / run_mcmc)"""
        return self._started

    def logpost(self):
        """betas[t] * ln_like + ln_prior, [T, W] (formed when asked for)"""
        return self._betas[:, None] * self._lnl + self._lnpr

    def set_state(self, p0):
        """Start from p0 [T, W, ndim]: one ln_prob call over all T * W walkers."""
        import torch
        p0 = torch.as_tensor(np.asarray(p0, dtype=np.float64))
        if tuple(p0.shape) != (self.T, self.W, self.ndim):
            raise ValueError("the start has shape %s, the sampler (ntemps, nwalkers, ndim) = %s"
                             % (tuple(p0.shape), (self.T, self.W, self.ndim)))
        self._pos.copy_(p0)
        n = self.T * self.W
        lnp = torch.empty(n, dtype=torch.float64, device=self.dev)
        lle = torch.empty((n, self.E), dtype=torch.float64, device=self.dev)
        self.ev(self._pos.view(n, self.ndim), out=lnp, lnlike_e=lle)
        ll = lle[:, 0].clone()
        for e in range(1, self.E):   # the kernels' order of summation
            ll += lle[:, e]
        if not bool(torch.isfinite(lnp).all()) or not bool(torch.isfinite(ll).all()):
            raise ValueError("the start has walkers with a non-finite log posterior")
        self._lnl.copy_(ll.view(self.T, self.W))
        self._lnpr.copy_((lnp - ll).view(self.T, self.W))
        self._naccept.zero_()
        self._nswap.zero_()
        self._started = True

    def step(self):
        """One iteration in place: both halves of every level, then the swaps."""
        if not self._started:
            raise RuntimeError("no state: pass p0 to sample() / run_mcmc() first")
        for half in (0, 1):
            self.ops.propose(self._pos, half, self.a, self.seed, self.rng_step, self.q, self.zfac)
            self.ev(self.q, out=self.lnp_new, lnlike_e=self.lle)
            self.ops.accept(self._pos, self._lnl, self._lnpr, half, self._betas, self.q, self.zfac, self.lnp_new,
                            self.lle, self.seed, self.rng_step, self._naccept)
        if self.T > 1:
            self.ops.swap(self._pos, self._alt, self._lnl, self._lnpr, self._betas, self.seed, self.rng_step,
                          self._nswap)
            self._pos, self._alt = self._alt, self._pos
        self.iteration += 1
        self.rng_step += 1

    # ---- ptemcee's surface (Sampler.sample / run_mcmc / reset / chain ...)
    def _begin(self, p0, iterations, thin, store):
        import torch
        if p0 is not None:
            self.set_state(p0)
        thin = max(1, int(thin))
        if not store:
            self._last = None
            return None, thin
        n = -(-int(iterations) // thin)
        Ts = 1 if self.cold_only else self.T
        f64 = dict(dtype=torch.float64, device=self.dev)
        buf = (torch.empty((n, Ts, self.W, self.ndim), **f64), torch.empty((n, Ts, self.W), **f64),
               torch.empty((n, Ts, self.W), **f64))
        return buf, thin

    def _store(self, buf, i, thin):
        if buf is not None and i % thin == 0:
            Ts = buf[0].shape[1]
            buf[0][i // thin].copy_(self._pos[:Ts])
            buf[1][i // thin].copy_(self.logpost()[:Ts])
            buf[2][i // thin].copy_(self._lnl[:Ts])

    def _end(self, buf, rows=None):
        """a stored run's chunk moves to host memory (as ptemcee keeps its chain)"""
        if buf is None:
            return
        if rows is not None:
            buf = tuple(b[:rows] for b in buf)
        self._last = tuple(b.cpu() for b in buf)
        self._chunks.append(self._last)

    def _report(self):
        return _host(self._pos), _host(self.logpost()), _host(self._lnl)

    def sample(self, p0=None, iterations=1, thin=1, storechain=True, store=None, **kwargs):
        """ptemcee's Sampler.sample: a generator over `iterations` steps
        yielding (pos [T, W, ndim], logpost [T, W], loglike [T, W]) as host
        arrays after each (mcmc_utils.py:200-216).  p0 None continues from the
        current state.  Each yield copies the ensemble to the host: the bulk,
        sync-free path is run_mcmc()."""
        buf, thin = self._begin(p0, iterations, thin, storechain if store is None else store)
        done = 0
        try:
            for i in range(int(iterations)):
                self.step()
                self._store(buf, i, thin)
                done = i + 1
                if done == int(iterations):
                    self._end(buf)
                    buf = None
                yield self._report()
        finally:
            if buf is not None:   # left early: the steps run are kept
                self._end(buf, rows=-(-done // thin))

    def run_mcmc(self, p0=None, iterations=1, thin=1, storechain=True, store=None, **kwargs):
        """`iterations` steps back to back (nothing crosses to the host until
        the end); returns (pos, logpost, loglike) of the last state."""
        buf, thin = self._begin(p0, iterations, thin, storechain if store is None else store)
        for i in range(int(iterations)):
            self.step()
            self._store(buf, i, thin)
        self._end(buf)
        return self._report()

    def last_run(self):
        """(chain [n, Ts, W, ndim], logpost [n, Ts, W], loglike [n, Ts, W]) of
        the most recent stored run as host tensors (Ts = 1 with cold_only),
        None if it stored nothing"""
        return self._last

    def reset(self):
        """ptemcee's reset: clears the chain and the acceptance and swap
        counters; the state and the RNG stream carry on (rng_step is kept)."""
        self.iteration = 0
        self._naccept.zero_()
        self._nswap.zero_()
        self._chunks = []
        self._last = None

    def _cat(self, k):
        import torch
        if not self._chunks:
            Ts = 1 if self.cold_only else self.T
            shape = (0, Ts, self.W, self.ndim) if k == 0 else (0, Ts, self.W)
            return torch.empty(shape, dtype=torch.float64)
        return torch.cat([c[k] for c in self._chunks])

    @property
    def chain(self):
        """host array [T, W, nsteps, ndim] ([1, ...] with cold_only)"""
        return _host(self._cat(0).permute(1, 2, 0, 3).contiguous())

    @property
    def logprobability(self):
        """the stored log posterior, [T, W, nsteps]"""
        return _host(self._cat(1).permute(1, 2, 0).contiguous())

    @property
    def loglikelihood(self):
        """the stored ln likelihood, [T, W, nsteps]"""
        return _host(self._cat(2).permute(1, 2, 0).contiguous())

    @property
    def flatchain(self):
        """[T, W * nsteps, ndim] (mcmcfit.py:326-329 takes [0])"""
        c = self.chain
        return c.reshape((c.shape[0], -1, self.ndim))

    @property
    def naccepted(self):
        return _host(self._naccept)

    @property
    def acceptance_fraction(self):
        """stretch moves accepted per slot and iteration, [T, W]"""
        return _host(self._naccept).astype(np.float64) / max(self.iteration, 1)

    @property
    def nswap(self):
        """[T, 2]: exchanges proposed and accepted between levels t and t - 1"""
        return _host(self._nswap)

    @property
    def tswap_acceptance_fraction(self):
        """per level, as ptemcee counts: the accepted share of the exchanges
        proposed to the level from either neighbour, [T] (zeros for T = 1)"""
        ns = self.nswap.astype(np.float64)
        both = ns.copy()
        both[:-1] += ns[1:]   # level t also takes part in pair (t + 1, t)
        return both[:, 1] / np.maximum(both[:, 0], 1.0)

    @property
    def random_state(self):
        """the Philox counter of the next iteration (the key is the seed)"""
        return self.rng_step

    @random_state.setter
    def random_state(self, step):
        self.rng_step = int(step)
