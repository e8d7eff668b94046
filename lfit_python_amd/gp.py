"""The Gaussian-process likelihood of the reference's GP trees, on the GPU.

Replaces the george objects SimpleGPEclipse builds (CVModel.py:603-696):
  kernel = ampin * kernels.Matern32Kernel(tau)                 CVModel.py:636
  kernel += ampout * kernels.Matern32Kernel(tau, block=gap)    CVModel.py:639-642
  gp = GP(kernel, solver=HODLRSolver)                          CVModel.py:645
  gp.compute(x, ye); gp.log_likelihood(residuals, quiet=True)  CVModel.py:687-691
and the posterior calls of plot_lc_model.plot_GP_eclipse
  gp.sample_conditional(residuals, x, size=300)                plot_lc_model.py:229
  gp.predict(residuals, t)
with the same call shapes.  The likelihood is exact (george's HODLR solver
approximates it) and costs O(N): lfg_gp_lnlike runs a 4-state Kalman filter
over the phase-sorted points (MODEL_SPEC.md section 10).  Only the kernel
family the reference builds is supported: one global Matern-3/2 term plus
Matern-3/2 terms of one common amplitude restricted to blocks, all with the
same metric.  The posterior is exact and O(N + M) as well: a smoother over
the merged grid of data and test phases (lfg_gp_predict, MODEL_SPEC 10.5).
"""
import ctypes

import numpy as np

from . import _native


class _Kernel:
    """A sum of amp * Matern32(metric) terms, each optionally on a block."""

    def __init__(self, terms):
        self.terms = list(terms)

    def __rmul__(self, a):
        return _Kernel([(float(a) * amp, metric, blk) for amp, metric, blk in self.terms])

    __mul__ = __rmul__

    def __add__(self, other):
        return _Kernel(self.terms + other.terms)


class kernels:  # noqa: N801 - mirrors george.kernels
    @staticmethod
    def Matern32Kernel(metric, block=None):  # noqa: N802 - george's name
        """george: k(r^2) = (1 + sqrt(3 r^2)) exp(-sqrt(3 r^2)), r^2 = d^2 / metric;
        with block = (lo, hi), zero unless both points lie in [lo, hi]."""
        blk = None if block is None else tuple(float(v) for v in np.atleast_2d(block)[0])
        return _Kernel([(1.0, float(metric), blk)])


HODLRSolver = None  # accepted and ignored: the solve is exact


def _split(kernel):
    glob = [t for t in kernel.terms if t[2] is None]
    blk = [t for t in kernel.terms if t[2] is not None]
    metrics = {t[1] for t in kernel.terms}
    if len(glob) != 1 or len(metrics) != 1 or len({t[0] for t in blk}) > 1:
        raise NotImplementedError("only ampin*M32(tau) + sum_k ampout*M32(tau, block_k) is supported")
    ampout = blk[0][0] if blk else 0.0
    return glob[0][0], ampout, metrics.pop(), [t[2] for t in blk]


def log_likelihood_batch(x, ye, res, hyp, blocks, device=None):
    """GP log-likelihoods of W residual vectors on the GPU.

    x, ye [N] (any order); res [W, N]; hyp [W, 3] = ampin, ampout, tau;
    blocks [W, nb, 2].  Returns a numpy array [W]."""
    import torch
    _native.require_gpu()
    L = _native.lib()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    order = np.argsort(x, kind="stable")  # the filter runs over sorted phases
    res = np.atleast_2d(np.asarray(res, dtype=np.float64))[:, order]
    W, N = res.shape
    hyp = np.ascontiguousarray(np.asarray(hyp, dtype=np.float64).reshape(W, 3))
    blocks = np.asarray(blocks, dtype=np.float64).reshape(W, -1, 2)
    nb = blocks.shape[1]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    xt, yt, rt, ht = t(x[order]), t(np.asarray(ye, dtype=np.float64).reshape(-1)[order]), t(res), t(hyp)
    bt = t(blocks if nb else np.zeros((W, 1, 2)))
    out = torch.empty(W, dtype=torch.float64, device=dev)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    rc = L.lfg_gp_lnlike(vp(xt), vp(yt), vp(rt), W, N, vp(ht), vp(bt), nb, vp(out), _native.stream_ptr(dev))
    _native.check(rc, "lfg_gp_lnlike")
    return out.cpu().numpy()


def _m32(d, tau):
    s = np.sqrt(3.0 * d * d / tau)
    return (1.0 + s) * np.exp(-s)


def _kernel_matrix(a, b, ampin, ampout, tau, blocks):
    """k(a_i, b_j) of MODEL_SPEC 10.1 (host side: the right-hand sides and the
    prior term of predict's full covariance)"""
    base = _m32(a[:, None] - b[None, :], tau)
    K = ampin * base
    for lo, hi in blocks:
        K = K + ampout * base * (((a >= lo) & (a <= hi))[:, None] & ((b >= lo) & (b <= hi))[None, :])
    return K


class _Merged:
    """Data phases x (any order) and test phases t on one sorted grid, on the
    device: the arguments lfg_gp_predict and lfg_gp_sample share."""

    def __init__(self, x, ye, res, hyp, blocks, t, device):
        import torch
        _native.require_gpu()
        self.dev = dev = (torch.device(device) if device is not None
                          else torch.device("cuda", torch.cuda.current_device()))
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        res = np.atleast_2d(np.asarray(res, dtype=np.float64))
        self.W, N = res.shape
        if x.size != N:
            raise ValueError("res has %d points per vector, x has %d" % (N, x.size))
        self.M, self.n = t.size, N + t.size
        z = np.concatenate([x, t])
        order = np.argsort(z, kind="stable")
        inv = np.empty(self.n, dtype=np.int64)
        inv[order] = np.arange(self.n)
        self.it = inv[N:]                       # where each test point sits on the grid
        rm = np.zeros((self.W, self.n))
        rm[:, inv[:N]] = res
        yem = np.zeros(self.n)
        ye = np.asarray(ye, dtype=np.float64)
        yem[inv[:N]] = ye.reshape(-1) if ye.size == N else np.broadcast_to(ye, x.shape)
        hyp = np.ascontiguousarray(np.asarray(hyp, dtype=np.float64).reshape(self.W, 3))
        blocks = np.asarray(blocks, dtype=np.float64).reshape(self.W, -1, 2)
        self.nb = blocks.shape[1]
        if self.nb > _native.GP_PREDICT_MAX_NB:
            raise NotImplementedError("at most %d changepoint blocks per vector" % _native.GP_PREDICT_MAX_NB)
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        self.x, self.ye, self.res, self.hyp = f64(z[order]), f64(yem), f64(rm), f64(hyp)
        self.obs = torch.as_tensor((order < N).astype(np.int32), device=dev)
        self.blocks = f64(blocks if self.nb else np.zeros((self.W, 1, 2)))
        self.status = torch.empty(self.W, dtype=torch.int32, device=dev)
        self.it_dev = torch.as_tensor(self.it, device=dev)

    def head(self):
        vp = lambda a: ctypes.c_void_p(a.data_ptr())
        return [vp(self.x), vp(self.ye), vp(self.obs), vp(self.res), self.W, self.n, vp(self.hyp), vp(self.blocks),
                self.nb]


def predict_batch(x, ye, res, hyp, blocks, t, return_var=True, device=None, return_status=False):
    """Conditional mean and variance of the GP at test phases t, for W
    residual vectors on the GPU (george's gp.predict(r, t, return_var=True),
    batched).

    x, ye [N] and t [M] in any order; res [W, N]; hyp [W, 3] = ampin, ampout,
    tau; blocks [W, nb, 2].  Returns numpy (mean [W, M], var [W, M]), or mean
    alone with return_var=False; with return_status=True the status [W] is
    appended: a non-zero entry marks a vector whose rows are NaN (a non-finite
    residual, an invalid hyper-parameter or a covariance that is not positive
    definite)."""
    import torch
    L = _native.lib()
    g = _Merged(x, ye, res, hyp, blocks, t, device)
    mean = torch.empty((g.W, g.n), dtype=torch.float64, device=g.dev)
    var = torch.empty((g.W, g.n), dtype=torch.float64, device=g.dev) if return_var else None
    nbytes = L.lfg_gp_predict_workspace_size(g.W, g.n)
    ws = _native.Workspace.get(nbytes, g.dev)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    rc = L.lfg_gp_predict(*g.head(), vp(mean), vp(var) if return_var else None, vp(g.status), vp(ws), nbytes,
                          _native.stream_ptr(g.dev))
    _native.check(rc, "lfg_gp_predict")
    out = [mean[:, g.it_dev].cpu().numpy()]
    if return_var:
        out.append(var[:, g.it_dev].cpu().numpy())
    if return_status:
        out.append(g.status.cpu().numpy())
    return out[0] if len(out) == 1 else tuple(out)


def sample_conditional_batch(x, ye, res, hyp, blocks, t, size, seed=0, device=None, return_status=False, first=0):
    """`size` draws of the GP at t conditioned on each of W residual vectors
    (george's gp.sample_conditional, batched): numpy [W, size, M].  Matheron's
    rule on the GPU: a prior path over the merged grid plus the smoother's
    mean of what it leaves unexplained (MODEL_SPEC 10.5).  The draws depend
    on (seed, first + vector, draw, point) alone: a batch cut into several
    calls, each with `first` the index of its row 0, gives the same bits."""
    import torch
    L = _native.lib()
    size = int(size)
    if size < 1:
        raise ValueError("size must be at least 1")
    g = _Merged(x, ye, res, hyp, blocks, t, device)
    out = torch.empty((g.W, size, g.n), dtype=torch.float64, device=g.dev)
    nbytes = L.lfg_gp_sample_workspace_size(g.W, g.n, size)
    if nbytes == 0:
        raise ValueError("W * size = %d is beyond the sampler's 2^30 vectors" % (g.W * size))
    ws = _native.Workspace.get(nbytes, g.dev)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    rc = L.lfg_gp_sample(*g.head(), size, int(seed) & (2 ** 64 - 1), int(first), vp(out), vp(g.status), vp(ws), nbytes,
                         _native.stream_ptr(g.dev))
    _native.check(rc, "lfg_gp_sample")
    draws = out[:, :, g.it_dev].cpu().numpy()
    return (draws, g.status.cpu().numpy()) if return_status else draws


class GP:
    """george.GP for the kernel of CVModel.py:636-645."""

    def __init__(self, kernel, solver=None, device=None):
        self.kernel = kernel
        self.ampin, self.ampout, self.tau, self.blocks = _split(kernel)
        self.device = device
        self.x = self.ye = None

    def compute(self, x, yerr):
        self.x = np.asarray(x, dtype=np.float64)
        self.ye = np.broadcast_to(np.asarray(yerr, dtype=np.float64), self.x.shape)

    def log_likelihood(self, y, quiet=False):
        if self.x is None:
            raise RuntimeError("call compute(x, yerr) first")
        blocks = np.asarray(self.blocks, dtype=np.float64).reshape(1, -1, 2)
        ll = float(log_likelihood_batch(self.x, self.ye, np.asarray(y)[None, :],
                                        [[self.ampin, self.ampout, self.tau]], blocks, self.device)[0])
        if not np.isfinite(ll) and not quiet:
            raise ValueError("the GP covariance is not positive definite")
        return ll

    def _args(self, y):
        if self.x is None:
            raise RuntimeError("call compute(x, yerr) first")
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        if y.size != self.x.size:
            raise ValueError("y has %d points, compute() was given %d" % (y.size, self.x.size))
        return y, [[self.ampin, self.ampout, self.tau]], np.asarray(self.blocks, dtype=np.float64).reshape(1, -1, 2)

    def predict(self, y, t, return_cov=True, return_var=False):
        """george's GP.predict: mu [M]; (mu, var) with return_var; (mu, cov
        [M, M]) by default.  The full covariance is M more vectors through the
        mean-only smoother: k(t_i, t_j) - k_i^T K^-1 k_j, the second term the
        conditional mean at t_i of the kernel column k(x, t_j)."""
        y, hyp, blocks = self._args(y)
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if return_var:
            mu, var, st = predict_batch(self.x, self.ye, y[None, :], hyp, blocks, t, True, self.device, True)
            self._raise(st)
            return mu[0], var[0]
        if not return_cov:
            mu, st = predict_batch(self.x, self.ye, y[None, :], hyp, blocks, t, False, self.device, True)
            self._raise(st)
            return mu[0]
        x = self.x.reshape(-1)
        cols = _kernel_matrix(t, x, self.ampin, self.ampout, self.tau, self.blocks)   # [M, N]
        m, st = predict_batch(x, self.ye, np.vstack([y[None, :], cols]), np.repeat(hyp, 1 + t.size, 0),
                              np.repeat(blocks, 1 + t.size, 0), t, False, self.device, True)
        self._raise(st[:1])
        A = m[1:]
        cov = _kernel_matrix(t, t, self.ampin, self.ampout, self.tau, self.blocks) - 0.5 * (A + A.T)
        return m[0], cov

    def sample_conditional(self, y, t, size=1, seed=None):
        """george's GP.sample_conditional: [size, M] draws at t given y, [M]
        when size == 1.  seed=None takes one from numpy's global generator."""
        y, hyp, blocks = self._args(y)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 62))
        draws, st = sample_conditional_batch(self.x, self.ye, y[None, :], hyp, blocks, t, size, seed, self.device,
                                             True)
        self._raise(st)
        return draws[0, 0] if int(size) == 1 else draws[0]

    @staticmethod
    def _raise(status):
        if np.any(status != 0):
            raise ValueError("the GP has no posterior here: non-finite residuals, an invalid hyper-parameter or a "
                             "covariance that is not positive definite")
