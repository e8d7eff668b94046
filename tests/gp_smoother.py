"""Test helper: the GP posterior of MODEL_SPEC 10.5 restated in numpy.

  dense_predict   the definition: K from MODEL_SPEC 10.1, a dense solve
  merge           data and test phases into one sorted grid (obs = 0: test)
  smooth          the forward filter and the modified Bryson-Frazier backward
                  pass that lfg_device.hpp's GPForward / GPBackward run, with
                  plain 4 x 4 matrices
  step_noise, prior_path
                  the state-space simulation of a prior path (Matheron's rule)
"""
import math

import numpy as np

from tests.gp_kalman import block_of


def m32(d, tau):
    s = np.sqrt(3.0 * d * d / tau)
    return (1.0 + s) * np.exp(-s)


def kernel(a, b, ampin, ampout, tau, blocks):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    base = m32(a[:, None] - b[None, :], tau)
    K = ampin * base
    for lo, hi in blocks:
        ia, ib = (a >= lo) & (a <= hi), (b >= lo) & (b <= hi)
        K = K + ampout * base * (ia[:, None] & ib[None, :])
    return K


def dense_predict(x, ye, r, ampin, ampout, tau, blocks, t):
    """(mean [M], cov [M, M]) of the latent process at t given r at x"""
    x, ye, r, t = (np.asarray(v, dtype=np.float64) for v in (x, ye, r, t))
    K = kernel(x, x, ampin, ampout, tau, blocks) + np.diag(ye * ye)
    Ks = kernel(x, t, ampin, ampout, tau, blocks)
    sol = np.linalg.solve(K, np.column_stack([r, Ks]))
    return Ks.T @ sol[:, 0], kernel(t, t, ampin, ampout, tau, blocks) - Ks.T @ sol[:, 1:]


def merge(x, t):
    """The sorted grid of data x (any order) and test points t: (xm [n],
    obs [n], idx_x [N], idx_t [M]) with xm[idx_x] = x, xm[idx_t] = t."""
    x, t = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(t, dtype=np.float64).reshape(-1)
    z = np.concatenate([x, t])
    order = np.argsort(z, kind="stable")
    inv = np.empty(z.size, dtype=np.int64)
    inv[order] = np.arange(z.size)
    obs = (order < x.size).astype(np.int32)
    return z[order], obs, inv[:x.size], inv[x.size:]


def _phi(lam, d):
    u = lam * d
    e = math.exp(-u)
    F2 = e * np.array([[1.0 + u, d], [-lam * u, 1.0 - u]])
    F = np.zeros((4, 4))
    F[:2, :2] = F2
    F[2:, 2:] = F2
    return F


def smooth(x, ye, obs, r, ampin, ampout, tau, blocks, want_var=True):
    """(mean [n], var [n]) at every point of the sorted merged grid"""
    x, ye, r = (np.asarray(v, dtype=np.float64) for v in (x, ye, r))
    n = len(x)
    assert np.all(np.diff(x) >= 0)
    lam = math.sqrt(3.0 / tau)
    pinf = np.diag([ampin, ampin * lam * lam, ampout, ampout * lam * lam])
    m, P = np.zeros(4), pinf.copy()
    blk = [block_of(v, blocks) for v in x]
    rec, Fs = [], []
    for i in range(n):
        F = np.eye(4)
        if i > 0:
            F = _phi(lam, x[i] - x[i - 1])
        fresh = blk[i] >= 0 and blk[i] != (blk[i - 1] if i > 0 else -1)
        if fresh:
            F[2:, :] = 0.0
        if i > 0:
            m = F @ m
            D = F @ (P - pinf) @ F.T
            if fresh:
                D[2:, :] = 0.0
                D[:, 2:] = 0.0
            P = D + pinf
        H = np.array([1.0, 0.0, 1.0 if blk[i] >= 0 else 0.0, 0.0])
        k = P @ H
        yhat = H @ m
        S, v = 1.0, 0.0
        if obs[i]:
            S = H @ k + ye[i] * ye[i]
            v = r[i] - yhat
            m = m + k * (v / S)
            P = P - np.outer(k, k) / S
        rec.append((k, S, v, yhat, H))
        Fs.append(F)
    lamh, Lam = np.zeros(4), np.zeros((4, 4))
    mean, var = np.empty(n), np.empty(n)
    for i in range(n - 1, -1, -1):
        k, S, v, yhat, H = rec[i]
        if obs[i]:
            C = np.eye(4) - np.outer(k, H) / S
            Lam = np.outer(H, H) / S + C.T @ Lam @ C
            lamh = -H * v / S + C.T @ lamh
        mean[i] = yhat - k @ lamh
        var[i] = max(H @ k - k @ Lam @ k, 0.0)
        Lam = Fs[i].T @ Lam @ Fs[i]
        lamh = Fs[i].T @ lamh
    return (mean, var) if want_var else mean


def step_noise(lam, d):
    """Lower Cholesky factor [[c00, 0], [c10, c11]] of Q / a, Q = Pinf - Phi
    Pinf Phi^T, free of cancellation (gp_step_noise in lfg_device.hpp)"""
    s = 2.0 * lam * d
    e = math.exp(-s)
    if s < 1.0:
        t3 = 0.0
        for k in range(22, 3, -1):
            t3 = (1.0 + t3) * s / k
        t3 = (1.0 + t3) * s * s * s / 6.0
        q00, q11 = e * t3, e * (2.0 * s + t3)
    else:
        q00 = 1.0 - e * (1.0 + s + 0.5 * s * s)
        q11 = 1.0 - e * (1.0 - s + 0.5 * s * s)
    q01 = 0.5 * e * s * s
    if not q00 > 0.0:
        return np.zeros((2, 2))
    c00 = math.sqrt(q00)
    return np.array([[c00, 0.0], [lam * q01 / c00, lam * math.sqrt(max(q11 - q01 * q01 / q00, 0.0))]])


def prior_path(x, ampin, ampout, tau, blocks, xi):
    """A prior draw f* [n] over the sorted grid from normals xi [n, 4], and
    the states [n, 4] behind it"""
    x = np.asarray(x, dtype=np.float64)
    lam = math.sqrt(3.0 / tau)
    sa = np.array([math.sqrt(ampin), math.sqrt(ampin), math.sqrt(ampout), math.sqrt(ampout)])
    stat = sa * np.array([1.0, lam, 1.0, lam])
    st = np.empty((len(x), 4))
    f = np.empty(len(x))
    s = stat * xi[0]
    bp = -1
    for i in range(len(x)):
        blk = block_of(x[i], blocks)
        if i > 0:
            d = x[i] - x[i - 1]
            c = step_noise(lam, d)
            noise = np.concatenate([c @ xi[i, :2], c @ xi[i, 2:]]) * sa
            s = _phi(lam, d) @ s + noise
            if blk >= 0 and blk != bp:
                s[2:] = stat[2:] * xi[i, 2:]
        bp = blk
        st[i] = s
        f[i] = s[0] + (s[2] if blk >= 0 else 0.0)
    return f, st


# the project's GP bar on the natural scale: sqrt(ampin + ampout) for the
# mean, ampin + ampout for the variance (both forms are exact in FP64)
BAR = 1e-9


def make_case(seed, N, nb, extra=0):
    """x, ye, r, hyp, blocks, t: the hyper-parameter ranges of
    test_gp_kernel_matches_dense_oracle; t before, after and on the data, on
    a block's lo and hi exactly, inside and outside blocks (16 + 3 nb + extra of
    them)"""
    rng = np.random.default_rng(seed)
    x = rng.permutation(np.linspace(-0.2, 0.3, N)) if N > 1 else np.array([0.07])
    ye = rng.uniform(0.003, 0.006, N)
    r = 0.004 * rng.standard_normal(N)
    hyp = np.array([np.exp(rng.uniform(-11, -8)), np.exp(rng.uniform(-11, -8)), np.exp(rng.uniform(-6.9, -2))])
    d = rng.uniform(0.01, 0.05)
    blocks = np.array([[-1 + d, -d], [d, 1 - d], [-d / 2, d / 2]])[:nb]
    t = [-0.31, -0.25, 0.31, 0.4, x[0], x[N // 2], x[-1], 0.0, -0.1, 0.1, -0.2]
    for lo, hi in blocks:
        t += [lo, hi, 0.5 * (max(lo, -0.3) + min(hi, 0.4))]
    t = np.array(t + list(rng.uniform(-0.3, 0.4, 5 + extra)))
    return x, ye, r, hyp, blocks, t


def check(mean, var, x, ye, r, hyp, blocks, t):
    mu, cov = dense_predict(x, ye, r, *hyp, blocks, t)
    scale = hyp[0] + hyp[1]
    em = np.max(np.abs(mean - mu)) / np.sqrt(scale)
    assert em <= BAR, ("mean", em)
    if var is not None:
        ev = np.max(np.abs(var - np.diag(cov))) / scale
        assert ev <= BAR, ("var", ev)
