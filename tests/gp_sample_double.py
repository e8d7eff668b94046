"""Host test double of the device's conditional GP draws (lfg_gp_sample,
k_gp_smooth<true, false>; MODEL_SPEC 10.5): numpy Philox4x32-10 with the
kernel's counter layout and Box-Muller mapping, fed to the prior-path
simulation and the smoother of tests/gp_smoother.py.  No arithmetic of its
own beyond the normals: draw = f* + smooth(r - f* - ye z4).

  pair_from_words, block_normals
              two normals from one Philox block
  normals     the six normals of every (draw, point) of one vector
  draws       the conditional draws of one vector on the whole merged grid
  linear_map  the same draw as an exact affine map of its normals: the affine
              part is the conditional mean and A A^T the conditional
              covariance (tests/test_gp_sample_double.py holds both to the
              dense conditional)
  MUTATIONS   one convention flipped each; the tests use them to show that
              they would notice
  CASES       the named shapes tests/test_gpu_gp_sample_double.py runs on the
              device, built here so that the CPU test can assert what occurs
              in them

The angle.  cos and sin of 2 pi u are taken after an exact reduction by
quarter turns: a = 4 u, q = the nearest integer, r = a - q in [-1/2, 1/2]
(exact: a and q are multiples of 2^-51 below 4), then cos and sin of
r pi / 2, |r pi / 2| <= pi / 4, rotated by q.  The argument carries one
rounding of at most pi / 4, so both normals are right to an ulp or two;
cos(2 pi u) formed directly would lose up to 2 pi ulps absolute."""
import math

import numpy as np

from tests import gp_smoother as gs
from tests.stretch_double import MASK, philox, u53

MUTATIONS = ("point_draw_swapped", "gh_blocks_swapped", "eps_from_z5", "boxmuller_sin_first", "seed_hi_dropped",
             "first_ignored", "no_restart_at_block")


def _cossin2pi(u):
    a = 4.0 * np.asarray(u, np.float64)
    q = np.floor(a + 0.5)
    th = (a - q) * (0.5 * math.pi)
    c, s = np.cos(th), np.sin(th)
    k = q.astype(np.int64) & 3
    return np.choose(k, [c, -s, -c, s]), np.choose(k, [s, c, -s, -c])


def pair_from_words(w0, w1, w2, w3, mutate=None):
    """Box-Muller: radius from u53(w0, w1), angle from u53(w2, w3); the even
    normal is rad cos, the odd one rad sin"""
    rad = np.sqrt(-2.0 * np.log(1.0 - u53(w0, w1)))    # 1 - u in (0, 1]
    c, s = _cossin2pi(u53(w2, w3))
    return (rad * s, rad * c) if mutate == "boxmuller_sin_first" else (rad * c, rad * s)


def block_normals(c0, c1, c2, c3, k0, k1, mutate=None):
    return pair_from_words(*philox(c0, c1, c2, c3, k0, k1), mutate=mutate)


def normals(n, S, vkey, seed, mutate=None):
    """z [S, n, 6] of the vector keyed vkey: counter = (point on the merged
    grid, draw, vkey, j), key = (seed lo, seed hi); j = 0 gives (z0, z1) for
    g, j = 1 (z2, z3) for h, j = 2 z4 = eps (z5 is unused)"""
    p = np.broadcast_to(np.arange(n, dtype=np.uint64)[None, :], (S, n))
    s = np.broadcast_to(np.arange(S, dtype=np.uint64)[:, None], (S, n))
    if mutate == "point_draw_swapped":
        p, s = s, p
    k0 = np.uint64(seed) & MASK
    k1 = np.uint64(0) if mutate == "seed_hi_dropped" else np.uint64(seed) >> np.uint64(32)
    z = np.empty((S, n, 6))
    for j in range(3):
        jj = 1 - j if (mutate == "gh_blocks_swapped" and j < 2) else j
        z[:, :, 2 * j], z[:, :, 2 * j + 1] = block_normals(p, s, np.uint64(vkey) & MASK, np.uint64(jj), k0, k1, mutate)
    if mutate == "eps_from_z5":
        z[:, :, [4, 5]] = z[:, :, [5, 4]]
    return z


def _in_block(xm, blocks):
    return np.array([gs.block_of(v, blocks) >= 0 for v in xm])


def _prior(xm, hyp, blocks, xi, mutate=None):
    """gs.prior_path; no_restart_at_block: h runs on as one stationary
    process over the whole grid (prior_path with one block that holds every
    point) and is only switched on and off by the blocks"""
    if mutate != "no_restart_at_block":
        return gs.prior_path(xm, *hyp, blocks, xi)[0]
    st = gs.prior_path(xm, *hyp, [(-np.inf, np.inf)], xi)[1]
    return st[:, 0] + np.where(_in_block(xm, blocks), st[:, 2], 0.0)


def _draw(xm, yem, obs, rm, hyp, blocks, z, mutate=None):
    f = _prior(xm, hyp, blocks, z[:, :4], mutate)
    eps = np.where(obs != 0, yem * z[:, 4], 0.0)
    return f + gs.smooth(xm, yem, obs, rm - f - eps, *hyp, blocks, want_var=False)


def vkey_of(first, row, mutate=None):
    return int(row) if mutate == "first_ignored" else (int(first) + int(row)) % 2 ** 32


def draws(xm, yem, obs, rm, hyp, blocks, S, seed, first, row, mutate=None):
    """[S, n]: the S conditional draws of vector `row` of a call whose row 0
    is keyed `first`, on the whole merged grid.  rm [n] is the vector's
    residuals on the grid (anything where obs = 0)."""
    z = normals(len(xm), S, vkey_of(first, row, mutate), seed, mutate)
    rm = np.where(np.asarray(obs) != 0, rm, 0.0)
    return np.stack([_draw(xm, yem, obs, rm, hyp, blocks, z[s], mutate) for s in range(S)])


def linear_map(xm, yem, obs, rm, hyp, blocks, mutate=None):
    """(b [n], A [n, 5 n]): the draw as b + A z over the normals z[p, 0..4]
    of its points (column 5 p + c).  Formed from the two linear pieces the
    draw is made of, each probed with unit vectors: f* = L xi (prior_path)
    and smooth(r) = M r, so b = M r and A = (I - M) L - M diag(ye) on the
    eps columns; only data rows of M's argument count."""
    n = len(xm)
    obs = np.asarray(obs)
    rm = np.where(obs != 0, rm, 0.0)
    L = np.zeros((n, 4 * n))
    for j in range(4 * n):
        xi = np.zeros(4 * n)
        xi[j] = 1.0
        L[:, j] = _prior(xm, hyp, blocks, xi.reshape(n, 4), mutate)
    M = np.zeros((n, n))
    for k in np.flatnonzero(obs):
        e = np.zeros(n)
        e[k] = 1.0
        M[:, k] = gs.smooth(xm, yem, obs, e, *hyp, blocks, want_var=False)
    A = np.zeros((n, 5 * n))
    G = L - M @ L
    for c in range(4):
        A[:, c::5] = G[:, c::4]
    A[:, 4::5] = -M * np.where(obs != 0, yem, 0.0)[None, :]
    return gs.smooth(xm, yem, obs, rm, *hyp, blocks, want_var=False), A


# ------------------------------------------------------------------ the named cases
class Call:
    """One lfg_gp_sample call: W vectors over one (x, ye, t), S draws each"""

    def __init__(self, x, ye, res, hyp, blocks, t, S, seed, first=0):
        self.x, self.ye, self.t = (np.asarray(v, np.float64).reshape(-1) for v in (x, ye, t))
        self.res = np.atleast_2d(np.asarray(res, np.float64))
        self.W = self.res.shape[0]
        self.hyp = np.asarray(hyp, np.float64).reshape(self.W, 3)
        self.blocks = np.asarray(blocks, np.float64).reshape(self.W, -1, 2)
        self.nb = self.blocks.shape[1]
        self.S, self.seed, self.first = int(S), int(seed), int(first)
        self.xm, self.obs, self.ix, self.it = gs.merge(self.x, self.t)
        self.n = self.xm.size
        self.yem = np.zeros(self.n)
        self.yem[self.ix] = self.ye
        self.rm = np.zeros((self.W, self.n))
        self.rm[:, self.ix] = self.res

    def vector(self, w):
        return self.xm, self.yem, self.obs, self.rm[w], self.hyp[w], self.blocks[w]

    def draws(self, w, mutate=None):
        return draws(*self.vector(w), self.S, self.seed, self.first, w, mutate)

    def all_draws(self, mutate=None):
        """[W, S, n], lfg_gp_sample's out"""
        return np.stack([self.draws(w, mutate) for w in range(self.W)])

    def scale(self, w):
        return self.hyp[w, 0] + self.hyp[w, 1]

    def head(self, W):
        """the call of the first W vectors alone"""
        return Call(self.x, self.ye, self.res[:W], self.hyp[:W], self.blocks[:W], self.t, self.S, self.seed, self.first)


def _batch(seed, N, W, nb, extra, S, key, first=0):
    """W vectors over vector 0's (x, ye, t), each with the residuals,
    hyper-parameters and blocks of a make_case of its own"""
    cs = [gs.make_case(seed + 1000 * w, N, nb, extra) for w in range(W)]
    blocks = np.stack([c[4] for c in cs]) if nb else np.zeros((W, 0, 2))
    return Call(cs[0][0], cs[0][1], np.stack([c[2] for c in cs]), np.stack([c[3] for c in cs]), blocks, cs[0][5], S, key,
                first)


TAU_LO, TAU_HI = math.exp(-6.9), math.exp(-2.0)    # make_case's range of tau


def _steps(tau, seed):
    """Every kind of step on one grid of 40 points: tied data, test points on
    data, a test point 1e-13 after a datum, steps either side of s = 2 lam d
    = 1 at this tau, a gap of 0.15"""
    rng = np.random.default_rng(seed)
    xs = np.concatenate([np.linspace(-0.2, 0.02, 12), [0.02], np.linspace(0.17, 0.3, 11)])   # 0.02 twice; then the gap
    x = rng.permutation(xs)
    ye = rng.uniform(0.003, 0.006, x.size)
    r = 0.004 * rng.standard_normal(x.size)
    hyp = np.array([math.exp(-9.3), math.exp(-8.4), tau])
    blocks = np.array([[-0.97, -0.03], [0.03, 0.97]])
    # on data (one of them the tied pair), 1e-13 after a datum, on both blocks' inner edges, between the
    # blocks, before and after the data, three within 0.001 of each other
    t = np.array([0.25, xs[5], xs[4] + 1e-13, 0.02, xs[0], xs[-1], -0.03, 0.03, 0.5, 0.001, -0.25, 0.35, xs[15], 0.171,
                  0.1705, -0.119])
    return Call(x, ye, r, hyp, blocks, t, 4, 97 + seed)


def _build_cases():
    C = {}
    x1, ye1, r1, h1, _, _ = gs.make_case(1, 1, 0)
    C["one_point"] = [Call(x1, ye1, r1, h1, np.zeros((1, 0, 2)), [], 1, 11)]
    x2, ye2, r2, h2, b2, _ = gs.make_case(2, 1, 2)
    C["two_points"] = [Call(x2, ye2, r2, h2, b2, [0.12], 2, 12)]
    # make_case gives 16 + 3 nb + extra test points
    C["tile_31_32_33"] = [_batch(30 + n, n - 22, 2, 2, 0, 3, 13) for n in (31, 32, 33)]
    C["tiles_64_65_97"] = [_batch(60 + n, n - 27, 1, 3, 2, 5, 14) for n in (64, 65, 97)]
    wave = _batch(65, 11, 65, 2, 0, 1, 15)
    C["wave_63_64_65"] = [wave.head(63), wave.head(64), wave]
    C["straddle"] = [_batch(43, 11, 3, 2, 0, 43, 16)]
    C["keys"] = [_batch(7, 11, 2, 2, 0, 3, 2 ** 40 + 7, first) for first in (5, 2 ** 31 - 1)]
    C["steps"] = [_steps(TAU_LO, 1), _steps(TAU_HI, 2)]
    return C


CASES = _build_cases()
