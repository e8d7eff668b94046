"""CPU: the host double of the device's conditional GP draws
(tests/gp_sample_double.py) anchored outside itself, so that the GPU
comparison against it (tests/test_gpu_gp_sample_double.py) cannot pass on a
mistake the double shares with the kernel: its normals against normals
computed by hand from the Philox words, its law (the affine part and A A^T of
the draw's exact linear map) against the dense conditional at every merged
point of every case, each mutation told by a named case, and the populations
of the cases the device runs."""
import math

import numpy as np
import pytest

from tests import gp_sample_double as gd
from tests import gp_smoother as gs
from tests import stretch_double as sd
from tests.test_stretch_double import KAT

BAR = gs.BAR
TELLS = 1e3 * BAR      # a mutation is told when it moves a draw by more than this, in sqrt(ampin + ampout)


def _by_hand(words):
    w0, w1, w2, w3 = (int(w) for w in words)
    u = ((w0 >> 5) * 2 ** 26 + (w1 >> 6)) / 2.0 ** 53
    a = ((w2 >> 5) * 2 ** 26 + (w3 >> 6)) / 2.0 ** 53
    rad = math.sqrt(-2.0 * math.log(1.0 - u))
    return rad * math.cos(2.0 * math.pi * a), rad * math.sin(2.0 * math.pi * a), rad


def test_normals_of_a_known_answer_counter():
    """Random123's digits-of-pi vector: its published output words, Box-Muller by hand"""
    ctr, key, want = KAT[2]
    words = [int(h, 16) for h in want.split()]
    z0, z1, rad = _by_hand(words)
    got = gd.block_normals(*ctr, *key)
    # the hand's angle 2 pi a carries up to 2 pi ulps; the double's is reduced first
    assert abs(float(got[0]) - z0) <= 4e-15 * rad and abs(float(got[1]) - z1) <= 4e-15 * rad
    assert abs(z0) > 0.1 and abs(z1) > 0.1 and abs(abs(z0) - abs(z1)) > 0.1    # cos and sin, signs: all told
    s0, s1 = gd.block_normals(*ctr, *key, mutate="boxmuller_sin_first")
    assert float(s0) == float(got[1]) and float(s1) == float(got[0])


def test_normals_counter_layout_by_hand():
    """normals()[draw, point, 2 j + k] is word pair k of philox((point, draw, vkey, j), (seed lo, seed hi))"""
    n, S, vkey, seed = 3, 2, 2 ** 31 + 4, 2 ** 40 + 7
    z = gd.normals(n, S, vkey, seed)
    assert z.shape == (S, n, 6)
    for (draw, p, j) in ((1, 2, 2), (0, 1, 0), (1, 0, 1)):
        words = sd.philox(p, draw, vkey, j, seed & 0xFFFFFFFF, seed >> 32)
        z0, z1, rad = _by_hand(words)
        assert abs(z[draw, p, 2 * j] - z0) <= 4e-15 * rad and abs(z[draw, p, 2 * j + 1] - z1) <= 4e-15 * rad
    flat = z.reshape(-1)
    assert len(set(flat.tolist())) == flat.size and np.isfinite(flat).all()
    # the angle's reduction at its seams: exact at the quarter turns, an ulp or two elsewhere
    u = np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0 - 2.0 ** -53, 0.3, 0.7])
    c, s = gd._cossin2pi(u)
    assert np.array_equal(c[[0, 2, 4, 6]], [1.0, 0.0, -1.0, 0.0]) and np.array_equal(s[[0, 2, 4, 6]], [0.0, 1.0, 0.0, -1.0])
    assert np.max(np.abs(c - np.cos(2 * np.pi * u))) <= 2e-15 and np.max(np.abs(s - np.sin(2 * np.pi * u))) <= 2e-15


# ------------------------------------------------------------------ the law
def _vectors(name):
    """(call index, vector) of every distinct problem of a case: a call that
    repeats another's vectors (wave_63_64_65's heads) adds none"""
    calls = gd.CASES[name]
    if name == "wave_63_64_65":
        return [(2, w) for w in range(calls[2].W)]
    if name == "keys":
        return [(0, w) for w in range(calls[0].W)]      # the second call differs in `first` alone
    return [(k, w) for k, c in enumerate(calls) for w in range(c.W)]


@pytest.fixture(scope="module")
def law():
    """per case: (max mean error / sqrt(scale), max covariance error / scale) over its vectors"""
    out = {}
    for name in gd.CASES:
        em = ev = 0.0
        for k, w in _vectors(name):
            c = gd.CASES[name][k]
            b, A = gd.linear_map(*c.vector(w))
            # the latent conditional at every merged point, the data included (t = xm)
            mu, cov = gs.dense_predict(c.x, c.ye, c.res[w], *c.hyp[w], c.blocks[w], c.xm)
            em = max(em, np.max(np.abs(b - mu)) / np.sqrt(c.scale(w)))
            ev = max(ev, np.max(np.abs(A @ A.T - cov)) / c.scale(w))
        out[name] = (em, ev)
    return out


@pytest.mark.parametrize("name", list(gd.CASES))
def test_law_is_the_dense_conditional(law, name):
    em, ev = law[name]
    print("law %-16s mean %.2e sqrt(scale)  cov %.2e scale" % (name, em, ev))
    assert em <= BAR, ("mean", em)
    assert ev <= BAR, ("cov", ev)


def test_linear_map_is_the_draw():
    """b + A z at the Philox normals reproduces draws(): the map the law test
    holds is the map of the draws the device is compared with"""
    for name in ("two_points", "tile_31_32_33", "steps", "keys"):
        c = gd.CASES[name][-1]
        w = c.W - 1
        b, A = gd.linear_map(*c.vector(w))
        z = gd.normals(c.n, c.S, gd.vkey_of(c.first, w), c.seed)
        want = b[None, :] + z[:, :, :5].reshape(c.S, -1) @ A.T
        assert np.max(np.abs(c.draws(w) - want)) <= 1e-12 * np.sqrt(c.scale(w)), name


# ------------------------------------------------------------------ mutations
@pytest.fixture(scope="module")
def told():
    """distance[mutation][case]: the largest move of any draw, in sqrt(scale)"""
    out = {}
    for name, calls in gd.CASES.items():
        pairs = [(c, w) for c in ([calls[-1]] if name == "wave_63_64_65" else calls) for w in range(c.W)]
        if name in ("wave_63_64_65", "straddle"):
            pairs = pairs[:3]          # every vector of these is alike to a mutation
        base = [(c, w, c.draws(w)) for c, w in pairs]
        for m in gd.MUTATIONS:
            out.setdefault(m, {})[name] = max(np.max(np.abs(c.draws(w, m) - d)) / np.sqrt(c.scale(w))
                                              for c, w, d in base)
    return out


# which case must tell which mutation (the cases built for it); any other case may tell it too
MUST_TELL = {"point_draw_swapped": "two_points", "gh_blocks_swapped": "one_point", "eps_from_z5": "one_point",
             "boxmuller_sin_first": "one_point", "seed_hi_dropped": "keys", "first_ignored": "keys",
             "no_restart_at_block": "steps"}


@pytest.mark.parametrize("mutation", gd.MUTATIONS)
def test_every_mutation_is_told(told, mutation):
    d = told[mutation]
    print("mutation %-20s " % mutation + "  ".join("%s %.1e" % kv for kv in d.items()))
    assert d[MUST_TELL[mutation]] > TELLS, d
    if mutation in ("seed_hi_dropped", "first_ignored"):
        # nothing else has a seed beyond 32 bits or a first above 0
        assert all(v == 0.0 for k, v in d.items() if k != "keys"), d


def test_no_restart_fails_the_covariance():
    """h carried across a gap between blocks is a wrong law, not only other bits"""
    c = gd.CASES["steps"][1]
    _, A = gd.linear_map(*c.vector(0), mutate="no_restart_at_block")
    _, cov = gs.dense_predict(c.x, c.ye, c.res[0], *c.hyp[0], c.blocks[0], c.xm)
    ev = np.max(np.abs(A @ A.T - cov)) / c.scale(0)
    print("no_restart_at_block: covariance off by %.2e scale" % ev)
    assert ev > TELLS


# ------------------------------------------------------------------ populations
def _steps_of(c, w):
    lam = math.sqrt(3.0 / c.hyp[w, 2])
    d = np.diff(c.xm)
    return d, 2.0 * lam * d


def test_case_shapes():
    C = gd.CASES
    shape = lambda name: [(c.n, c.W, c.S, c.nb) for c in C[name]]
    assert shape("one_point") == [(1, 1, 1, 0)] and C["one_point"][0].t.size == 0
    assert shape("two_points") == [(2, 1, 2, 2)]
    assert shape("tile_31_32_33") == [(31, 2, 3, 2), (32, 2, 3, 2), (33, 2, 3, 2)]
    assert shape("tiles_64_65_97") == [(64, 1, 5, 3), (65, 1, 5, 3), (97, 1, 5, 3)]
    assert shape("wave_63_64_65") == [(33, 63, 1, 2), (33, 64, 1, 2), (33, 65, 1, 2)]
    assert shape("straddle") == [(33, 3, 43, 2)]
    assert shape("keys") == [(33, 2, 3, 2)] * 2
    assert [(c.seed, c.first) for c in C["keys"]] == [(2 ** 40 + 7, 5), (2 ** 40 + 7, 2 ** 31 - 1)]
    assert shape("steps") == [(40, 1, 4, 2)] * 2
    assert [c.hyp[0, 2] for c in C["steps"]] == [gd.TAU_LO, gd.TAU_HI]
    wave = C["wave_63_64_65"][2]
    assert len({wave.hyp[w].tobytes() + wave.blocks[w].tobytes() for w in range(65)}) == 65
    for calls in C.values():
        for c in calls:
            assert np.array_equal(c.xm[c.ix], c.x) and np.array_equal(c.xm[c.it], c.t) and np.all(np.diff(c.xm) >= 0)
            assert np.all(c.blocks[:, :, 0] < c.blocks[:, :, 1])


def test_case_populations():
    C = gd.CASES
    for c in C["steps"]:
        d, s = _steps_of(c, 0)
        assert (s[d > 0] < 1.0).sum() >= 3 and (s >= 1.0).sum() >= 2, (c.hyp[0, 2], s)    # both gp_step_noise branches
        tied = d == 0
        assert np.any(tied & (c.obs[1:] == 1) & (c.obs[:-1] == 1))       # a tied pair of data
        assert np.any(tied & (c.obs[1:] != c.obs[:-1]))                  # a test point on a datum
        tiny = (d > 0.5e-13) & (d < 2e-13)
        assert tiny.sum() == 1 and c.obs[1:][tiny][0] == 0 and c.obs[:-1][tiny][0] == 1    # 1e-13 after a datum
        blk = np.array([gs.block_of(v, c.blocks[0]) for v in c.xm])
        assert blk[0] == 0                                               # a block holds p = 0
        opens = np.flatnonzero((blk[1:] >= 0) & (blk[1:] != blk[:-1])) + 1
        assert opens.size == 1 and blk[opens[0]] == 1 and blk[opens[0] - 1] == -1    # one opens at p > 0, after a gap
        assert (blk == -1).sum() >= 3                                    # points outside every block
        assert c.xm[opens[0]] == c.blocks[0, 1, 0] and np.any(c.xm == c.blocks[0, 0, 1])    # on the edges exactly
    # the s = 1 threshold is crossed by the same grid at the two taus
    assert (_steps_of(C["steps"][0], 0)[1] >= 1.0).sum() > (_steps_of(C["steps"][1], 0)[1] >= 1.0).sum()
    # a grid whose first point lies in no block, and blocks that open at p > 0 in every make_case grid
    for name in ("tile_31_32_33", "tiles_64_65_97", "straddle", "keys"):
        for c in C[name]:
            for w in range(c.W):
                blk = np.array([gs.block_of(v, c.blocks[w]) for v in c.xm])
                assert np.any((blk[1:] >= 0) & (blk[1:] != blk[:-1])) and np.any(blk == -1), (name, w)
            assert np.any(np.diff(c.xm) == 0)
    # tiles: the grids end one short of, on and one past a tile, and on 2 tiles, 2 + 1, 3 + 1
    assert [c.n % 32 for c in C["tile_31_32_33"]] == [31, 0, 1]
    assert [(c.n // 32, c.n % 32) for c in C["tiles_64_65_97"]] == [(2, 0), (2, 1), (3, 1)]
    assert all(np.any(np.array([gs.block_of(v, c.blocks[0]) for v in c.xm]) == 2) for c in C["tiles_64_65_97"])
    # waves: V one short of, on and one past a wave; a vector's draws in two waves
    assert [c.W * c.S for c in C["wave_63_64_65"]] == [63, 64, 65]
    c = C["straddle"][0]
    lanes = [(w * c.S // 64, (w * c.S + c.S - 1) // 64) for w in range(c.W)]
    assert lanes == [(0, 0), (0, 1), (1, 2)] and c.W * c.S == 129
    # keys: the unsigned sum first + row passes 2^31
    assert gd.vkey_of(C["keys"][1].first, 1) == 2 ** 31
