"""CPU: the stretch move's host double (tests/stretch_double.py) anchored
outside itself, so that the GPU comparison against it (test_gpu_sampler_double)
cannot pass on a mistake the double shares with the kernels' header comment:
Philox4x32-10 against the published known answers, the counter layout against
counters written out by hand, u53's ends, the exact fma against a case two
roundings get wrong, the two readings of (a - 1) u + 1, and the restated
moves (accept_regen, verdict, apply_verdicts, chain) against propose +
accept.  Every MUTATIONS entry of the double must fail the bit comparison the
GPU tests make."""
import numpy as np
import pytest

from tests import pt_double
from tests import stretch_double as sd

U32 = 0xFFFFFFFF


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


# Random123's kat_vectors, philox4x32 10: counter, key -> output.  The vector
# file is not shipped with this repository's toolchain; the first and the
# third line are the anchor (known independently of this project: the zero
# vector and the digits-of-pi vector).  The second is what the double gives
# and what the file is remembered to hold; it is kept as a record.
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((U32,) * 4, (U32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones_recorded", "pi"])
def test_philox_known_answers(ctr, key, want):
    assert _hex(sd.philox(*ctr, *key)) == want
    # vectorised over the first counter word as draw() uses it
    got = sd.philox(np.array([ctr[0], ctr[0]], np.uint64), ctr[1], ctr[2], ctr[3], *key)
    assert _hex(g[1] for g in got) == want


@pytest.mark.parametrize("step", [2**32 - 1, 2**32, 2**64 - 1, 5])
@pytest.mark.parametrize("seed", [7, 2**32, 2**40 + 7, 2**63 + 1])
def test_draw_counter_layout(seed, step):
    """counter = (walker, step lo, step hi, half * 2 + purpose), key = (seed
    lo, seed hi), written out by hand"""
    for half in (0, 1):
        for purpose in (0, 1):
            got = sd.draw(seed, step, half, purpose, 3)
            for i in range(3):
                want = sd.philox(i, step % 2**32, step // 2**32, (0, 1, 2, 3)[2 * half + purpose],
                                 seed % 2**32, seed // 2**32)
                assert [int(g[i]) for g in got] == [int(w) for w in want]
            lo = sd.draw(seed, step, half, purpose, 2, lo=1)
            assert [int(g[0]) for g in lo] == [int(g[1]) for g in got]
    # the four (half, purpose) streams and the two step words are distinct draws
    rows = {tuple(int(g[0]) for g in sd.draw(seed, step, h, p, 1)) for h in (0, 1) for p in (0, 1)}
    assert len(rows) == 4
    assert [int(g[0]) for g in sd.draw(seed, 2**32, 0, 0, 1)] != [int(g[0]) for g in sd.draw(seed, 0, 0, 0, 1)]
    assert [int(g[0]) for g in sd.draw(2**32, step, 0, 0, 1)] != [int(g[0]) for g in sd.draw(0, step, 0, 0, 1)]


def test_u53_ends():
    assert sd.u53(0, 0) == 0.0
    top = float(sd.u53(U32, U32))
    assert top == 1.0 - 2.0 ** -53 and top < 1.0
    assert float(sd.u53(31, 63)) == 0.0                 # the dropped low bits
    assert float(sd.u53(32, 0)) == 2.0 ** -27 and float(sd.u53(0, 64)) == 2.0 ** -53
    r = sd.draw(3, 9, 1, 1, 4096)
    u = sd.u53(r[0], r[1])
    assert u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55


def test_exact_fma_is_one_rounding():
    # (1 + e)(1 - e) - 1 = -e^2 exactly; the rounded product is 1
    e = 2.0 ** -30
    assert sd._fma1(1.0 + e, 1.0 - e, -1.0) == -e * e
    assert (1.0 + e) * (1.0 - e) + -1.0 == 0.0
    # a stretch row c + (s - c) z where the two roundings miss the fma
    rng = np.random.default_rng(1)
    s, c, z = rng.standard_normal(4000), rng.standard_normal(4000), rng.uniform(0.5, 2.0, 4000)
    one, two = sd.fma(s - c, z, c), c + (s - c) * z
    k = np.flatnonzero(one != two)
    assert 0 < k.size < 4000
    assert np.max(np.abs(one - two)) < 2.0 ** -49   # an ulp of the product: |s - c| z < 16
    from fractions import Fraction
    for i in k[:20]:
        exact = Fraction(float(s[i] - c[i])) * Fraction(float(z[i])) + Fraction(float(c[i]))
        assert abs(Fraction(float(one[i])) - exact) < abs(Fraction(float(two[i])) - exact)
    # non-finite operands fall through to IEEE arithmetic
    assert sd._fma1(np.inf, 1.0, 1.0) == np.inf and np.isnan(sd._fma1(np.nan, 1.0, 1.0))
    assert pt_double._fma is sd._fma


def test_z_readings_differ_off_powers_of_two():
    """(a - 1) u is exact when a - 1 is a power of two, so a = 2 and a = 1.5
    cannot tell fma(a - 1, u, 1) from a product and a sum; a = 2.5 and
    a = 1.3 can, which is why the GPU cases run there"""
    r = sd.draw(12345, 0, 0, 0, 2048)
    u = sd.u53(r[0], r[1])
    for a in (2.0, 1.5):
        np.testing.assert_array_equal(sd.z_of(u, a, True), sd.z_of(u, a, False))
    for a in (2.5, 1.3):
        z1, z0 = sd.z_of(u, a, True), sd.z_of(u, a, False)
        frac = np.mean(z1 != z0)
        assert 0.01 < frac < 0.5, frac               # a few per cent of the draws
        assert np.max(np.abs(z1 - z0) / z1) < 2.0 ** -49   # an ulp of zr, squared, two more roundings
    # z in [1 / a, a]: the top draw rounds up to a itself
    assert sd.z_of(0.0, 2.5, True) == 1.0 / 2.5 and sd.z_of(1.0 - 2.0 ** -53, 2.5, True) == 2.5


class Gauss:
    """ln_prob = -|x|^2 / 2 with planted values at chosen call rows"""

    def __init__(self, plant=None):
        self.plant = plant or {}
        self.calls = 0

    def __call__(self, q):
        out = -0.5 * np.sum(q * q, axis=1)
        for (call, row), v in self.plant.items():
            if call == self.calls:
                out[row] = v
        self.calls += 1
        return out


PLANTS = [("none", {}), ("-inf", {3: -np.inf}), ("nan", {2: np.nan}), ("+inf", {1: np.inf}),
          ("all", {0: np.nan, 1: np.inf, 2: -np.inf})]


@pytest.mark.parametrize("a", [2.0, 2.5, 1.3])
@pytest.mark.parametrize("name,plant", PLANTS, ids=[p[0] for p in PLANTS])
def test_restated_moves_agree_with_propose_accept(a, name, plant):
    """accept_regen, verdict + apply_verdicts (one shard, and shards with
    lo != 0) against propose(exact) + accept: same rows, ln_prob, counters
    and flags, with -inf / NaN / +inf new values and -inf old values"""
    rng = np.random.default_rng(5)
    W, nd, seed, step = 14, 3, 2**40 + 7, 2**32 - 1
    ns = W // 2
    pos0 = rng.standard_normal((W, nd))
    lnp0 = -0.5 * np.sum(pos0 * pos0, axis=1)
    lnp0[[4, 5, ns + 4, ns + 5]] = -np.inf          # walkers that start outside the prior
    for half in (0, 1):
        q, zf = sd.propose(pos0, half, a, seed, step, exact=True)
        new = -0.5 * np.sum(q * q, axis=1) + rng.standard_normal(ns)
        for k, v in plant.items():
            new[k] = v
        new[5] = -np.inf                             # -inf old and new: NaN difference, rejected
        ref = pos0.copy(), lnp0.copy(), np.zeros(W, np.int64)
        acc = sd.accept(*ref[:2], half, q, zf, new, seed, step, ref[2])
        assert acc[4] and not acc[5]                 # -inf old accepts its finite proposal
        for k, v in plant.items():
            assert acc[k] == (v == np.inf)
        got = pos0.copy(), lnp0.copy(), np.zeros(W, np.int64)
        flag = np.zeros(ns, bool)
        sd.accept_regen(*got[:2], half, a, new, seed, step, got[2], flag)
        for g, r in zip(got, ref):
            np.testing.assert_array_equal(g, r)
        np.testing.assert_array_equal(flag, acc)
        for cuts in ((0, ns), (0, 1, 3, ns)):
            v = np.concatenate([sd.verdict(new[lo:hi], lnp0, zf[lo:hi], lo, ns, half, seed, step)
                                for lo, hi in zip(cuts[:-1], cuts[1:])])
            np.testing.assert_array_equal(~np.isnan(v), acc & ~np.isnan(new))
            np.testing.assert_array_equal(v[~np.isnan(v)], new[~np.isnan(v)])
            got = pos0.copy(), lnp0.copy(), np.zeros(W, np.int64)
            flag = np.zeros(ns, bool)
            sd.apply_verdicts(*got[:2], half, a, v, seed, step, got[2], flag)
            # (a NaN new value accepted through a -inf old one could not be told
            # from a rejection; +inf - -inf is the only such difference and is finite)
            for g, r in zip(got, ref):
                np.testing.assert_array_equal(g, r)


def test_chain_is_the_red_blue_loop():
    rng = np.random.default_rng(9)
    W, nd, a, seed, step0 = 10, 2, 2.5, 2**63 + 1, 2**32 - 2
    pos0 = rng.standard_normal((W, nd))
    lnp0 = -0.5 * np.sum(pos0 * pos0, axis=1)
    lnp0[2] = -np.inf
    fn = Gauss({(3, 1): np.nan, (4, 0): -np.inf})
    c = sd.chain(pos0, lnp0, fn, a, seed, step0, 4)
    assert fn.calls == 8
    pos, lnp, nacc = pos0.copy(), lnp0.copy(), np.zeros(W, np.int64)
    fn2 = Gauss(fn.plant)
    for it in range(4):
        for half in (0, 1):
            q, zf = sd.propose(pos, half, a, seed, step0 + it, exact=True)
            acc = sd.accept(pos, lnp, half, q, zf, fn2(q), seed, step0 + it, nacc)
            np.testing.assert_array_equal(c.acc[it, half], acc)
        np.testing.assert_array_equal(c.pos[it], pos)
        np.testing.assert_array_equal(c.lnp[it], lnp)
        np.testing.assert_array_equal(c.naccept[it], nacc)
    assert c.pos.shape == (4, W, nd) and c.lnp.shape == (4, W) and c.acc.shape == (4, 2, W // 2)
    assert 0.0 < c.margin < np.inf
    # the -inf start, the NaN and the -inf proposal have operands, not margins
    assert len(c.nonfinite) >= 3
    assert any(old == -np.inf and np.isfinite(new) and took for _, _, new, old, took in c.nonfinite)
    assert any(np.isnan(new) and not took for _, _, new, old, took in c.nonfinite)
    assert c.naccept[0][2] == 1                       # the walker outside the prior moved at once
    assert c.acc.any() and not c.acc.all()


@pytest.mark.parametrize("mutate", sd.MUTATIONS)
def test_every_mutation_fails_the_bit_comparison(mutate):
    """each mutated double misses the double bit for bit at W = 10, a = 2.5,
    a seed and a step past 2^32, in the rows (and the acceptance draws for the
    counter mutations).  The two readings of z part on about 4 % of the draws:
    MUTATION_CASE's step is the first from 2^33 + 5 at which one of the five
    draws of each half does."""
    rng = np.random.default_rng(2)
    W, nd = 10, 7
    a, seed, step = sd.MUTATION_CASE
    pos = rng.standard_normal((W, nd))
    q = np.stack([sd.propose(pos, h, a, seed, step, exact=True)[0] for h in (0, 1)])
    qm = np.stack([sd.propose(pos, h, a, seed, step, exact=True, mutate=mutate)[0] for h in (0, 1)])
    assert np.any(q != qm)
    if mutate == "z_uncontracted":
        assert np.max(np.abs(q - qm)) < 1e-14         # one ulp of z: only a bit comparison sees it
    if mutate in ("step_hi_dropped", "half_purpose_swapped"):
        lu = np.stack([sd._lnu(seed, step, h, W // 2) for h in (0, 1)])
        lum = np.stack([sd._lnu(seed, step, h, W // 2, mutate) for h in (0, 1)])
        assert np.any(lu != lum)
    # at a = 2 and a step below 2^32 two of the four are invisible
    if mutate in ("z_uncontracted", "step_hi_dropped"):
        q2 = sd.propose(pos, 0, 2.0, seed, 5, exact=True)[0]
        np.testing.assert_array_equal(q2, sd.propose(pos, 0, 2.0, seed, 5, exact=True, mutate=mutate)[0])
