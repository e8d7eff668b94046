"""The parallel-tempered sampler without a GPU: the host double's moves
(tests/pt_double.py), sampler.PTSampler driven through it on CPU tensors, the
default ladder, and the mcmc_utils helpers of the usePT = 1 path."""
import numpy as np
import pytest

from lfit_python_amd import mcmc_utils, sampler
from tests import pt_double, stretch_double


def _sampler(T, W, ndim, seed=3, **kw):
    ev = pt_double.GaussianTarget()
    S = sampler.PTSampler(W, ndim, ev, ntemps=T, seed=seed, ops=pt_double.TorchCpuPTOps(), **kw)
    p0 = np.random.default_rng(seed).standard_normal((T, W, ndim))
    return S, p0


@pytest.mark.parametrize("W", [4, 36, 2052])
def test_swap_permutations_are_permutations(W):
    for level in (1, 4):
        A, B, lu = pt_double.swap_draws(W, seed=7, step=5, level=level)
        assert sorted(A) == list(range(W)) and sorted(B) == list(range(W))
        assert np.all(lu < 0.0) and lu.shape == (W,)
    # the two sides, and the pairs, draw different permutations
    A2, B2, _ = pt_double.swap_draws(W, seed=7, step=5, level=2)
    if W > 4:
        assert not np.array_equal(A, B) and not np.array_equal(A, A2) and not np.array_equal(B, B2)


def test_exact_fma_rows_differ_from_two_roundings_by_an_ulp_at_most():
    pos = 1.0 + 0.1 * np.random.default_rng(0).standard_normal((2, 8, 5))
    q0, z0 = pt_double.propose(pos, 0, 2.0, 1, 0)
    q1, z1 = pt_double.propose(pos, 0, 2.0, 1, 0, exact=True)
    assert np.array_equal(z0, z1)
    assert np.max(np.abs(q0 - q1) / np.abs(q1)) < 3e-16


def test_one_level_is_the_stretch_move_and_never_swaps():
    """T = 1: the counters are the stretch move's own, so the level follows
    stretch_double's chain; no swap is proposed."""
    S, p0 = _sampler(1, 8, 3)
    assert np.array_equal(S.betas, [1.0])
    pos, lp, ll = S.run_mcmc(p0, 6)
    assert S.nswap.sum() == 0 and np.array_equal(S.tswap_acceptance_fraction, [0.0])
    assert pos.shape == (1, 8, 3) and lp.shape == (1, 8) and ll.shape == (1, 8)
    x = p0[0].copy()
    f = lambda v: -0.5 * (v * v).sum(1) * (1.0 + 1.0 / 9.0)
    lnp = f(x)
    nacc = np.zeros(8, np.int32)
    for step in range(6):
        for half in (0, 1):
            q, zf = stretch_double.propose(x, half, 2.0, 3, step)
            stretch_double.accept(x, lnp, half, q, zf, f(q), 3, step, nacc)
    np.testing.assert_allclose(pos[0], x, rtol=1e-12)
    assert np.array_equal(S.naccepted[0], nacc)


def test_swaps_exchange_rows_with_their_scalars():
    """After swaps alone every slot still holds a consistent (row, lnl, lnpr)
    triple, each level pair's rows are conserved as a set, and the counters
    add up."""
    T, W, nd = 4, 10, 3
    rng = np.random.default_rng(1)
    pos = rng.standard_normal((T, W, nd))
    lnl, lnpr = -0.5 * (pos ** 2).sum(2), -(pos ** 2).sum(2) / 18.0
    p, l, r = pos.copy(), lnl.copy(), lnpr.copy()
    nswap = np.zeros((T, 2), np.int64)
    betas = sampler.default_betas(nd, T)
    log = pt_double.swap(p, l, r, betas, 9, 0, nswap)
    assert [i for i, *_ in log] == [3, 2, 1]
    assert np.array_equal(nswap[:, 0], [0, W, W, W])
    assert np.array_equal(nswap[1:, 1], [acc.sum() for *_, acc in log][::-1])
    assert 0 < nswap[:, 1].sum() < 3 * W
    np.testing.assert_array_equal(l, -0.5 * (p ** 2).sum(2))
    np.testing.assert_array_equal(r, -(p ** 2).sum(2) / 18.0)
    assert sorted(map(tuple, p.reshape(-1, nd))) == sorted(map(tuple, pos.reshape(-1, nd)))


def test_default_ladder():
    nd = 18
    r = 1.0 + 2.0 * np.sqrt(np.log(4.0)) / np.sqrt(nd)
    b = sampler.default_betas(nd, 5)
    np.testing.assert_allclose(b, r ** -np.arange(5.0), rtol=1e-15)
    assert b[0] == 1.0 and np.all(np.diff(b) < 0)
    # Tmax as in ptemcee: with ntemps it fixes the ratio, alone the count, inf a beta = 0 level
    np.testing.assert_allclose(sampler.default_betas(nd, 4, Tmax=1000.0), 1000.0 ** (-np.arange(4.0) / 3.0))
    n = len(sampler.default_betas(nd, Tmax=50.0))
    assert r ** (n - 1) >= 50.0 > r ** (n - 2)
    hot = sampler.default_betas(nd, 4, Tmax=np.inf)
    assert hot[-1] == 0.0 and np.allclose(hot[:3], r ** -np.arange(3.0))
    with pytest.raises(ValueError):
        sampler.default_betas(nd)
    ev = pt_double.GaussianTarget()
    ops = pt_double.TorchCpuPTOps()
    assert np.array_equal(sampler.PTSampler(8, nd, ev, ntemps=5, ops=ops).betas, b)
    assert np.array_equal(sampler.PTSampler(8, nd, ev, betas=[1.0, 0.3, 0.0], ops=ops).betas, [1.0, 0.3, 0.0])
    for bad in ([0.9, 0.5], [1.0, 1.0], [1.0, 0.5, 0.7], [1.0, -0.1]):
        with pytest.raises(ValueError):
            sampler.PTSampler(8, nd, ev, betas=bad, ops=ops)
    for W in (7, 2):
        with pytest.raises(ValueError):
            sampler.PTSampler(W, nd, ev, ntemps=2, ops=ops)


def test_sampler_surface_and_shapes():
    T, W, nd = 3, 8, 2
    S, p0 = _sampler(T, W, nd)
    seen = []
    for pos, lp, ll in S.sample(p0, iterations=5, storechain=True):
        assert pos.shape == (T, W, nd) and lp.shape == (T, W) and ll.shape == (T, W)
        np.testing.assert_allclose(ll, -0.5 * (pos ** 2).sum(2), rtol=1e-13)
        np.testing.assert_allclose(lp, S.betas[:, None] * ll - (pos ** 2).sum(2) / 18.0, rtol=1e-13)
        seen.append(pos)
    assert S.chain.shape == (T, W, 5, nd) and S.flatchain.shape == (T, W * 5, nd)
    assert S.logprobability.shape == (T, W, 5) and S.loglikelihood.shape == (T, W, 5)
    np.testing.assert_array_equal(S.chain[:, :, 4], seen[4])
    assert S.acceptance_fraction.shape == (T, W) and S.tswap_acceptance_fraction.shape == (T,)
    assert S.random_state == 5
    # run_mcmc continues the same chain as sample(); thin keeps every other step
    S2, _ = _sampler(T, W, nd)
    S2.run_mcmc(p0, 3, store=True)
    S2.run_mcmc(None, 2, storechain=True)
    np.testing.assert_array_equal(S2.chain, S.chain)
    S2.reset()
    assert S2.chain.shape == (T, W, 0, nd) and S2.random_state == 5 and S2.iteration == 0
    assert S2.nswap.sum() == 0 and S2.naccepted.sum() == 0
    S2.run_mcmc(None, 4, thin=2)
    assert S2.chain.shape == (T, W, 2, nd) and S2.random_state == 9
    # the cold-only store
    S3, _ = _sampler(T, W, nd, cold_only=True)
    S3.run_mcmc(p0, 5)
    assert S3.chain.shape == (1, W, 5, nd)
    np.testing.assert_array_equal(S3.chain[0], S.chain[0])
    np.testing.assert_array_equal(S3.logprobability[0], S.logprobability[0])


def test_a_non_finite_start_is_refused():
    S, p0 = _sampler(2, 8, 2)
    p0[1, 3, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        S.run_mcmc(p0, 1)
    with pytest.raises(ValueError, match="shape"):
        S.run_mcmc(p0[:, :4], 1)


def test_non_finite_proposals_are_never_accepted():
    """ln_prob = -inf or NaN rejects, whatever lnlike_e holds."""
    T, W, nd = 2, 8, 2
    rng = np.random.default_rng(0)
    pos = rng.standard_normal((T, W, nd))
    lnl, lnpr = -0.5 * (pos ** 2).sum(2), np.zeros((T, W))
    q, zf = pt_double.propose(pos, 0, 2.0, 1, 0)
    lnp_new = np.full(T * W // 2, 1e6)            # everything else is accepted
    lnp_new[[0, 5]] = -np.inf, np.nan
    lle = np.full((T * W // 2, 1), 1e6)
    nacc = np.zeros((T, W), np.int32)
    acc = pt_double.accept(pos, lnl, lnpr, 0, np.array([1.0, 0.5]), q, zf, lnp_new, lle, 1, 0, nacc)
    assert list(np.flatnonzero(~acc)) == [0, 5] and nacc.sum() == 6
    assert np.all(np.isfinite(lnl)) and np.all(np.isfinite(lnpr))


def test_initialise_walkers_pt_against_a_box_prior():
    p = np.array([1.0, 2.0, -3.0])
    box = lambda x, model=None: np.where(np.all(np.abs(x - p) < 0.15, axis=1), 0.0, -np.inf)  # noqa: E731
    box.batched = True
    p0 = mcmc_utils.initialise_walkers_pt(p, 0.1, 16, 3, box, seed=2)
    assert p0.shape == (3, 16, 3)
    assert np.all(np.isfinite(box(p0.reshape(-1, 3))))
    assert len(np.unique(p0.reshape(-1, 3), axis=0)) == 48
    # the per-vector ln_prior form of the reference
    one = lambda v, model: 0.0 if np.all(np.abs(v - p) < 0.15) else -np.inf  # noqa: E731
    assert np.array_equal(mcmc_utils.initialise_walkers_pt(p, 0.1, 16, 3, one, None, seed=2), p0)


def test_run_ptmcmc_save_writes_the_cold_level(tmp_path):
    T, W, nd = 3, 8, 2
    S, p0 = _sampler(T, W, nd, cold_only=True)
    f = str(tmp_path / "chain_prod.txt")
    out = mcmc_utils.run_ptmcmc_save(S, p0, 5, f, col_names="walker_no a b ln_prob", chunk=2)
    assert out is S
    lines = open(f).read().splitlines()
    assert lines[0] == "walker_no a b ln_prob" and len(lines) == 1 + 5 * W
    assert [int(l.split()[0]) for l in lines[1:1 + W]] == list(range(W))
    c = mcmc_utils.readchain(f)
    assert c.shape == (W, 5, nd + 1)
    np.testing.assert_array_equal(c[:, :, :nd], S.chain[0])          # repr round-trips
    np.testing.assert_allclose(c[:, :, nd], S.logprobability[0], atol=5e-7)   # written with %f
    # the cold log posterior: beta = 1
    x2 = (S.chain[0] ** 2).sum(2)
    np.testing.assert_allclose(S.logprobability[0], -0.5 * x2 - x2 / 18.0, rtol=1e-13)
    # the same chain as the reference's per-step loop over sample()
    S2, _ = _sampler(T, W, nd)
    cold = [pos[0] for pos, lp, ll in S2.sample(p0, iterations=5, store=True)]
    np.testing.assert_array_equal(np.stack(cold, 1), S.chain[0])


def test_shape_limits_without_gpu():
    """Refused shapes come back as LFG_E_ARGS before any launch; the
    workspace holds the permutations, the origin map and the pairs' ln u."""
    import ctypes
    from lfit_python_amd import _native
    L = _native.lib()
    p, p2 = ctypes.c_void_p(8), ctypes.c_void_p(16)
    for W in (7, 2, 8194):
        assert L.lfg_pt_workspace_size(2, W) == 0
        assert L.lfg_pt_propose(p, 2, W, 3, 0, 2.0, 1, 0, p, p, None) == -1
        assert L.lfg_pt_accept(p, p, p, 2, W, 3, 0, p, p, p, p, p, 1, 1, 0, None, None) == -1
        assert L.lfg_pt_swap(p, p2, p, p, 2, W, 3, p, 1, 0, p, p, 1 << 30, None) == -1
    assert L.lfg_pt_swap(p, p2, p, p, 2, 8, 3, p, 1, 0, p, p, 16, None) == -2
    assert L.lfg_pt_workspace_size(1, 4) >= 4 * 4
    assert L.lfg_pt_workspace_size(3, 36) >= (2 * 2 * 36 + 3 * 36) * 4 + 2 * 36 * 8


def test_world_above_one_is_refused(monkeypatch):
    import torch
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="one rank"):
        sampler.PTSampler(8, 2, pt_double.GaussianTarget(), ntemps=2, ops=pt_double.TorchCpuPTOps())


@pytest.mark.slow
def test_tempered_variances_of_a_gaussian_target():
    """lnlike = -|x|^2 / 2, lnprior = -|x|^2 / 18: level t samples a Gaussian
    of variance 1 / (beta_t + 1/9) per coordinate.  T = 4, W = 64, ndim = 4,
    3000 iterations, the first 500 dropped; the mean of x^2 per level within
    3 % (six seeds of this double stayed within 0.63 %; a z exponent of ndim
    or a swap criterion of the wrong sign shift levels by 18 % and more)."""
    T, W, nd = 4, 64, 4
    S, p0 = _sampler(T, W, nd, seed=1)
    S.run_mcmc(p0, 500, storechain=False)
    S.reset()
    S.run_mcmc(None, 2500)
    x2 = (S.chain ** 2).mean(axis=(1, 2, 3))
    want = 1.0 / (S.betas + 1.0 / 9.0)
    print("mean x^2 / expected - 1 per level:", x2 / want - 1.0)
    assert np.all(np.abs(x2 / want - 1.0) < 0.03)
    assert np.all((S.acceptance_fraction > 0.3) & (S.acceptance_fraction < 0.9))
    assert np.all((S.tswap_acceptance_fraction > 0.2) & (S.tswap_acceptance_fraction < 0.95))
