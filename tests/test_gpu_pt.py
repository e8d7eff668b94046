"""GPU: the parallel-tempered sampler.  The lfg_pt_* kernels draw for draw
against the host double (tests/pt_double.py), their shape limits, the
identity ln_prob = ln_prior + sum_e lnlike_e the tempered step relies on,
the tempered variances of a Gaussian target on the device, the usePT = 1
driver, and eager repeatability."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from tests import pt_double

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


class ToyTree:
    """A two-'eclipse' torch evaluator whose every operation is one IEEE
    multiply, add or compare per element, summed in a fixed order: the same
    bits on the device and on the host.  ln_prob is -inf where x0 > 1.5 and
    NaN where x1 < 0.5, with lnlike_e left finite there."""
    E = 2

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self.seen = {"-inf": 0, "nan": 0}

    def __call__(self, x, out=None, lnlike_e=None):
        import torch
        s = x[:, 0] * x[:, 0]
        for d in range(1, x.shape[1]):
            s = s + x[:, d] * x[:, d]
        l0 = s * -0.5
        l1 = (x[:, 0] * x[:, 1]) * 0.25
        lpr = (x[:, -1] * x[:, -1]) * -0.0625
        lnp = lpr + (l0 + l1)
        lnp = torch.where(x[:, 0] > 1.5, torch.full_like(lnp, float("-inf")), lnp)
        lnp = torch.where(x[:, 1] < 0.5, torch.full_like(lnp, float("nan")), lnp)
        self.seen["-inf"] += int(torch.isneginf(lnp).sum())
        self.seen["nan"] += int(torch.isnan(lnp).sum())
        if lnlike_e is not None:
            lnlike_e[:, 0].copy_(l0)
            lnlike_e[:, 1].copy_(l1)
        if out is None:
            return lnp
        out.copy_(lnp)
        return out


def _start(T, W, ndim, seed):
    rng = np.random.default_rng(seed)
    p0 = 1.0 + 0.25 * rng.standard_normal((T, W, ndim))
    p0[..., 0] = rng.uniform(0.7, 1.45, (T, W))   # a finite start: x0 <= 1.5, x1 >= 0.5
    p0[..., 1] = rng.uniform(0.55, 1.3, (T, W))
    return p0


def _draw_for_draw(T, W, ndim, a, seed):
    """Three full iterations, every stage compared: proposals to 1e-14
    relative; permutations, acceptances, swap decisions, counters and the
    state pos / lnl / lnpr exactly.  Among the proposals are ln_prob = -inf
    and NaN ones (none may move its walker)."""
    import torch
    from lfit_python_amd import sampler
    ns = W // 2
    dev = torch.device("cuda")
    betas = sampler.default_betas(ndim, T)
    ops, ev_d, ev_h = sampler.HipPTOps(dev), ToyTree(dev), ToyTree("cpu")
    f64 = dict(dtype=torch.float64, device=dev)
    # host state (numpy) and device state
    pos = _start(T, W, ndim, seed)
    lnp = torch.empty(T * W, dtype=torch.float64)
    lle = torch.empty((T * W, 2), dtype=torch.float64)
    ev_h(torch.as_tensor(pos.reshape(T * W, ndim)), out=lnp, lnlike_e=lle)
    assert bool(torch.isfinite(lnp).all())
    lnl = (lle[:, 0] + lle[:, 1]).numpy().reshape(T, W).copy()
    lnpr = lnp.numpy().reshape(T, W) - lnl
    nacc, nswap = np.zeros((T, W), np.int32), np.zeros((T, 2), np.int64)
    d_pos, d_alt = torch.as_tensor(pos, device=dev), torch.empty((T, W, ndim), **f64)
    d_lnl, d_lnpr = torch.as_tensor(lnl, device=dev), torch.as_tensor(lnpr, device=dev)
    d_betas = torch.as_tensor(betas, device=dev)
    d_q, d_zf = torch.empty((T * ns, ndim), **f64), torch.empty(T * ns, **f64)
    d_lnp, d_lle = torch.empty(T * ns, **f64), torch.empty((T * ns, 2), **f64)
    d_nacc = torch.zeros((T, W), dtype=torch.int32, device=dev)
    d_nswap = torch.zeros((T, 2), dtype=torch.int64, device=dev)
    h_lnp, h_lle = torch.empty(T * ns, dtype=torch.float64), torch.empty((T * ns, 2), dtype=torch.float64)
    t_of = np.repeat(np.arange(T), ns)
    moved = 0
    for step in range(3):
        for half in (0, 1):
            ops.propose(d_pos, half, a, seed, step, d_q, d_zf)
            q, zf = pt_double.propose(pos, half, a, seed, step, exact=True)
            np.testing.assert_allclose(d_q.cpu().numpy(), q, rtol=1e-14, atol=0)
            np.testing.assert_allclose(d_zf.cpu().numpy(), zf, rtol=1e-14, atol=0)
            ev_d(d_q, out=d_lnp, lnlike_e=d_lle)
            ev_h(torch.as_tensor(q), out=h_lnp, lnlike_e=h_lle)
            before = d_pos.cpu().numpy()
            ops.accept(d_pos, d_lnl, d_lnpr, half, d_betas, d_q, d_zf, d_lnp, d_lle, seed, step, d_nacc)
            acc = pt_double.accept(pos, lnl, lnpr, half, betas, q, zf, h_lnp.numpy(), h_lle.numpy(), seed, step,
                                   nacc)
            after = d_pos.cpu().numpy()
            bad = ~np.isfinite(d_lnp.cpu().numpy())
            w_of = half * ns + np.tile(np.arange(ns), T)
            assert np.array_equal(after[t_of[bad], w_of[bad]], before[t_of[bad], w_of[bad]])
            assert not acc[bad].any()
            moved += int(acc.sum())
            np.testing.assert_array_equal(d_nacc.cpu().numpy(), nacc)
            np.testing.assert_array_equal(after, pos)
            np.testing.assert_array_equal(d_lnl.cpu().numpy(), lnl)
            np.testing.assert_array_equal(d_lnpr.cpu().numpy(), lnpr)
        ops.swap(d_pos, d_alt, d_lnl, d_lnpr, d_betas, seed, step, d_nswap)
        d_pos, d_alt = d_alt, d_pos
        log = pt_double.swap(pos, lnl, lnpr, betas, seed, step, nswap)
        perm = ops.workspace(T, W).cpu().numpy()[:(T - 1) * 2 * W].reshape(T - 1, 2, W)
        for i, A, B, _ in log:
            np.testing.assert_array_equal(perm[i - 1, 0], A)
            np.testing.assert_array_equal(perm[i - 1, 1], B)
        np.testing.assert_array_equal(d_nswap.cpu().numpy(), nswap)
        np.testing.assert_array_equal(d_pos.cpu().numpy(), pos)
        np.testing.assert_array_equal(d_lnl.cpu().numpy(), lnl)
        np.testing.assert_array_equal(d_lnpr.cpu().numpy(), lnpr)
    assert ev_d.seen == ev_h.seen
    if T * W >= 72:   # the case is exercised (the 4-walker shape draws too few proposals to be sure)
        assert ev_d.seen["-inf"] > 0 and ev_d.seen["nan"] > 0
    assert 0 < moved < 6 * T * ns
    if T > 1:
        assert np.all(nswap[1:, 0] == 3 * W) and np.all((0 < nswap[1:, 1]) & (nswap[1:, 1] < 3 * W))


@pytest.mark.parametrize("T,W,ndim", [(1, 4, 3), (2, 36, 87), (5, 64, 18), (3, 2052, 5)])
def test_kernels_match_the_double_draw_for_draw(T, W, ndim):
    _draw_for_draw(T, W, ndim, 2.0, 1234 + W)


@pytest.mark.parametrize("T,W,ndim", [(1, 4, 3), (2, 36, 87)])
def test_kernels_match_the_double_off_a2(T, W, ndim):
    """the same comparison at a = 2.5 and a seed past 2^32: (a - 1) u is no
    longer exact, so k_pt_propose's z must be the double's fma(a - 1, u, 1)
    reading (stretch_double.z_of) for the accepted rows to equal the host's"""
    _draw_for_draw(T, W, ndim, 2.5, 2**40 + 7 + W)


def test_swap_at_the_largest_ensemble():
    """W = LFG_PT_MAX_W (the whole LDS sort buffer, a power of two: no
    padding): permutations and the state after the swaps, exactly."""
    import torch
    from lfit_python_amd import sampler
    T, W, ndim, seed, step = 2, 8192, 2, 5, 1 << 33
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    pos = rng.standard_normal((T, W, ndim))
    lnl, lnpr = -3.0 * rng.random((T, W)), rng.standard_normal((T, W))
    betas = np.array([1.0, 0.4])
    ops = sampler.HipPTOps(dev)
    d = [torch.as_tensor(x, device=dev) for x in (pos, lnl, lnpr, betas)]
    out = torch.empty_like(d[0])
    d_nswap = torch.zeros((T, 2), dtype=torch.int64, device=dev)
    ops.swap(d[0], out, d[1], d[2], d[3], seed, step, d_nswap)
    nswap = np.zeros((T, 2), np.int64)
    (_, A, B, acc), = pt_double.swap(pos, lnl, lnpr, betas, seed, step, nswap)
    perm = ops.workspace(T, W).cpu().numpy()[:2 * W].reshape(2, W)
    np.testing.assert_array_equal(perm[0], A)
    np.testing.assert_array_equal(perm[1], B)
    assert 0 < acc.sum() < W
    np.testing.assert_array_equal(d_nswap.cpu().numpy(), nswap)
    np.testing.assert_array_equal(out.cpu().numpy(), pos)
    np.testing.assert_array_equal(d[1].cpu().numpy(), lnl)
    np.testing.assert_array_equal(d[2].cpu().numpy(), lnpr)


def test_shape_limits_are_refused():
    """W odd, W < 4 and W over LFG_PT_MAX_W return LFG_E_ARGS from every
    entry point, before any launch; the workspace size of such a shape is 0."""
    import torch
    from lfit_python_amd import _native
    L = _native.lib()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p, st = ctypes.c_void_p(buf.data_ptr()), _native.stream_ptr(buf.device)
    p2 = ctypes.c_void_p(buf.data_ptr() + (1 << 15))
    for W in (7, 2, 8194, 0, -4):
        assert L.lfg_pt_workspace_size(2, W) == 0
        assert L.lfg_pt_propose(p, 2, W, 3, 0, 2.0, 1, 0, p, p, st) == -1
        assert L.lfg_pt_accept(p, p, p, 2, W, 3, 0, p, p, p, p, p, 1, 1, 0, None, st) == -1
        assert L.lfg_pt_swap(p, p2, p, p, 2, W, 3, p, 1, 0, p, p, 1 << 19, st) == -1
    assert L.lfg_pt_workspace_size(0, 8) == 0 and L.lfg_pt_workspace_size(1 << 20, 4096) == 0
    assert L.lfg_pt_propose(p, 2, 8, 0, 0, 2.0, 1, 0, p, p, st) == -1        # ndim
    assert L.lfg_pt_propose(p, 2, 8, 3, 2, 2.0, 1, 0, p, p, st) == -1        # half
    assert L.lfg_pt_swap(p, p, p, p, 2, 8, 3, p, 1, 0, p, p, 1 << 19, st) == -1   # in place
    assert L.lfg_pt_swap(p, p2, p, p, 2, 8, 3, p, 1, 0, p, p, 16, st) == -2   # workspace
    assert L.lfg_pt_workspace_size(2, 8192) >= (2 * 8192 + 2 * 8192) * 4
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0   # nothing ran


@pytest.mark.parametrize("tag", ["simple", "tree", "gp"])
def test_lnprob_is_prior_plus_the_eclipse_likelihoods(tag, tmp_path):
    """ln_prob == ln_prior + sum_e lnlike_e to 1e-12 relative wherever ln_prob
    is finite: what lets the tempered step split one lfg_lnprob call into
    ln_like and ln_prior.  A one-eclipse chi^2 tree (k_pair's own combine),
    the six-eclipse chi^2 tree and the GP tree (k_gp_like's combine)."""
    import torch
    from lfit_python_amd import batch, cvmodel
    from tests.helpers import golden_tree
    if tag == "gp":
        d = np.load(os.path.join(GOLD, "lnprob_gp.npz"))
        m = cvmodel.construct_model(os.path.join(GOLD, "ref_test_data", "mcmc_input.dat"))
    else:
        d, m = golden_tree(tag, tmp_path)
    t = batch.compile_tree(m)
    assert t.gp == (tag == "gp") and (t.E == 1) == (tag == "simple")
    ev = batch.LnProbEvaluator(t)
    x = torch.as_tensor(d["walkers"], device="cuda")
    lle = torch.empty((len(x), t.E), dtype=torch.float64, device="cuda")
    lnp = ev(x, lnlike_e=lle).cpu().numpy()
    lpr = ev.ln_prior(x).cpu().numpy()
    lle = lle.cpu().numpy()
    fin = np.isfinite(lnp)
    assert fin.sum() >= 8
    ll = np.zeros(len(lnp))
    for e in range(t.E):
        ll = ll + lle[:, e]
    err = np.abs(lnp[fin] - (lpr[fin] + ll[fin])) / np.abs(lnp[fin])
    print("max relative error of the identity:", err.max())
    assert err.max() <= 1e-12


def test_tempered_variances_on_the_device():
    """The HIP kernels with a torch evaluator on the device: lnlike =
    -|x|^2 / 2, lnprior = -|x|^2 / (2 * 3^2), T = 4, W = 64, ndim = 4, the
    default ladder, 3000 iterations, the first 500 dropped.  The mean of x^2
    per level equals 1 / (beta + 1/9) within 3 %: five times the 0.63 % that
    the NumPy statement of the algorithm stays within over six seeds (with
    this test's seed, 1, it gives 0.36 %), and far below what an error would
    cause (a z exponent of ndim instead of ndim - 1: 18-25 % on every level;
    a swap criterion of the wrong sign: 40 % and more)."""
    import torch
    from lfit_python_amd import sampler
    T, W, nd = 4, 64, 4
    S = sampler.PTSampler(W, nd, pt_double.GaussianTarget("cuda"), ntemps=T, seed=1)
    assert isinstance(S.ops, sampler.HipPTOps)
    p0 = np.random.default_rng(1).standard_normal((T, W, nd))
    S.run_mcmc(p0, 500, storechain=False)
    S.reset()
    S.run_mcmc(None, 2500)
    x2 = (S.chain ** 2).mean(axis=(1, 2, 3))
    want = 1.0 / (S.betas + 1.0 / 9.0)
    print("mean x^2 / expected - 1 per level:", x2 / want - 1.0)
    assert np.all(np.abs(x2 / want - 1.0) < 0.03)
    assert np.all(S.nswap[1:, 0] == 2500 * W)


def _small_pt_input(tmp_path, **over):
    """test_mcmcfit._small_input's input (one chi^2 eclipse, simple bright
    spot, 32 walkers) with usePT = 1 over three levels."""
    src = os.path.join(GOLD, "ref_test_data")
    text = open(os.path.join(src, "mcmc_input.dat"), encoding="utf-8", errors="replace").read().splitlines()
    keys = dict(useGP="0", complex="0", nwalkers="32", nburn="3", nprod="5", double_burnin="1", comp_scat="1",
                usePT="1", ntemps="3")
    keys.update(over)
    out = []
    for line in text:
        k = line.split("=", 1)[0].strip() if "=" in line else None
        out.append("%s = %s" % (k, keys.pop(k)) if k in keys else line)
    out.append("neclipses = 1")
    out += ["%s = %s" % kv for kv in keys.items()]
    tmp_path.mkdir(parents=True, exist_ok=True)
    (tmp_path / "mcmc_input.dat").write_text("\n".join(out) + "\n")
    shutil.copytree(os.path.join(src, "lightcurves"), tmp_path / "lightcurves")
    return str(tmp_path / "mcmc_input.dat")


def test_driver_runs_a_tempered_fit(tmp_path, oracle):
    from lfit_python_amd import batch, cvmodel, mcmcfit, sampler
    from tests.test_gpu_lnprob import LNP_RTOL, _same
    path = _small_pt_input(tmp_path)
    assert mcmcfit.read_run_config(path)["usePT"] is True
    chain = str(tmp_path / "chain_prod.txt")
    out = mcmcfit.run(path, chain_file=chain, seed=5, chunk=2, log=lambda *a: None)
    assert out["status"] == "ok" and out["npars"] == 14 and out["nwalkers"] == 32 and out["ntemps"] == 3
    lines = open(chain).read().splitlines()
    m = cvmodel.construct_model(path)
    assert lines[0] == "walker_no " + " ".join(m.dynasty_par_names) + " ln_prob"
    assert len(lines) == 1 + 5 * 32
    c = sampler.read_chain(chain)
    assert c.shape == (32, 5, 15) and np.all(np.isfinite(c))
    rows = c.reshape(-1, 15)
    ref, _, _ = oracle.lnprob_batch(np.ascontiguousarray(rows[:, :14]), batch.compile_tree(m))
    _same(rows[:, 14], ref, LNP_RTOL)
    acc, tswap = np.array(out["acceptance_levels"]), np.array(out["tswap_acceptance"])
    assert acc.shape == (3,) and tswap.shape == (3,)
    assert np.all((0.0 < acc) & (acc < 1.0)) and np.all((0.0 < tswap) & (tswap < 1.0))
    assert 0.0 < out["acceptance"] < 1.0


def test_same_seed_same_chain(tmp_path):
    """Two eager runs with one seed: bit-identical chains at every level."""
    import torch
    from lfit_python_amd import batch, mcmc_utils, sampler
    from tests.helpers import golden_tree
    _, m = golden_tree("simple", tmp_path)
    t = batch.compile_tree(m)
    ev = batch.LnProbEvaluator(t)
    p = np.array(m.dynasty_par_vals)
    p0 = mcmc_utils.initialise_walkers_pt(p, 1e-3, 32, 3, mcmc_utils.batched_ln_prior(ev), seed=4)
    runs = []
    for _ in range(2):
        S = sampler.PTSampler(32, t.ndim, batch.LnProbEvaluator(t), ntemps=3, seed=9)
        S.run_mcmc(p0, 4)
        runs.append((S.chain, S.logprobability, S.loglikelihood, S.naccepted, S.nswap))
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x, y)
    assert runs[0][3].sum() > 0 and np.all(np.isfinite(runs[0][0]))
    other = sampler.PTSampler(32, t.ndim, ev, ntemps=3, seed=10)
    other.run_mcmc(p0, 4)
    assert not np.array_equal(other.chain, runs[0][0])
