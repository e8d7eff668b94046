"""GPU: every statement of the stretch move against the exact host double
(tests/stretch_double.py), off a = 2.

The draw z = ((a - 1) u + 1)^2 / a, the partner __umulhi(r.z, ns) and the row
fma(s - c, z, c) are written out in k_propose, k_accept_regen,
k_apply_verdicts, make_prop (with the partner's candidate and the FOLD
variant), stretch_draw, k_pair's fold_rows, k_pt_propose and k_wd_step_half;
include/lfg.h promises that they agree bit for bit.  At a = 2 the product
(a - 1) u is exact, so a site that formed (a - 1) u + 1 with two roundings
where the others use one fma could not show; a = 2.5 and a = 1.3 tell them
apart (test_stretch_double.py).

Part 1, the kernels one by one: rows bit-identical to the double, z itself
read back through rows that are z (s = 1, c = 0), partners through rows that
name their index, verdicts and counters with planted -inf / NaN / +inf
ln_prob and -inf old ln_prob, at ensemble sizes around the wave and the
REGEN_WAVES block, ndim around the 64-lane row loop, seeds and steps past
2^32.

Part 2, every half-step mode of EnsembleSampler and hand-driven rank
workspaces against stretch_double.chain, whose ln_prob is a second
LnProbEvaluator (lfg_lnprob, no sampler state) called on the double's own
proposals: positions, ln_prob and acceptance counters bit-identical."""
import ctypes

import numpy as np
import pytest

from tests import stretch_double as sd
from tests.test_gpu_lnprob import _flux_fn

pytestmark = pytest.mark.gpu

SEEDS = ((12345, 0), (2**40 + 7, 2**32 - 1), (2**63 + 1, 2**33 + 5))
NDIMS = (1, 2, 18, 64, 65, 130)
WS = (4, 6, 10, 126, 130)
AS = (2.0, 2.5, 1.3)
GUARD = 64
SENTINEL = 777.0


def _f64(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")


def _guarded(x):
    """x on the device inside a buffer with GUARD sentinel doubles on each side"""
    import torch
    buf = torch.full((x.size + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    view = buf[GUARD:GUARD + x.size].view(x.shape)
    view.copy_(_f64(x))
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _apply_verdicts(pos, lnp, half, a, seed, step, v, nacc):
    import torch
    from lfit_python_amd import _native
    W, nd = pos.shape
    rc = _native.lib().lfg_stretch_apply_verdicts(_vp(pos), _vp(lnp), W, nd, half, a, seed, step, _vp(v), _vp(nacc),
                                                  _native.stream_ptr(torch.device("cuda")))
    assert rc == 0


def _plant(rng, lnp_old, ns, k):
    """new ln_prob of a half: about half accepted, -inf / NaN / +inf planted
    in turn at the first walkers (k rotates them, so that W = 4 meets each)"""
    new = lnp_old + rng.standard_normal(ns)
    vals = (-np.inf, np.nan, np.inf)
    for i in range(min(ns, 3)):
        new[i] = vals[(i + k) % 3]
    return new


# ------------------------------------------------------------ part 1: the kernels
@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("W", WS)
def test_kernels_match_the_exact_double(W, a):
    """lfg_stretch_propose / _propose_dev rows bit-identical to the double and
    zfac to 1e-15 (log is not correctly rounded); lfg_stretch_accept /
    _accept_dev / _accept_regen / _apply_verdicts leave exactly the host's
    ensemble, ln_prob and counters, with planted -inf / NaN / +inf proposals
    and a walker whose old ln_prob is -inf; nothing outside the ensemble is
    written (ndim = 65, 130: the row loop's second and third round)."""
    import torch
    from lfit_python_amd.sampler import HipStretchOps
    ops = HipStretchOps(torch.device("cuda"))
    ns = W // 2
    rng = np.random.default_rng(1000 + W)
    kinds = set()
    for nd in NDIMS:
        pos = rng.standard_normal((W, nd))
        lnp = rng.standard_normal(W)
        for k, (seed, step) in enumerate(SEEDS):
            for half in (0, 1):
                sl = slice(half * ns, (half + 1) * ns)
                lnp0 = lnp.copy()
                lnp0[half * ns + ns - 1] = -np.inf
                qh, zh = sd.propose(pos, half, a, seed, step, exact=True)
                P, stepd = _f64(pos), torch.full((1,), step, dtype=torch.int64, device="cuda")
                q, zf = torch.empty((ns, nd), dtype=torch.float64, device="cuda"), torch.empty(ns, dtype=torch.float64,
                                                                                             device="cuda")
                ops.propose(P, half, a, seed, step, q, zf)
                np.testing.assert_array_equal(q.cpu().numpy(), qh)
                np.testing.assert_allclose(zf.cpu().numpy(), zh, rtol=1e-15, atol=1e-15)
                q2, zf2 = torch.full_like(q, np.nan), torch.full_like(zf, np.nan)
                ops.propose_dev(P, half, a, seed, stepd, q2, zf2)
                assert torch.equal(q2, q) and torch.equal(zf2, zf)
                new = _plant(rng, lnp[sl], ns, k + half)
                ph, lh, nh = pos.copy(), lnp0.copy(), np.zeros(W, np.int64)
                acc = sd.accept(ph, lh, half, qh, zh, new, seed, step, nh)
                for i in range(min(ns, 3)):
                    assert acc[i] == (new[i] == np.inf) or lnp0[half * ns + i] == -np.inf
                    kinds.add((repr(float(new[i])), bool(acc[i])))
                if ns > 3:
                    assert acc[ns - 1] and np.isfinite(new[ns - 1])   # -inf old: its finite proposal is taken
                vh = np.where(acc, new, np.nan)
                NEW, V = _f64(new), _f64(vh)
                for entry in ("accept", "accept_dev", "accept_regen", "apply_verdicts"):
                    buf, Pd = _guarded(pos)
                    Ld, na = _f64(lnp0), torch.zeros(W, dtype=torch.int32, device="cuda")
                    if entry == "accept":
                        ops.accept(Pd, Ld, half, q, zf, NEW, seed, step, na)
                    elif entry == "accept_dev":
                        ops.accept_dev(Pd, Ld, half, q, zf, NEW, seed, stepd, na)
                    elif entry == "accept_regen":
                        ops.accept_regen(Pd, Ld, half, a, NEW, seed, step, na)
                    else:
                        _apply_verdicts(Pd, Ld, half, a, seed, step, V, na)
                    where = (entry, W, nd, a, seed, step, half)
                    np.testing.assert_array_equal(Pd.cpu().numpy(), ph, err_msg=str(where))
                    np.testing.assert_array_equal(Ld.cpu().numpy(), lh, err_msg=str(where))
                    np.testing.assert_array_equal(na.cpu().numpy(), nh, err_msg=str(where))
                    assert _guards_intact(buf), where
    # every planted value met both as a rejection (-inf, NaN) and an acceptance (+inf)
    assert {("-inf", False), ("nan", False), ("inf", True)} <= kinds


@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("W", WS)
def test_z_and_partner_at_every_entry_point(W, a):
    """z read back exactly: with the moving half at 1 and the partner half at
    0 a proposal row is fma(1 - 0, z, 0) = z.  It is z_of(u, a,
    contracted=True), fma(a - 1, u, 1)^2 / a, bit for bit, at lfg_stretch_propose,
    _propose_dev, _accept_regen, _apply_verdicts and lfg_pt_propose; the
    other reading differs from the device on the draws where the two part.
    The partner: with the moving half at 0 and partner row j at j + 1 the row
    is fma(-(j + 1), z, j + 1), which names j."""
    import torch
    from lfit_python_amd import sampler
    ops, pt = sampler.HipStretchOps(torch.device("cuda")), sampler.HipPTOps(torch.device("cuda"))
    ns, nd = W // 2, 3
    parted = 0
    for seed, step in SEEDS:
        for half in (0, 1):
            sl, ot = slice(half * ns, (half + 1) * ns), slice((1 - half) * ns, (2 - half) * ns)
            r = sd.draw(seed, step, half, 0, ns)
            u = sd.u53(r[0], r[1])
            z1, z0 = sd.z_of(u, a, True), sd.z_of(u, a, False)
            j = [int(x) * ns >> 32 for x in r[2]]                 # __umulhi(r.z, ns) by hand
            pos = np.zeros((W, nd))
            pos[sl] = 1.0
            P, stepd = _f64(pos), torch.full((1,), step, dtype=torch.int64, device="cuda")
            q, zf = torch.empty((ns, nd), dtype=torch.float64, device="cuda"), torch.empty(ns, dtype=torch.float64,
                                                                                         device="cuda")
            got = {}
            ops.propose(P, half, a, seed, step, q, zf)
            got["propose"] = q.cpu().numpy()
            ops.propose_dev(P, half, a, seed, stepd, q, zf)
            got["propose_dev"] = q.cpu().numpy()
            pt.propose(P.view(1, W, nd), half, a, seed, step, q, zf)
            got["pt_propose"] = q.cpu().numpy()
            take = _f64(np.full(ns, np.inf))
            for entry in ("accept_regen", "apply_verdicts"):
                Pd, Ld = P.clone(), torch.zeros(W, dtype=torch.float64, device="cuda")
                na = torch.zeros(W, dtype=torch.int32, device="cuda")
                if entry == "accept_regen":
                    ops.accept_regen(Pd, Ld, half, a, take, seed, step, na)
                else:
                    _apply_verdicts(Pd, Ld, half, a, seed, step, take, na)
                assert int(na.sum()) == ns
                got[entry] = Pd[sl].cpu().numpy()
            for entry, rows in got.items():
                for d in range(nd):
                    np.testing.assert_array_equal(rows[:, d], z1, err_msg=str((entry, W, a, seed, step, half)))
            parted += int(np.sum(z1 != z0))
            if a == 2.0:
                np.testing.assert_array_equal(z1, z0)
            # partners
            pos = np.zeros((W, nd))
            pos[ot] = (np.arange(ns) + 1.0)[:, None]
            ops.propose(_f64(pos), half, a, seed, step, q, zf)
            rows = q.cpu().numpy()
            want = sd.fma(-(np.array(j) + 1.0), z1, np.array(j) + 1.0)
            for d in range(nd):
                np.testing.assert_array_equal(rows[:, d], want)
            far = np.abs(1.0 - z1) > 1e-2
            np.testing.assert_array_equal(np.rint(rows[far, 0] / (1.0 - z1[far])).astype(int) - 1, np.array(j)[far])
            assert max(j) < ns and sd.stretch_draws(ns, half, a, seed, step)[1].tolist() == j
    if a != 2.0 and W >= 126:
        assert parted > 0      # the comparison above did tell the two readings apart


@pytest.mark.parametrize("a", AS)
@pytest.mark.parametrize("W", (4, 10, 130))
def test_one_dimension(W, a):
    """ndim = 1: zfac = 0 ln z is exactly 0 (z > 0 is finite: never 0 x inf,
    never NaN), and the re-forming acceptance moves column 0 of its own row
    and nothing else (lanes 1 .. 63 of the wave have no column)."""
    import torch
    from lfit_python_amd.sampler import HipStretchOps
    ops = HipStretchOps(torch.device("cuda"))
    ns = W // 2
    rng = np.random.default_rng(W)
    pos = rng.standard_normal((W, 1))
    for seed, step in SEEDS:
        for half in (0, 1):
            sl = slice(half * ns, (half + 1) * ns)
            qh, zh = sd.propose(pos, half, a, seed, step, exact=True)
            assert np.all(zh == 0.0)
            q, zf = torch.empty((ns, 1), dtype=torch.float64, device="cuda"), torch.full((ns,), np.nan,
                                                                                        dtype=torch.float64, device="cuda")
            ops.propose(_f64(pos), half, a, seed, step, q, zf)
            assert bool((zf == 0.0).all())
            np.testing.assert_array_equal(q.cpu().numpy(), qh)
            new = np.where(np.arange(ns) % 2 == 0, np.inf, -np.inf)    # every other walker moves
            for entry in ("accept_regen", "apply_verdicts"):
                buf, Pd = _guarded(pos)
                Ld, na = torch.zeros(W, dtype=torch.float64, device="cuda"), torch.zeros(W, dtype=torch.int32,
                                                                                        device="cuda")
                if entry == "accept_regen":
                    ops.accept_regen(Pd, Ld, half, a, _f64(new), seed, step, na)
                else:
                    _apply_verdicts(Pd, Ld, half, a, seed, step, _f64(np.where(new > 0, new, np.nan)), na)
                want = pos.copy()
                want[sl][::2] = qh[::2]
                np.testing.assert_array_equal(Pd.cpu().numpy(), want)
                assert _guards_intact(buf)
                assert na.cpu().numpy().tolist() == [int(half * ns <= w < (half + 1) * ns and (w - half * ns) % 2 == 0)
                                                     for w in range(W)]


@pytest.mark.parametrize("mutate", sd.MUTATIONS)
def test_every_mutation_is_seen(mutate):
    """the device's rows and acceptance (W = 10, a = 2.5, MUTATION_CASE's seed
    and step) equal the double's and miss each mutated double's"""
    import torch
    from lfit_python_amd.sampler import HipStretchOps
    ops = HipStretchOps(torch.device("cuda"))
    W, nd = 10, 7
    a, seed, step = sd.MUTATION_CASE
    rng = np.random.default_rng(2)
    pos = rng.standard_normal((W, nd))
    lnp = rng.standard_normal(W)
    new = lnp.reshape(2, 5) + rng.standard_normal((2, 5))
    seen = False
    for half in (0, 1):
        q, zf = torch.empty((5, nd), dtype=torch.float64, device="cuda"), torch.empty(5, dtype=torch.float64,
                                                                                     device="cuda")
        P, Ld = _f64(pos), _f64(lnp)
        na = torch.zeros(W, dtype=torch.int32, device="cuda")
        ops.propose(P, half, a, seed, step, q, zf)
        ops.accept_regen(P, Ld, half, a, _f64(new[half]), seed, step, na)
        for m in (None, mutate):
            qh, _ = sd.propose(pos, half, a, seed, step, exact=True, mutate=m)
            ph, lh, nh = pos.copy(), lnp.copy(), np.zeros(W, np.int64)
            sd.accept_regen(ph, lh, half, a, new[half], seed, step, nh, mutate=m)
            same = np.array_equal(q.cpu().numpy(), qh) and np.array_equal(P.cpu().numpy(), ph)
            if m is None:
                assert same
            else:
                seen = seen or not same
    assert seen


# --------------------------------------------- part 2: the modes against the host chain
ITERS = 5
TRIP_SEED0, TRIP_SEED = 41, 41
OUTSIDE = 1   # the walker that starts outside q's uniform prior in `odd` and `nine`
#        W     ranks   tree       a    seed        first step   layouts          graph
CASES = {
    "min": (4, (1, 2), "complex", 2.5, 2**40 + 7, 0, ("pair", "two_kernel"), True),
    "odd": (6, (3,), "complex", 1.3, 7, 2**32 - 2, ("pair", "two_kernel"), True),
    "nine": (18, (3,), "complex", 2.5, 2**63 + 1, 2**32 - 2, ("pair", "two_kernel"), False),
    "nine_simple": (18, (3,), "simple", 2.5, 2**63 + 1, 2**32 - 2, ("pair", "two_kernel"), False),
    "wave": (130, (5,), "complex", 2.5, 21, 0, ("pair", "two_kernel"), True),
    "tree": (None, (1,), "e6", 2.5, 23, 2**32 - 1, ("default",), False),   # W = 2 ndim + 2 = 170: ns = 85 is odd
    "long": (10, (5,), "long", 1.3, 29, 0, ("default",), False),
    "gp": (10, (1,), "gp", 2.5, 31, 0, ("default",), False),
    # Two cases for the reading of z in the chains.  At a = 2.5 the two readings of (a - 1) u + 1
    # part only for u > 2/3 (z >= 1.6), moves that these tight ensembles never accept, so there the chains
    # cannot tell the readings apart at a site that RE-forms an accepted row (accept_regen, apply_verdicts,
    # fold_rows, the candidates); at a = 1.3 they part over z in 0.85 .. 1.3.  `wave` at a = 1.3, and `long`
    # with the first seed from 30 at which 7 of the 50 draws part (none of `long`'s do; the LONG k_pair
    # units are compiled apart from the rest).
    "wave_parts": (130, (5,), "complex", 1.3, 21, 0, ("pair", "two_kernel"), True),
    "long_parts": (10, (5,), "long", 1.3, 102, 0, ("default",), False),
    # MODEL_SPEC 10.3's cache rule in the middle of the ensemble: the E = 1 ladder tree of tests/gp_trees.py
    # with the cache's rwd at 2.2 x the start value and its dist_cp unfilled (the device fills it), so that
    # walkers below the start rwd trip the rule (k_gp_dcp; in k_pair<GP> wave 0's lanes write G_GP_DCP and
    # G_GP_OK of the slot wave 7 copies the chosen candidate's record into) and those above it do not.  The
    # first seed from TRIP_SEED0 at which _check_preconditions' conditions for this case hold.
    "gp_trip": (12, (1, 3), "gp_trip", 2.5, TRIP_SEED, 0, ("pair", "two_kernel"), True),
}
# cases in which an accepted move sits on a draw where the readings part
PARTED = ("wave_parts", "long_parts")
SAMPLER_MODES = ("separate", "spec", "step_half", "lnprob_accept", "shard1", "shard1_spec", "fold")
LAYOUT_ID = {"pair": 1, "two_kernel": 0, "default": -1}


def _grid():
    out = []
    for name, (W, ranks, tree, a, seed, step0, layouts, graph) in CASES.items():
        for lay in layouts:
            modes = SAMPLER_MODES + (("graph",) if graph else ()) + tuple("ranks%d" % R for R in ranks)
            out += [pytest.param(name, lay, m, id="%s-%s-%s" % (name, lay, m)) for m in modes]
    return out


_trees, _refs = {}, {}


def _tree(kind, oracle):
    if kind not in _trees:
        from lfit_python_amd import batch, synthetic
        nsub = 1
        if kind == "complex":
            m = synthetic.config_single(65, flux_fn=_flux_fn)
        elif kind == "simple":
            m = synthetic.config_single(65, complex_bs=False, flux_fn=_flux_fn)
        elif kind == "e6":
            m = synthetic.config_tree(2, 65, flux_fn=_flux_fn)
        elif kind == "long":
            nsub = 3
            m = synthetic.config_single(513, flux_fn=_flux_fn, nsub=3)
        elif kind == "gp_trip":
            from tests import gp_trees
            m, _ = gp_trees.rule_case(oracle, "rule_e1")
        else:
            from tests import gp_trees
            m, nsub = gp_trees._tree(oracle, "cuts")
        t = batch.compile_tree(m, nsub=nsub)
        if kind == "gp_trip":
            t.gp_base[:, 2] *= 2.2
            t.gp_base[:, 3] = np.nan
        _trees[kind] = (m, t)
    return _trees[kind]


class _Layout:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from lfit_python_amd import _native
        self.prev = _native.lib().lfg_set_layout(self.mode)

    def __exit__(self, *exc):
        from lfit_python_amd import _native
        _native.lib().lfg_set_layout(self.prev)


def _reference(name, lay, oracle):
    """The case's start and its host chain with ln_prob evaluated on layout
    `lay`; computed once, shared by the modes, never written"""
    key = (name, lay)
    if key not in _refs:
        import torch
        from lfit_python_amd import batch, sampler
        W, ranks, kind, a, seed, step0, _, _ = CASES[name]
        m, t = _tree(kind, oracle)
        W = W or 2 * t.ndim + 2
        with _Layout(LAYOUT_ID[lay]):
            ev = batch.LnProbEvaluator(t)
            fn = lambda p: ev(torch.as_tensor(np.ascontiguousarray(p), device="cuda")).cpu().numpy()
            p0 = np.array(m.dynasty_par_vals)
            init = sampler.initialise_walkers(p0, sampler.comp_scatter(m.dynasty_par_names, 0.1), W, fn, seed=W)
            if name in ("odd", "nine", "nine_simple"):
                init[OUTSIDE, list(m.dynasty_par_names).index("q_core")] = 0.51   # uniform 0.03 .. 0.5
            lnp0 = fn(init)
            c = sd.chain(init, lnp0, fn, a, seed, step0, ITERS)
        for x in (init, lnp0, c.pos, c.lnp, c.naccept, c.acc, c.lnp_new):
            x.setflags(write=False)
        _refs[key] = (t, init, lnp0, c)
    return _refs[key]


def _sampler_chain(mode, t, init, lnp0, a, seed, step0):
    import torch
    from lfit_python_amd import batch, sampler
    ev = batch.LnProbEvaluator(t)
    S = sampler.EnsembleSampler(init.shape[0], t.ndim, ev, a=a, seed=seed)
    S.fuse = mode in ("spec", "step_half", "lnprob_accept")
    S.spec = mode in ("spec", "shard1_spec", "fold")
    S.force_shard = mode in ("shard1", "shard1_spec", "fold")
    S.fold = mode == "fold"
    S.use_graph = mode == "graph"
    if mode == "lnprob_accept":
        def half(pos, lnp, h, a_, seed_, step, q, zfac, naccept, lnp_new=None):
            S.ops.propose(pos, h, a_, seed_, step, q, zfac)
            ev.lnprob_accept(q, pos, lnp, h, zfac, seed_, step, naccept, lnp_new=lnp_new)
        S.half_timer = half
    S.set_state(init.copy(), lnp0.copy())   # (the shared reference is read-only)
    S.random_state = step0
    S.run_mcmc(None, ITERS)
    assert S.random_state == step0 + ITERS
    if mode == "graph":
        assert S._graph is not None and int(S._step_dev.item()) == step0 + ITERS
    if mode == "fold":
        assert S._V is not None
    if mode in ("spec", "shard1_spec"):
        assert ev._spec_key is not None          # the candidates were live to the end
    torch.cuda.synchronize()
    return S.chain_dev.cpu().numpy(), S.lnprob_dev.cpu().numpy(), S.naccept.cpu().numpy()


def _rank_chains(t, init, lnp0, a, seed, step0, R):
    """R ranks' workspaces driven by hand (tests/test_gpu_fold.py's pattern):
    each holds the whole ensemble and runs lfg_stretch_step_shard_fold on
    walkers k n .. (k + 1) n - 1 of every half; the verdict shards
    concatenated as the all_gather hands them over"""
    import torch
    from lfit_python_amd import batch
    W = init.shape[0]
    n = W // 2 // R
    assert n * R == W // 2
    f64 = dict(dtype=torch.float64, device="cuda")
    evs = [batch.LnProbEvaluator(t, max_walkers=W // 2) for _ in range(R)]
    pos = [torch.as_tensor(init.copy(), **f64).contiguous() for _ in range(R)]
    lnp = [torch.as_tensor(lnp0.copy(), **f64) for _ in range(R)]
    nacc = [torch.zeros(W, dtype=torch.int32, device="cuda") for _ in range(R)]
    q = [torch.empty((n, t.ndim), **f64) for _ in range(R)]
    zf, lsh, vsh = ([torch.empty(n, **f64) for _ in range(R)] for _ in range(3))
    V = [None, None]
    chain, lchain, spec_used = [], [], 0

    def record():
        for k in range(1, R):
            assert torch.equal(pos[k], pos[0]) and torch.equal(lnp[k], lnp[0]) and torch.equal(nacc[k], nacc[0])
        chain.append(pos[0].cpu().numpy())
        lchain.append(lnp[0].cpu().numpy())

    for it in range(ITERS):
        for half in (0, 1):
            vprev = V[1 - half]
            for k in range(R):
                key = evs[k]._spec_key
                spec_used += int(key is not None and key[-2:] == (half, step0 + it) and vprev is not None)
                evs[k].step_shard_fold(pos[k], lnp[k], half, a, seed, step0 + it, k * n, q[k], zf[k], lsh[k], vprev,
                                       vsh[k], nacc[k])
            if half == 0 and it > 0:
                record()
            V[half] = torch.cat(vsh)
            lall, acc = torch.cat(lsh), ~torch.isnan(V[half])
            assert torch.equal(V[half][acc], lall[acc])
    for k in range(R):
        evs[k].apply_verdicts(pos[k], lnp[k], 1, a, seed, step0 + ITERS - 1, V[1], nacc[k])
    record()
    assert spec_used == R * (2 * ITERS - 1)
    return np.stack(chain), np.stack(lchain), nacc[0].cpu().numpy()


def _check_preconditions(name, c, a, seed, step0):
    """conditions of the comparison, not measurements: no decision within
    1e-9 of its threshold (an ulp of log cannot flip it), both verdicts in
    each half, a pair whose partner moved in the half-step before (the
    speculative lanes' candidate 1)"""
    assert c.margin >= 1e-9, (name, c.margin)
    ns = c.acc.shape[2]
    for half in (0, 1):
        assert c.acc[:, half].any() and not c.acc[:, half].all(), (name, half)
    cand1 = 0
    for it in range(ITERS):
        for half in (0, 1):
            if it == 0 and half == 0:
                continue
            prev = c.acc[it, 0] if half == 1 else c.acc[it - 1, 1]
            cand1 += int(prev[sd.stretch_draws(ns, half, a, seed, step0 + it)[1]].sum())
    assert cand1 > 0, name
    if name in PARTED:
        parted = 0
        for it in range(ITERS):
            for half in (0, 1):
                r = sd.draw(seed, step0 + it, half, 0, ns)
                u = sd.u53(r[0], r[1])
                parted += int((c.acc[it, half] & (sd.z_of(u, a, True) != sd.z_of(u, a, False))).sum())
        assert parted > 0, name


def _trip_conditions(t, init, c, a, seed, step0):
    """gp_trip, on the host chain: the proposals replayed from the recorded
    decisions; a list of what fails (empty: the case stands)"""
    from tests import gp_trees
    from tests import wdphases_double as wd
    base = tuple(t.gp_base[0, :3])
    ns = c.acc.shape[2]

    def trip(rows):
        p = np.array([gp_trees.eclipse_pars(t, 0, v) for v in rows])
        near = [abs(abs(B - v) / v - wd.RULE) <= 1e-6 * wd.RULE for B, col in zip(base, (4, 5, 8)) for v in p[:, col]]
        return np.array([wd.tripped(base, v[4], v[5], v[8]) for v in p]), any(near)
    pos = np.array(init)
    prop = {(True, False): 0, (False, True): 0}     # (the walker's row tripped, its proposal tripped)
    took = dict(prop)
    near_any, cand1_pending = False, 0
    for it in range(ITERS):
        for half in (0, 1):
            sl = slice(half * ns, (half + 1) * ns)
            q, _ = sd.propose(pos, half, a, seed, step0 + it, exact=True)
            now, _ = trip(pos[sl])
            new, near = trip(q)
            near_any = near_any or near
            acc = c.acc[it, half]
            for k in range(ns):
                if (now[k], new[k]) in prop:
                    prop[(now[k], new[k])] += 1
                    took[(now[k], new[k])] += int(acc[k])
            if it or half:
                prev = c.acc[it, 0] if half == 1 else c.acc[it - 1, 1]
                cand1_pending += int((prev[sd.stretch_draws(ns, half, a, seed, step0 + it)[1]] & new).sum())
            pos[sl][acc] = q[acc]
        if not np.array_equal(pos, c.pos[it]):
            return ["the replay left the chain at step %d" % it]
    bad = ["no proposal %s -> %s" % k for k, n in prop.items() if n == 0]
    bad += ["no accepted proposal %s -> %s" % k for k, n in took.items() if n == 0]
    bad += ["no pending candidate-1 pair"] * (cand1_pending == 0)
    bad += ["a proposal within 1e-6 of the rule's threshold"] * bool(near_any)
    return bad


@pytest.mark.parametrize("name,lay,mode", _grid())
def test_mode_matches_the_host_chain(name, lay, mode, oracle):
    """positions, ln_prob and acceptance counters of one mode, bit for bit"""
    W, ranks, kind, a, seed, step0, _, _ = CASES[name]
    R = int(mode[5:]) if mode.startswith("ranks") else 0
    t = _tree(kind, oracle)[1]
    n = ((W or 2 * t.ndim + 2) // 2 // R) if R else 0
    # a shard too small for its speculative lanes' two whole waves (fewer
    # than two pairs: lnprob_impl's pair_path) runs on the two-kernel layout
    # whatever lfg_set_layout says; its ln_prob sums are that layout's
    ref_lay = "two_kernel" if (R and n * t.E < 2) else lay
    t, init, lnp0, c = _reference(name, ref_lay, oracle)
    _check_preconditions(name, c, a, seed, step0)
    if name == "gp_trip":
        assert np.isnan(t.gp_base[:, 3]).all() and _trip_conditions(t, init, c, a, seed, step0) == []
    with _Layout(LAYOUT_ID[lay]):
        if R:
            got = _rank_chains(t, init, lnp0, a, seed, step0, R)
        else:
            got = _sampler_chain(mode, t, init, lnp0, a, seed, step0)
    np.testing.assert_array_equal(got[0], c.pos)
    np.testing.assert_array_equal(got[1], c.lnp)
    np.testing.assert_array_equal(got[2], c.naccept[-1])
    if name in ("odd", "nine", "nine_simple"):
        # the walker outside the prior: -inf at the start, it takes its first
        # finite proposal (diff = +inf) and its counter says so
        assert lnp0[OUTSIDE] == -np.inf
        fin = np.flatnonzero(np.isfinite(c.lnp_new[:, 0, OUTSIDE]))
        assert fin.size, name
        first = int(fin[0])
        assert not np.isfinite(got[1][:first, OUTSIDE]).any()
        assert got[1][first, OUTSIDE] == c.lnp_new[first, 0, OUTSIDE]
        assert np.array_equal(got[0][:first, OUTSIDE], np.broadcast_to(init[OUTSIDE], (first, init.shape[1])))
        assert not np.array_equal(got[0][first, OUTSIDE], init[OUTSIDE])
        assert c.naccept[first][OUTSIDE] == 1 and got[2][OUTSIDE] >= 1
