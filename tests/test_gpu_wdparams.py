"""GPU: lfg_wd_lnprob and lfg_wd_step_half (include/lfg_wd.h; MODEL_SPEC
section 13) and lfit_python_amd.wdparams on the device.

  parity    the fixed batch of tests/wd_double.py against the scipy double,
            every prior set, with and without colour corrections: status
            equal, magnitudes to 1e-12, ln_prob and ln_like within each row's
            propagated bound (tests/wd_double.py)
  counts    n of 1, 63, 64, 65, 255, 256, 257: row i of any batch is
            bit-identical to the same row evaluated alone, and a second run
            of a batch to the first
  strides   a chain read in place (ld = 9) and a thinned view of it
  guards    tests/abi_guard.py's arena: every output exactly its shape and
            written, inputs and tables unchanged, guard bytes intact; the
            same on a side stream with the default stream kept busy
  fused     lfg_wd_step_half against propose -> lfg_wd_lnprob -> accept for W
            of 8, 130 and 514, 5 steps: pos, lnp, naccept (and q, zfac,
            lnp_new) bit-identical; so is the HIP-graph replay
  samplers  PTSampler's stored state against a fresh evaluation; a planted
            truth recovered by the ensemble sampler; the driver end to end
All shapes are small: 257 rows evaluated alone are the reference of the counts.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import abi_guard as ag
from tests import wd_double as wdd

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65, 255, 256, 257)
NROWS = 257


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    import torch
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def model():
    return wdd.build_model("A", True)


@pytest.fixture(scope="module")
def ev(model):
    from lfit_python_amd import wdparams
    return wdparams.WDEvaluator(model)


@pytest.fixture(scope="module")
def rows():
    """257 rows: the whole fixed batch, repeated and shuffled"""
    b, _ = wdd.shared("A", True)
    k = (np.arange(NROWS) % len(b["theta"]))[np.random.default_rng(5).permutation(NROWS)]
    return b["theta"][k].copy()


def _eval(ev, x, ld=None, n=None):
    """(lnp, lnlike, mags [B, n], status) of rows of a device tensor"""
    import torch
    n = x.shape[0] if n is None else n
    dev, B = ev.device, ev.model.B
    lnp = torch.empty(n, dtype=torch.float64, device=dev)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    mags = torch.empty((B, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ev.evaluate(x, ld=ld, n=n, out=lnp, lnlike=ll, mags=mags, status=st)
    return lnp, ll, mags, st


@pytest.fixture(scope="module")
def alone(ev, rows):
    """every one of the 257 rows evaluated alone"""
    import torch
    x = torch.as_tensor(rows, device=ev.device)
    got = [_eval(ev, x[i:i + 1]) for i in range(NROWS)]
    return (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got]), torch.cat([g[2] for g in got], dim=1),
            torch.cat([g[3] for g in got]))


@pytest.mark.parametrize("prior_set,corrected", wdd.COMBOS)
def test_parity_with_the_double(prior_set, corrected):
    import torch
    from lfit_python_amd import wdparams
    b, ref = wdd.shared(prior_set, corrected)
    e = wdparams.WDEvaluator(wdd.build_model(prior_set, corrected))
    lnp, ll, mags, st = (t.cpu().numpy() for t in _eval(e, torch.as_tensor(b["theta"], device=e.device)))
    dm, rel = wdd.check_against(lnp, mags.T, ll, st, ref, "device")
    print("device - double: magnitudes %.3g, ln_prob %.3g of its bound" % (dm, rel))
    # the evaluator's call is the same launch
    assert np.array_equal(e(torch.as_tensor(b["theta"], device=e.device)).cpu().numpy(), lnp)


@pytest.mark.parametrize("n", COUNTS)
def test_counts_are_bit_identical_to_rows_alone(ev, rows, alone, n):
    import torch
    x = torch.as_tensor(rows[:n], device=ev.device)
    got = _eval(ev, x)
    want = (alone[0][:n], alone[1][:n], alone[2][:, :n], alone[3][:n])
    assert _same(got, want)
    assert _same(_eval(ev, x), got)


def test_a_strided_chain_is_read_in_place(ev, rows, alone):
    import torch
    ld, thin, n = 9, 3, 200
    chain = np.random.default_rng(2).uniform(-1, 1, (n, ld))
    chain[:, 2:6] = rows[:n]
    c = torch.as_tensor(chain, device=ev.device)
    flat = c.reshape(-1)
    got = _eval(ev, flat[2:], ld=ld, n=n)
    assert _same(got, (alone[0][:n], alone[1][:n], alone[2][:, :n], alone[3][:n]))
    assert _same((c.cpu(),), (torch.as_tensor(chain),))      # (bit for bit: the rows hold NaN)
    k = -(-n // thin)
    got = _eval(ev, flat[2:], ld=thin * ld, n=k)
    assert _same(got, (alone[0][:n:thin], alone[1][:n:thin], alone[2][:, :n:thin], alone[3][:n:thin]))
    # a [n, 9] view's columns 2..5 through the tensor's own stride
    assert _same(_eval(ev, c[:, 2:6]), (alone[0][:n], alone[1][:n], alone[2][:, :n], alone[3][:n]))


# ------------------------------------------------------------------ guarded buffers
def _guarded(A, model, rows, n, ld=4):
    import torch
    from lfit_python_amd import _native
    tab = {name: A.inp("tab_" + name, a) for name, a in model.arrays.items()}
    S = model.struct_over(lambda name: tab[name].data_ptr())
    chain = np.full((n, ld), 3.0)
    chain[:, :4] = rows[:n]
    th = A.inp("theta", chain.reshape(-1)[:(n - 1) * ld + 4])   # ends on the last row's fourth column
    lnp = A.out("lnp", (n,), torch.float64)
    ll = A.out("lnlike", (n,), torch.float64)
    mags = A.out("mags", (model.B, n), torch.float64)
    st = A.out("status", (n,), torch.int32)
    rc = _native.lib().lfg_wd_lnprob(ag.ptr(th), ld, n, ctypes.byref(S), ag.ptr(lnp), ag.ptr(ll), ag.ptr(mags),
                                     ag.ptr(st), A.stream_ptr())
    assert rc == 0
    A.check()                                   # guards intact, inputs and tables unchanged
    assert not any(A.poisoned(k).any() for k in ("lnp", "lnlike", "mags", "status"))
    return lnp.clone(), ll.clone(), mags.clone(), st.clone()


@pytest.fixture(scope="module")
def arena():
    return ag.Arena(nbytes=16 * 1024 * 1024)


@pytest.mark.parametrize("n,ld", ((1, 4), (257, 4), (65, 6)))
def test_guarded_buffers(model, rows, alone, arena, n, ld):
    arena.reset(ag.POISON)
    got = _guarded(arena, model, rows, n, ld)
    assert _same(got, (alone[0][:n], alone[1][:n], alone[2][:, :n], alone[3][:n]))


def test_guarded_buffers_on_a_side_stream(model, rows, alone, arena):
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    x = torch.full((2048, 2048), 1e-3, device="cuda")
    for _ in range(16):                          # the default stream is kept busy meanwhile
        x = x @ x
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        arena.reset(ag.POISON)
        got = _guarded(arena, model, rows, NROWS)
        assert _same(got, alone)
    torch.cuda.synchronize()


def test_argument_checks_launch_nothing(ev, model):
    import torch
    from lfit_python_amd import _native
    L = _native.lib()
    x = torch.zeros((4, 4), dtype=torch.float64, device=ev.device)
    out = torch.full((4,), 7.0, dtype=torch.float64, device=ev.device)
    S, sp = ev.M, _native.stream_ptr(ev.device)
    E = -1   # LFG_E_ARGS
    assert L.lfg_wd_lnprob(ag.ptr(x), 4, 0, ctypes.byref(S), None, None, None, None, sp) == 0
    assert L.lfg_wd_lnprob(ag.ptr(x), 3, 4, ctypes.byref(S), ag.ptr(out), None, None, None, sp) == E
    assert L.lfg_wd_lnprob(ag.ptr(x), 4, -1, ctypes.byref(S), ag.ptr(out), None, None, None, sp) == E
    assert L.lfg_wd_lnprob(None, 4, 4, ctypes.byref(S), ag.ptr(out), None, None, None, sp) == E
    assert L.lfg_wd_lnprob(ag.ptr(x), 4, 4, ctypes.byref(S), None, None, None, None, sp) == E
    assert L.lfg_wd_lnprob(ag.ptr(x), 4, 4, None, ag.ptr(out), None, None, None, sp) == E
    bad = model.device_struct(ev.device).__class__.from_buffer_copy(S)
    bad.B = 9
    assert L.lfg_wd_lnprob(ag.ptr(x), 4, 4, ctypes.byref(bad), ag.ptr(out), None, None, None, sp) == E
    bad.B, bad.ny = S.B, 129
    assert L.lfg_wd_lnprob(ag.ptr(x), 4, 4, ctypes.byref(bad), ag.ptr(out), None, None, None, sp) == E
    assert L.lfg_wd_step_half(ag.ptr(x), ag.ptr(out), 3, 0, 2.0, 1, 0, None, ctypes.byref(S), ag.ptr(x), ag.ptr(out),
                              ag.ptr(out), None, sp) == E
    assert L.lfg_wd_step_half(ag.ptr(x), ag.ptr(out), 4, 0, 1.0, 1, 0, None, ctypes.byref(S), ag.ptr(x), ag.ptr(out),
                              ag.ptr(out), None, sp) == E
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------ the samplers
def _start(ev, W, seed):
    """W walkers in a ball around the flux set's white dwarf, all with a finite ln_prob"""
    from lfit_python_amd import sampler
    import torch
    f = lambda p: ev(torch.as_tensor(p, dtype=torch.float64, device=ev.device)).cpu().numpy()
    return sampler.initialise_walkers(np.array([13000.0, 8.2, 2.4, 0.006]), 0.05, W, f, seed=seed)


def _fused_matches_three_launches(ev, W, a, seed):
    import torch
    from lfit_python_amd import sampler
    p0 = _start(ev, W, seed=W)
    fused, three, graph = (sampler.EnsembleSampler(W, 4, ev, a=a, seed=seed) for _ in range(3))
    assert fused.fuse and three.fuse
    three.fuse = graph.fuse = False
    graph.use_graph = True
    for S in (fused, three, graph):
        S.set_state(p0)
    for step in range(5):
        for S in (fused, three, graph):
            S.step()
        torch.cuda.synchronize()
        for S in (fused, graph):
            assert _same((S.pos, S.lnp, S.naccept), (three.pos, three.lnp, three.naccept)), (step, S is graph)
        assert _same((fused.q, fused.zfac, fused.lnp_new), (three.q, three.zfac, three.lnp_new)), step
    assert graph._graph is not None                      # the replay path ran
    assert int(three.naccept.sum()) > 0 and int((three.naccept < 5).sum()) > 0   # both verdicts occurred


@pytest.mark.parametrize("W", (8, 130, 514))
def test_fused_half_step_matches_three_launches(ev, W):
    _fused_matches_three_launches(ev, W, 2.0, 77)


def test_fused_half_step_matches_three_launches_off_a2(ev):
    """a = 2.5, a seed past 2^32: (a - 1) u is no longer exact, so the fused
    kernel's fma(a - 1, u, 1) must be what k_propose's unit forms"""
    _fused_matches_three_launches(ev, 130, 2.5, 2**40 + 77)


def test_fused_half_step_matches_the_exact_double_off_a2(ev):
    """lfg_wd_step_half at a = 2.5, seed and step past 2^32, against the
    stretch move's host double in the device's arithmetic: rows bit-identical,
    zfac to 1e-15, and with the device's own ln_prob of the proposals the
    host's verdicts, ensemble and counters exactly"""
    import torch
    from lfit_python_amd import _native
    from tests import stretch_double as sd
    W, a, seed, step = 130, 2.5, 2**40 + 7, 2**32 + 3
    ns = W // 2
    p0 = _start(ev, W, seed=3)
    P0 = torch.as_tensor(p0, device=ev.device)
    lnp0 = ev(P0)
    f64 = dict(dtype=torch.float64, device=ev.device)
    taken = 0
    for half in (0, 1):
        pos, lnp = P0.clone(), lnp0.clone()
        q, zf, new = torch.empty((ns, 4), **f64), torch.empty(ns, **f64), torch.empty(ns, **f64)
        nacc = torch.zeros(W, dtype=torch.int32, device=ev.device)
        rc = _native.lib().lfg_wd_step_half(ag.ptr(pos), ag.ptr(lnp), W, half, a, seed, step, None,
                                            ctypes.byref(ev.M), ag.ptr(q), ag.ptr(zf), ag.ptr(new), ag.ptr(nacc),
                                            _native.stream_ptr(ev.device))
        assert rc == 0
        qh, zh = sd.propose(p0, half, a, seed, step, exact=True)
        np.testing.assert_array_equal(q.cpu().numpy(), qh)
        np.testing.assert_allclose(zf.cpu().numpy(), zh, rtol=1e-15, atol=1e-15)
        ph, lh, nh = p0.copy(), lnp0.cpu().numpy().copy(), np.zeros(W, np.int64)
        acc = sd.accept(ph, lh, half, qh, zh, new.cpu().numpy(), seed, step, nh)
        np.testing.assert_array_equal(pos.cpu().numpy(), ph)
        np.testing.assert_array_equal(lnp.cpu().numpy(), lh)
        np.testing.assert_array_equal(nacc.cpu().numpy(), nh)
        taken += int(acc.sum())
    assert 0 < taken < W


def test_fused_half_step_reads_a_device_step_counter(ev):
    import torch
    from lfit_python_amd import _native
    W = 130
    p0 = torch.as_tensor(_start(ev, W, seed=3), device=ev.device)
    lnp0 = ev(p0)

    def run(stepp, step):
        pos, lnp = p0.clone(), lnp0.clone()
        q = torch.empty((W // 2, 4), dtype=torch.float64, device=ev.device)
        zf, new = torch.empty(W // 2, dtype=torch.float64, device=ev.device), torch.empty(W // 2, dtype=torch.float64,
                                                                                         device=ev.device)
        nacc = torch.zeros(W, dtype=torch.int32, device=ev.device)
        rc = _native.lib().lfg_wd_step_half(ag.ptr(pos), ag.ptr(lnp), W, 1, 2.0, 99, step, ag.ptr(stepp),
                                            ctypes.byref(ev.M), ag.ptr(q), ag.ptr(zf), ag.ptr(new), ag.ptr(nacc),
                                            _native.stream_ptr(ev.device))
        assert rc == 0
        return pos, lnp, q, zf, new, nacc
    counter = torch.full((1,), 41, dtype=torch.int64, device=ev.device)
    assert _same(run(counter, 0), run(None, 41))
    assert not _same(run(None, 40)[:1], run(None, 41)[:1])


def test_pt_sampler_state_is_a_fresh_evaluation(ev):
    import torch
    from lfit_python_amd import pt
    T, W = 3, 8
    S = pt.PTSampler(W, 4, ev, ntemps=T, seed=5)
    p0 = np.stack([_start(ev, W, seed=10 + t) for t in range(T)])
    S.run_mcmc(p0, 3, storechain=False)
    x = S.pos.reshape(T * W, 4).contiguous()
    lnp, ll, _, _ = _eval(ev, x)
    assert _same((S.loglike.reshape(-1),), (ll,))
    assert _same((S.logprior.reshape(-1),), (lnp - ll,))
    assert int(S.naccepted.sum()) > 0


TRUTH = np.array([14500.0, 8.15, 2.6, 0.008])


def test_planted_truth_is_recovered():
    import torch
    from lfit_python_amd import sampler, wdparams
    from lfit_python_amd.tree import Param
    # the truth's own model fluxes in five bands, 3 % errors, noiseless
    D = wdd.Double("A", False)
    truth_mags = D.run(TRUTH[None])["mags"][0]
    flux = 3631e3 * 10.0 ** (-0.4 * truth_mags)
    table = wdparams.load_da_table(os.path.join(wdd.WD_ATMOS, "Bergeron", "Table_DA_sdss"))
    obs = [wdparams.Flux(f, 0.03 * f, band, syserr=0.0) for f, (band, _, _) in zip(flux, wdd.FLUXES)]
    pars = [Param.fromString(k, v) for k, v in (("teff", "14000 uniform 5000 90000"), ("logg", "8.0 uniform 7.01 9.49"),
                                                  ("plax", "2.6 gauss 2.6 0.1"), ("ebv", "0.008 uniform 0.0 0.02"))]
    e = wdparams.WDEvaluator(wdparams.WDModel(*pars, obs, table))
    f = lambda p: e(torch.as_tensor(p, dtype=torch.float64, device=e.device)).cpu().numpy()
    W = 64
    p0 = sampler.initialise_walkers(np.array([14000.0, 8.0, 2.6, 0.008]), 0.02, W, f, seed=1)
    S = sampler.EnsembleSampler(W, 4, e, seed=2026)
    S.run_mcmc(p0, 300, storechain=False)
    S.reset()
    S.run_mcmc(None, 300)
    flat = S.flatchain
    assert flat.shape == (300 * W, 4)
    mean, sd = flat.mean(axis=0), flat.std(axis=0)
    print("mean", mean, "sd", sd, "pull", (mean - TRUTH) / sd)
    assert np.all(sd > 0) and np.all(np.abs(mean - TRUTH) <= 5.0 * sd)
    assert 0.1 < S.acceptance_fraction.mean() < 0.9


def test_driver_end_to_end(tmp_path, monkeypatch, capsys):
    from lfit_python_amd import sampler, wdparams
    rng = np.random.default_rng(8)
    names = ["wdFlux_u", "q_core", "wdFlux_g", "wdFlux_r", "wdFlux_i", "wdFlux_z"]
    W, steps = 6, 40
    chain = np.empty((steps, W, len(names)))
    chain[:, :, 1] = rng.uniform(0.05, 0.1, (steps, W))
    for col, (_, v, e) in zip((0, 2, 3, 4, 5), wdd.FLUXES):
        chain[:, :, col] = rng.normal(v, e, (steps, W))
    sampler.write_chain(str(tmp_path / "chain_prod.txt"), names, chain, np.zeros((steps, W)))
    text = open(os.path.join(wdd.WD_ATMOS, "wdinput.dat")).read()
    text = text.replace("../hierarchical_FinalFit/chain_prod.txt", "chain_prod.txt")
    text = text.replace("nburn    = 2000", "nburn    = 30").replace("nprod    = 1000", "nprod    = 20")
    text = text.replace("nwalkers = 200", "nwalkers = 16").replace("scatter  = 0.10", "scatter  = 0.01")
    text = text.replace("teff  =   20000", "teff  =   13000").replace("logg  =   7.5 ", "logg  =   8.2 ")
    (tmp_path / "wdinput.dat").write_text(text + "\ncorrect_g = tnt uspec g\nntemps = 2\n")
    monkeypatch.chdir(tmp_path)
    assert wdparams.main(["wdinput.dat", "--dir", wdd.WD_ATMOS]) == 0
    out = capsys.readouterr().out
    with open(tmp_path / "chain_wd.txt") as fh:
        assert fh.readline() == "walker_no Teff log_g Parallax E(B-V) ln_prob\n"
    c = sampler.read_chain(str(tmp_path / "chain_wd.txt"))
    assert c.shape == (16, 20, 5) and np.isfinite(c).all()
    for name in ("Teff", "log_g", "Parallax", "E(B-V)"):
        assert any(l.startswith(name + " = ") and " +" in l and " -" in l for l in out.splitlines()), name
    assert "Chisq = " in out and "lfit_python_amd.calcPhysicalParams" in out
    # the plain ensemble sampler, no chain: fluxes from the input's own keys
    (tmp_path / "wdinput2.dat").write_text(text + "\nntemps = 1\nflux_g = 0.0936 0.0011\nflux_r = 0.0732 0.0009\n"
                                           "flux_kg5 = 0.0850 0.0010\n")
    assert wdparams.main(["wdinput2.dat", "--no-chain", "--dir", wdd.WD_ATMOS]) == 0
    c2 = sampler.read_chain(str(tmp_path / "chain_wd.txt"))
    assert c2.shape == (16, 20, 5) and np.isfinite(c2).all()
    # --summarise reads the chain back and prints the same percentiles
    capsys.readouterr()
    assert wdparams.main(["wdinput2.dat", "--no-chain", "--summarise", "--dir", wdd.WD_ATMOS]) == 0
    best = np.percentile(c2[:, :, 0].reshape(-1), 50)
    assert ("Teff = %f" % best) in capsys.readouterr().out
