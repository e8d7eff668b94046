"""GPU: the chain summary kernels (include/lfg_chain.h, MODEL_SPEC section 14)
against the numpy double and the case list of tests/chain_double.py, in
guarded buffers (tests/abi_guard.py): sizes, layouts, value columns, quantile
ranks, windows and the sigma clip, R-hat, the memory contract, refusals, and
the Python layer up to the driver's --summary.

n, n_bad, min, max and ostat are exact; quant within 4 ulp of max(|a|, |b|);
mean, m2 and rhat within chain_double.moment_bound: 8 times plain FP64
numpy's own deviation from the np.longdouble evaluation of the same column,
floor 8 ulp of the result (measured: profiles/chainstats/README.md).
"""
import ctypes
import os

import numpy as np
import pytest

from tests import abi_guard as ag
from tests import chain_double as cd
from tests.abi_guard import ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from lfit_python_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def arena():
    return ag.Arena()


def call(L, A, buf, off, steps, W, C, sld, wld, window=None, fracs=cd.FRACS, rhat=False, ws_short=0):
    """lfg_chain_stats in allocator A's buffers -> (rc, dict of host arrays)"""
    import torch
    fr = np.ascontiguousarray(fracs, dtype=np.float64)
    nq = fr.size
    chain = A.inp("chain", buf)
    win = None if window is None else A.inp("window", np.ascontiguousarray(window, dtype=np.float64))
    o = {"n": A.out("n", C, torch.int64), "n_bad": A.out("n_bad", C, torch.int64)}
    for k in ("mean", "m2", "min", "max"):
        o[k] = A.out(k, C, torch.float64)
    o["ostat"] = A.out("ostat", (C, nq, 2), torch.float64)
    o["quant"] = A.out("quant", (C, nq), torch.float64)
    o["rhat"] = A.out("rhat", C, torch.float64) if rhat else None
    nbytes = L.lfg_chain_workspace_size(max(steps, 0), max(W, 0), min(max(C, 1), 4096), min(max(nq, 0), 8))
    ws = A.ws("ws", nbytes)
    rc = L.lfg_chain_stats(ctypes.c_void_p(chain.data_ptr() + 8 * off), steps, W, C, sld, wld, ptr(win),
                           fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nq, ptr(o["n"]), ptr(o["n_bad"]),
                           ptr(o["mean"]), ptr(o["m2"]), ptr(o["min"]), ptr(o["max"]), ptr(o["ostat"]),
                           ptr(o["quant"]), ptr(o["rhat"]), ptr(ws), nbytes - ws_short, A.stream_ptr())
    A.check()
    return rc, {k: (None if t is None else t.cpu().numpy()) for k, t in o.items()}


@pytest.fixture()
def device(L, arena):
    def backend(buf, off, steps, W, C, sld, wld, window, fracs, rhat):
        arena.reset()
        rc, out = call(L, arena, buf, off, steps, W, C, sld, wld, window, fracs, rhat)
        assert rc == 0
        for k, t in out.items():
            if t is not None:
                assert not arena.poisoned(k).any(), k   # every output element is written
        return out
    return backend


def test_tiles(L):
    assert L.lfg_chain_tile_rows() + 1 == 257 and (257, 1) in cd.SIZES
    assert L.lfg_chain_hist_tile(3) < 21 and L.lfg_chain_hist_tile(0) == 0 and L.lfg_chain_hist_tile(9) == 0


@pytest.mark.parametrize("size", cd.SIZES)
@pytest.mark.parametrize("kind", cd.LAYOUTS)
def test_sizes_and_layouts(device, size, kind):
    x, want = cd.shared(size[0], size[1], 7)
    cd.run_case(device, x, kind, want=want)


@pytest.mark.parametrize("C", (1, 14, 18, 21, 87))
def test_column_counts(device, C):
    """21 and 87 columns are more than one histogram tile; 14, 18 and 87 take
    the 16-byte loads in the plain layout and single loads in the padded one"""
    x, want = cd.shared(37, 6, C)
    cd.run_case(device, x, "chain_dev", want=want)
    got = cd.run_case(device, x, "padded", want=want)
    assert np.all(got["n_bad"] == want["n_bad"])    # the NaN column beyond C is never read


def test_the_offset_column_is_an_honest_case():
    """naive sum-of-squares in FP64 misses, on the 1e6 + 1e-3 N(0, 1) column, the bound held here"""
    from tests.test_chainstats_cpu import test_naive_sum_of_squares_fails_the_offset_column as naive
    naive()


def test_flat_chain(device):
    x, want = cd.shared(5003, 1, 18)
    cd.run_case(device, x, "chain_dev", want=want)


def test_quantile_ranks(device):
    rng = np.random.default_rng(11)
    fr = (0.0, 0.16, 0.5, 0.84, 1.0)
    for n in range(2, 61):
        cd.run_case(device, rng.normal(size=(n, 1, 1)), fracs=fr)


def test_eight_quantiles(device):
    x, _ = cd.shared(64, 64, 7)
    cd.run_case(device, x, fracs=(0.0, 0.025, 0.16, 0.5, 0.5, 0.84, 0.975, 1.0))


@pytest.mark.parametrize("column", ("skewed", "gapped"))
def test_sigma_clip(column):
    """five clip rounds and the final stats, never leaving the device, against
    wdparams.sigma_clipped_stats on the host copy"""
    from lfit_python_amd import chainstats, wdparams
    v = getattr(cd, column)()
    mean, med, std, s = chainstats.sigma_clipped_stats(v.reshape(-1, 1), full=True)
    keep = cd.clip_survivors(v)
    assert s.n[0] == keep.size < v.size
    if column == "gapped":
        assert cd.clip_no_intersection(v) != keep.size
    want = wdparams.sigma_clipped_stats(v)
    assert abs(mean[0] - want[0]) <= 8 * cd.ulp(np.abs(keep).max())
    assert abs(med[0] - want[1]) <= 4 * cd.ulp(np.abs(s.ostat[0, 0]).max())
    assert abs(std[0] - want[2]) <= 8 * cd.ulp(want[2])
    cd.check({k: getattr(s, k) for k in ("n", "n_bad", "mean", "m2", "min", "max", "ostat", "quant")},
             cd.expected(keep.reshape(-1, 1, 1), fracs=(0.5,)), column)


def test_window_that_excludes_everything(device):
    x, _ = cd.shared(37, 6, 7)
    r = cd.run_case(device, x, window=np.tile([1e301, 1e302], (7, 1)))
    assert np.all(r["n"] == 0) and np.all(np.isnan(r["mean"])) and np.all(np.isnan(r["quant"]))


def test_partial_window(device):
    x, _ = cd.shared(64, 64, 7)
    cd.run_case(device, x, "skipthin", window=np.tile([-0.5, 1.5], (7, 1)))


def test_rhat(device):
    from lfit_python_amd import chainstats
    from tests.test_chainstats_cpu import rhat_chains
    mixed, offset = rhat_chains()
    r = cd.run_case(device, mixed, rhat=True)
    assert np.all(np.abs(r["rhat"] - 1.0) < 0.05)
    r = cd.run_case(device, offset, "walker_major", rhat=True)
    assert np.all(r["rhat"] > 1.5)
    want = cd.expected(offset, fracs=(), rhat=True)
    got = chainstats.gr_diagnostic(np.ascontiguousarray(offset.transpose(1, 0, 2)))   # (nwalkers, nsteps, ndim)
    assert np.all(np.abs(got - want["rhat"]) <= cd.moment_bound(want["rhat"], want["rhat_np"]))
    for steps, W in ((1, 5), (5, 1)):
        assert np.all(np.isnan(cd.run_case(device, cd.chain(steps, W, 2), rhat=True)["rhat"]))
    long = np.random.default_rng(8).normal(size=(700, 3, 2))   # the steps of a walker in several chunks
    cd.run_case(device, long, rhat=True)


def test_scratch_contents_and_repeats_do_not_matter(L, arena):
    import torch
    x, want = cd.shared(64, 64, 7)
    buf, off, sld, wld = cd.layout(x, "chain_dev")
    runs = []
    for fill in (ag.POISON, 0, None, None):
        arena.reset(fill)
        rc, out = call(L, arena, buf, off, 64, 64, 7, sld, wld, rhat=True)
        assert rc == 0
        runs.append(arena.result())
    for other in runs[1:]:
        assert all(np.array_equal(runs[0][k], other[k]) for k in runs[0])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        arena.reset()
        rc, out = call(L, arena, buf, off, 64, 64, 7, sld, wld, rhat=True)
        got = arena.result()
    assert rc == 0 and all(np.array_equal(runs[0][k], got[k]) for k in runs[0])
    cd.check(out, want, "side stream")


def test_refusals_write_nothing(L, arena):
    v = np.arange(48.0)
    ok = dict(buf=v, off=0, steps=4, W=2, C=3, sld=6, wld=3, fracs=(0.5,))
    cases = [dict(steps=-1), dict(W=-1), dict(C=0), dict(C=4097), dict(sld=0), dict(wld=0), dict(fracs=(0.5, 1.5)),
             dict(fracs=(-0.1,)), dict(fracs=(np.nan,)), dict(fracs=(0.5,) * 9), dict(ws_short=1),
             dict(window=np.tile([-1.0, 1.0], (3, 1)), rhat=True)]
    for change in cases:
        arena.reset()
        args = dict(ok, **change)
        nC = min(max(args["C"], 1), 16)   # (the output buffers of a refused C only have to exist)
        rc, _ = call(L, ag_small(arena, nC), **args)
        assert rc == -1, change
        for name in ("n", "n_bad", "mean", "m2", "min", "max", "ostat", "quant"):
            assert arena.poisoned(name).all(), (change, name)
    # a null required pointer
    import torch
    arena.reset()
    n = arena.out("n", 3, torch.int64)
    fr = (ctypes.c_double * 1)(0.5)
    rc = L.lfg_chain_stats(None, 4, 2, 3, 6, 3, None, fr, 1, ptr(n), None, None, None, None, None, None, None, None,
                           None, 0, arena.stream_ptr())
    arena.check()
    assert rc == -1 and arena.poisoned("n").all()
    # steps = 0: the empty-column values
    arena.reset()
    rc, out = call(L, arena, v, 0, 0, 2, 3, 6, 3, fracs=(0.5,), rhat=True)
    assert rc == 0 and np.all(out["n"] == 0) and np.all(out["n_bad"] == 0)
    assert all(np.all(np.isnan(out[k])) for k in ("mean", "m2", "min", "max", "ostat", "quant", "rhat"))


class ag_small:
    """call()'s allocator for a refused C: outputs sized for `n` columns whatever C says"""

    def __init__(self, arena, n):
        self.arena, self.n = arena, n

    def __getattr__(self, name):
        return getattr(self.arena, name)

    def out(self, name, shape, dtype):
        shape = shape if isinstance(shape, tuple) else (shape,)
        return self.arena.out(name, (self.n,) + tuple(shape[1:]), dtype)


def test_python_layer_views():
    """chainstats.stats on tensors as they come: the sampler's layout with
    nskip and thin, a walker-major host array, a flat chain with a column
    subset; no copy of the device chain is made"""
    import torch
    from lfit_python_amd import chainstats
    x, _ = cd.shared(37, 6, 7)
    keys = ("n", "n_bad", "mean", "m2", "min", "max", "ostat", "quant")
    t = torch.as_tensor(np.array(x)).cuda()
    s = chainstats.stats(t, nskip=2, thin=3)
    cd.check({k: getattr(s, k) for k in keys}, cd.expected(x[2::3]), "nskip/thin")
    s = chainstats.stats(np.ascontiguousarray(x.transpose(1, 0, 2)), walker_major=True, rhat=True)
    cd.check({k: getattr(s, k) for k in keys}, cd.expected(x), "walker-major")
    flat = np.array(x.reshape(-1, 7))
    s = chainstats.stats(flat, cols=slice(1, 5), quantiles=(0.5,))
    cd.check({k: getattr(s, k) for k in keys}, cd.expected(x[:, :, 1:5], fracs=(0.5,)), "flat cols")
    assert np.allclose(s.std(1)[0], np.std(flat[:, 1], ddof=1), rtol=1e-12)


def test_wd_fluxes_match_the_host_route():
    from lfit_python_amd import chainstats, wdparams
    rng = np.random.default_rng(4)
    names = ["q", "wdFlux_g", "wdFlux_kg5", "wdFlux_r", "dphi"]
    flat = np.abs(rng.lognormal(-2.0, 0.3, size=(3000, 5)))
    got = chainstats.wd_fluxes(flat, names)
    want = wdparams.fluxes_from_chain(flat, names)
    assert [f.band for f in got] == [f.band for f in want] and len(got) == 2
    for a, b in zip(got, want):
        assert abs(a.flux - b.flux) <= 1e-14 * b.flux and abs(a.err - b.err) <= 1e-13 * b.err


def test_driver_summary(tmp_path):
    """mcmcfit.run(summary=True) summarises chain_dev: modparams.csv equals
    pandas' on the same chain; without it the driver's output is unchanged"""
    import pandas as pd
    from lfit_python_amd import chainstats, cvmodel, mcmcfit, sampler
    from tests.test_mcmcfit import _small_input
    said = []
    path = _small_input(tmp_path / "a")
    out = mcmcfit.run(path, chain_file=str(tmp_path / "a" / "chain_prod.txt"), seed=5, chunk=2, summary=True,
                      log=lambda *a: said.append(" ".join(map(str, a))))
    plain = mcmcfit.run(_small_input(tmp_path / "b"), chain_file=str(tmp_path / "b" / "chain_prod.txt"), seed=5,
                        chunk=2, log=lambda *a: None)
    assert "summary" not in plain and {k: v for k, v in out.items() if k not in ("summary", "chain_file")} == \
        {k: v for k, v in plain.items() if k != "chain_file"}
    assert open(out["chain_file"], "rb").read() == open(plain["chain_file"], "rb").read()
    summ = out["summary"]
    assert summ["modparams"] == str(tmp_path / "a" / "modparams.csv")
    names = cvmodel.construct_model(path).dynasty_par_names
    c = sampler.read_chain(out["chain_file"])                     # [W][steps][npars + 1], exact (repr round trip)
    data = pd.DataFrame(c[:, :, :-1].reshape(-1, len(names)), columns=names)
    got = pd.read_csv(summ["modparams"], index_col=0, float_precision="round_trip")
    assert list(got.index) == names and list(got.columns) == ["mean", "84th percentile", "16th percentile"]
    want = cd.expected(c[:, :, :-1].transpose(1, 0, 2), fracs=(0.16, 0.84))
    s = summ["stats"]
    cd.check({k: getattr(s, k) for k in ("n", "n_bad", "mean", "m2", "min", "max", "ostat", "quant")}, want, "driver")
    assert np.allclose(got["mean"], data.mean(), rtol=1e-13, atol=0)
    assert np.array_equal(got["84th percentile"].to_numpy(), s.quant[:, 1])
    assert np.all(np.abs(got["16th percentile"] - data.quantile(0.16)) <= 4 * cd.ulp(data.abs().max()))
    assert "Initial guess has a chisq of" in summ["initial_report"] and "D.o.F." in summ["initial_report"]
    assert "MCMC result has a chisq of" in summ["final_report"] and "a ln_prob of" in summ["final_report"]
    assert any("MCMC result has a chisq of" in line for line in said)
    assert summ["lnprob_mean"].shape == (5,) and np.allclose(summ["lnprob_mean"], c[:, :, -1].mean(axis=0), atol=1e-5)
    # the same numbers from the chain file through fit_summary (walker-major, a trailing ln_prob column)
    again = chainstats.fit_summary(c, names, out_dir=str(tmp_path / "b"), walker_major=True, log=lambda *a: None)
    other = pd.read_csv(again["modparams"], index_col=0, float_precision="round_trip")
    assert list(other.index) == names and np.allclose(other.to_numpy(), got.to_numpy(), rtol=1e-15, atol=0)
