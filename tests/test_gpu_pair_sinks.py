"""k_pair's sinks with merged run entries (LFG_PAIR_SINK_MERGE) against the
oracle, on window sets where the merged path and the path it falls back to
both run.

A solved element's run ends go into the LDS difference arrays with their
adjacent entries summed (lfg_sweep.hpp: apply_runs_merged) where no lane of
the wave has a run end of two windows or more; otherwise the wave runs
apply_runs_batched as before.  The per-pair constants of the sink (the disc
total's reciprocal, itwd, the two phase indices) are formed once, ahead of
the phase barrier.  The cases are where that code changes its shape:

    tiling grids of 2, 3, 4, 8 points   elements inside one window or across
                                        one join: no window covered whole
    tiling, 65 points                   two waves hold points; whole runs
    65 points with gaps (0.4)           an end may have no partial window
    65 and 300 points, overlap 3.5      run ends of 4 windows: the fallback
    65 points, zero widths              points: never partial
    65 points, widths 0.6 / 1.4         lo and hi stay sorted; ends of 1 or 2
    65 points within |phase| < 0.015    elements cover every window:
                                        P2 = 0, P3 = m, no entry at m

Each case: 8 walkers from the 1 % ball on config_single, ln_prob and the
per-eclipse ln_like through lfg_lnprob on both kernel layouts (the two-kernel
layout keeps apply_runs and is the control), against oracle.lnprob_batch at
LNP_RTOL.  The reference of a case is computed once and shared.  The first
test, which needs no GPU, checks cpu_baseline's port against the same
references: the inputs are sound before a GPU sees them."""
import numpy as np
import pytest

from tests.test_gpu_lnprob import LAYOUTS, LNP_RTOL, _same, layout  # noqa: F401  (fixture)

W = 8
CASES = [("tiling", 2), ("tiling", 3), ("tiling", 4), ("tiling", 8), ("tiling", 65),
         ("gaps", 65), ("overlap", 65), ("zero", 65), ("alternating", 65), ("overlap", 300), ("narrow", 65)]
IDS = ["%s-%d" % c for c in CASES]
_CASES = {}


def _windows(kind, n):
    from lfit_python_amd.synthetic import phase_grid
    x, w = phase_grid(n, -0.015, 0.015) if kind == "narrow" else phase_grid(n)
    if kind == "gaps":
        w = 0.4 * w
    elif kind == "overlap":
        w = 3.5 * w
    elif kind == "zero":
        w = np.zeros_like(w)
    elif kind == "alternating":
        w = w * np.where(np.arange(n) % 2 == 0, 0.6, 1.4)
    return x, w


def _case(key, oracle):
    """(tree, walkers, oracle ln_prob, oracle ln_like per eclipse) of a case"""
    if key not in _CASES:
        from lfit_python_amd import batch, synthetic
        from lfit_python_amd.synthetic import NOISE
        kind, n = key
        m = synthetic.config_single(300)
        leaf = m.leaves()[0]
        x, w = _windows(kind, n)
        leaf.lc.x, leaf.lc.w = x, w
        leaf.lc.ye = NOISE * np.ones_like(x)
        st, f = oracle.flux(leaf.cv_parlist, x, w)
        assert st == 0
        leaf.lc.y = f + NOISE * np.random.default_rng(3).standard_normal(f.shape)
        t = batch.compile_tree(m)
        p0 = np.array(m.dynasty_par_vals)
        walk = p0 * (1.0 + 0.01 * np.random.default_rng(23).standard_normal((W, p0.size)))
        ref, rlle, _ = oracle.lnprob_batch(walk, t)
        assert np.all(np.isfinite(ref))
        _CASES[key] = (t, walk, ref, rlle)
    return _CASES[key]


@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    return cpu.CpuPort(cpu.build(out=str(tmp_path_factory.mktemp("cpu") / "liblfg_cpu.so")))


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_cpu_port_meets_the_oracle_on_the_case(oracle, port, key):
    t, walk, ref, _ = _case(key, oracle)
    _same(port.lnprob_batch(walk, t)[0], ref, LNP_RTOL)


@pytest.mark.gpu
@LAYOUTS
@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_pair_sinks_match_oracle(oracle, key, layout):
    import ctypes
    import torch
    from lfit_python_amd import _native, batch
    t, walk, ref, rlle = _case(key, oracle)
    ev = batch.LnProbEvaluator(t)
    assert _native.lib().lfg_layout(ctypes.byref(ev.ctree)) == layout   # the tree takes the layout under test
    lle = torch.empty((W, t.E), dtype=torch.float64, device="cuda")
    got = ev(torch.as_tensor(walk, device="cuda"), lnlike_e=lle).cpu().numpy()
    _same(got, ref, LNP_RTOL)
    _same(lle.cpu().numpy(), rlle, LNP_RTOL)
