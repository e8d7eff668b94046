"""The device's conditional GP draws (lfg_gp_sample, k_gp_smooth<true, false>;
MODEL_SPEC 10.5) against the host double of tests/gp_sample_double.py, draw
for draw, on the whole merged grid: the C ABI called directly through
gp._Merged + ctypes, out [W, S, n] compared at every point, data points
included.  tests/test_gp_sample_double.py holds the double itself to the dense
conditional and to normals computed by hand.

Bar: max |device - double| <= 1e-9 sqrt(ampin + ampout), the project's GP bar
(gs.BAR).  The two sides share no code: they differ by the roundings of log,
sincospi, exp and the recursions, which profiles/gp_sample_double/README.md
records at 1e-14 or below."""
import ctypes

import numpy as np
import pytest

from tests import gp_sample_double as gd
from tests import gp_smoother as gs

pytestmark = pytest.mark.gpu
BAR = gs.BAR


def device_draws(c):
    """lfg_gp_sample on a Call: (out [W, S, n], status [W]) as numpy"""
    import torch
    from lfit_python_amd import _native, gp
    L = _native.lib()
    g = gp._Merged(c.x, c.ye, c.res, c.hyp, c.blocks, c.t, None)
    # the grid the double works on is the grid the device is given
    assert g.W == c.W and g.n == c.n and g.nb == c.nb
    assert np.array_equal(g.x.cpu().numpy(), c.xm) and np.array_equal(g.obs.cpu().numpy(), c.obs)
    assert np.array_equal(g.ye.cpu().numpy(), c.yem) and np.array_equal(g.res.cpu().numpy(), c.rm, equal_nan=True)
    out = torch.full((c.W, c.S, c.n), -7.0, dtype=torch.float64, device=g.dev)
    nbytes = L.lfg_gp_sample_workspace_size(c.W, c.n, c.S)
    assert nbytes >= 8 * c.n * c.W * c.S * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g.dev)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())
    rc = L.lfg_gp_sample(*g.head(), c.S, c.seed, c.first, vp(out), vp(g.status), vp(ws), nbytes,
                         _native.stream_ptr(g.dev))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), g.status.cpu().numpy()


def worst(dev, dbl, c):
    """max over the call's vectors of |device - double| / sqrt(ampin + ampout)"""
    assert dev.shape == dbl.shape == (c.W, c.S, c.n)
    return max(np.max(np.abs(dev[w] - dbl[w])) / np.sqrt(c.scale(w)) for w in range(c.W))


@pytest.mark.parametrize("name", list(gd.CASES))
def test_draws_match_the_double(name):
    calls = gd.CASES[name]
    # wave_63_64_65's calls are heads of its last: one double serves the three
    shared = calls[-1].all_draws() if name == "wave_63_64_65" else None
    for c in calls:
        dev, st = device_draws(c)
        dbl = shared[:c.W] if shared is not None else c.all_draws()
        assert not st.any() and np.isfinite(dev).all()
        e = worst(dev, dbl, c)
        print("gp_sample_double %-16s n %3d W %2d S %2d first %10d: %.2e sqrt(ampin + ampout)"
              % (name, c.n, c.W, c.S, c.first, e))
        assert e <= BAR, (name, c.n, c.W, e)


def test_wrappers_select_and_shape():
    """gp.sample_conditional_batch and GP.sample_conditional on unsorted x and
    an unsorted t that repeats a phase: the draws at t, in t's order, and [M]
    for size == 1"""
    from lfit_python_amd import gp
    from tests.test_gpu_gp_predict import _gp_of
    x, ye, r, hyp, blocks, t = gs.make_case(21, 12, 2)
    t = np.concatenate([t[::-1], t[3:5], [x[2]]])
    assert np.any(np.diff(x) < 0) and np.any(np.diff(t) > 0) and np.any(np.diff(t) < 0)
    assert np.unique(t).size < t.size
    c = gd.Call(x, ye, r, hyp, blocks, t, 3, 2 ** 33 + 5, first=4)
    dbl = c.all_draws()
    scale = np.sqrt(c.scale(0))
    got = gp.sample_conditional_batch(x, ye, r[None], hyp[None], blocks[None], t, 3, seed=c.seed, first=4)
    assert got.shape == (1, 3, t.size)
    print("gp_sample_double wrappers: batch %.2e sqrt(ampin + ampout)" % (np.max(np.abs(got - dbl[:, :, c.it])) / scale))
    assert np.max(np.abs(got - dbl[:, :, c.it])) <= BAR * scale
    g = _gp_of(hyp, blocks)
    g.compute(x, ye)
    c0 = gd.Call(x, ye, r, hyp, blocks, t, 3, 77)
    many = g.sample_conditional(r, t, size=3, seed=77)
    assert many.shape == (3, t.size)
    assert np.max(np.abs(many - c0.draws(0)[:, c.it])) <= BAR * scale
    one = g.sample_conditional(r, t, size=1, seed=77)
    assert one.shape == (t.size,)
    assert np.max(np.abs(one - gd.Call(x, ye, r, hyp, blocks, t, 1, 77).draws(0)[0, c.it])) <= BAR * scale
    assert np.array_equal(one, many[0])        # draw 0 does not depend on S


def test_failures_stay_in_their_vector():
    """A NaN residual in vector 0 and tau = 0 in vector 2: their S rows are
    NaN and their status non-zero; vector 1's draws are the double's, and the
    bits of vector 1 sampled alone with first = 1"""
    base = gd.CASES["tile_31_32_33"][2]
    S = 4
    res = np.stack([base.res[0], base.res[0], base.res[0]])
    res[0, 5] = np.nan
    hyp = np.tile(base.hyp[0], (3, 1))
    hyp[2, 2] = 0.0
    blocks = np.tile(base.blocks[0], (3, 1, 1))
    c = gd.Call(base.x, base.ye, res, hyp, blocks, base.t, S, 31)
    dev, st = device_draws(c)
    assert st[0] != 0 and st[1] == 0 and st[2] != 0
    assert np.isnan(dev[0]).all() and np.isnan(dev[2]).all()
    e = np.max(np.abs(dev[1] - c.draws(1))) / np.sqrt(c.scale(1))
    print("gp_sample_double failures: healthy vector %.2e sqrt(ampin + ampout)" % e)
    assert e <= BAR, e
    alone, st1 = device_draws(gd.Call(base.x, base.ye, res[1], hyp[1], blocks[1], base.t, S, 31, first=1))
    assert st1[0] == 0 and np.array_equal(alone[0], dev[1])
