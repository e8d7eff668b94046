"""GPU: k_pair LONG's closed-form and edge branches against the oracle.

tests/test_gpu_long.py runs the LONG path on one geometry (eclipse '0'), a
uniform phase grid and a constant error bar.  The cases here are built so
that windows of the classes of tests/long_windows.py occur in numbers
(tests/test_long_windows.py asserts the populations on the CPU, for the same
seeded walkers):

  spot_dense    windows narrower than the gaps between the spot's entries:
                quiet windows inside the spot's hull, 0 < E < 1 (and E = 1)
  beam_dark     tilt 175 deg: the beaming term never positive (LongB.any == 0)
  beam_lit      tilt 4 deg: never negative
  wrap_sub      windows that straddle +-0.5 with S = 3
  beam_cluster  windows on a beaming zero crossing (w = 0.002: those next to it
                hold a donor crossing and take the sub-bin loop too)
  beam_narrow   the same cluster at w = 0.0002: quiet windows next to the zero
                on either side, each walker's zero elsewhere among them
  wide_s1       S = 1 and w >= 0.0159: the closed form's wide-window
                Dirichlet branch (at S >= 2 no window that wide is quiet)
  simple_long   a 14-parameter eclipse on the LONG path (S = 3, and S = 1)
  tiny          fewer points than a wave, or than the eight waves
  mixed_tree    a LONG tree whose eclipses differ in length
  ragged_ye     error bars that differ per point

Every case: ln_prob and the per-eclipse ln-like against oracle.lnprob_batch at
LNP_RTOL.  The sharp variants shrink the error bars (and the noise) a
hundredfold, so that a flux error weighs a hundred times more; the bar is the
same.  build_case() needs no GPU (tools/quiet_count.py and the CPU tests use
it too).

Measured on an MI355X, worst |gpu - oracle| / |oracle| of the per-eclipse
ln-like over the walkers (ln_prob within 5 % of it, but for tiny_1 and tiny_2):
spot_dense 1.4e-11 (sharp 5.2e-11), beam_dark 3.4e-12 (sharp 4.9e-11),
beam_lit 4.7e-12 (sharp 4.6e-11), wrap_sub 4.2e-12 (sharp 2.8e-11),
beam_cluster 8.5e-13, beam_narrow 3.3e-12, wide_s1 1.4e-12, simple_long
3.0e-12 (S = 3), 2.5e-12 (S = 1), tiny_63 / 64 / 65 1.2e-11 to 1.7e-11,
tiny_513 3.9e-12, ragged_ye 1.9e-11, mixed_tree 3.0e-12.  tiny_1's one-point
ln-like differs by 1.7e-9 relative at worst, on the walker whose single
residual nearly vanishes (ln-like -9.7e-6: 1.6e-14 absolute), and tiny_2's
ln_prob by 2.1e-9 where prior and ln-like cancel to 0.0017 (3.5e-12 absolute):
rounding on small numbers.  The sharp variants sit where the kernels' flux parity
(1.9e-13) puts them, about 1e-10; no case came near LNP_RTOL.
"""
import ctypes
import zlib

import numpy as np
import pytest

from tests.test_gpu_lnprob import LNP_RTOL, _same
from tests.test_gpu_long import _walkers

pytestmark = pytest.mark.gpu

W = 48
WALKER_SEED = 7
CLASS_CASES = ("spot_dense", "beam_dark", "beam_lit", "wrap_sub", "beam_cluster", "beam_narrow", "wide_s1")
NSUB = {"spot_dense": 3, "beam_dark": 4, "beam_lit": 4, "wrap_sub": 3, "beam_cluster": 5, "beam_narrow": 5,
        "wide_s1": 1, "ragged_ye": 3, "simple_long_s3": 3, "simple_long_s1": 1, "tiny_1": 2, "tiny_2": 2,
        "tiny_63": 2, "tiny_64": 2, "tiny_65": 2, "tiny_513": 1}
_built = {}


def _tilted(tilt, nsub):
    """eclipse '0' at another tilt of the spot's beaming"""
    from lfit_python_amd import synthetic
    vals = list(synthetic._EVALS['0'][1])
    vals[synthetic._ENAMES.index('tilt')] = tilt
    band, p = synthetic.eclipse_param_strings('0', values=vals)
    return synthetic.build_tree([('0', band, p)], 300, True, None, nsub=nsub)


def _grid(oracle, name, m, rng):
    from lfit_python_amd.synthetic import phase_grid
    if name in ("spot_dense", "ragged_ye"):
        x = np.linspace(-0.03, 0.11, 600)
        return x, np.mean(np.diff(x)) * np.ones_like(x) / 2.0
    if name in ("beam_dark", "beam_lit"):
        return phase_grid(300)
    if name == "wrap_sub":
        x = np.concatenate([np.linspace(0.3, 1.1, 236), rng.uniform(0.49, 0.51, 64)])
        return x, np.concatenate([np.full(236, 0.8 / 235 / 2.0), np.full(64, 0.006)])
    if name in ("beam_cluster", "beam_narrow"):
        from tests.long_windows import Geometry
        x, w = phase_grid(300)
        g = Geometry(oracle, m.leaves()[0].cv_parlist)
        z = g.beam_zeros[np.argmin(np.abs(g.beam_zeros - 0.16))]
        assert abs(z - 0.16) < 0.01
        x = np.concatenate([x, z + g.phi0 + rng.uniform(-0.004, 0.004, 64)])
        return x, np.concatenate([w, np.full(64, 0.002 if name == "beam_cluster" else 0.0002)])
    if name == "simple_long_s3":
        return phase_grid(700)
    if name == "simple_long_s1":
        return phase_grid(600)
    if name == "wide_s1":
        return phase_grid(600)[0], 0.02 * rng.uniform(0.8, 1.5, 600)
    n = int(name.split("_")[1])  # tiny
    if n == 513:
        return phase_grid(513)
    x = np.array([0.01]) if n == 1 else np.linspace(-0.05, 0.08, n)
    return x, np.full(n, 0.001)


def _fill(oracle, leaf, x, w, ye, nsub, rng):
    lc = leaf.lc
    lc.x, lc.w, lc.ye = x, w, ye
    st, f = oracle.flux(leaf.cv_parlist, x, w, nsub=nsub)
    assert st == 0
    lc.y = f + ye * rng.standard_normal(f.shape)


def build_case(oracle, name, sharp=False):
    """(model, sub-bins) of a single-eclipse case: the light curve is the
    oracle's flux at the truth plus seeded noise of the error bars' size"""
    from lfit_python_amd import synthetic
    from lfit_python_amd.synthetic import NOISE
    if (name, sharp) in _built:
        return _built[name, sharp]
    nsub = NSUB[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in ("spot_dense", "ragged_ye"):
        m = synthetic.config_single(300, nsub=nsub, label='1')
    elif name in ("beam_dark", "beam_lit"):
        m = _tilted(175.0 if name == "beam_dark" else 4.0, nsub)
    elif name.startswith("simple_long"):
        m = synthetic.config_single(300, complex_bs=False, nsub=nsub)
    else:
        m = synthetic.config_single(300, nsub=nsub)
    x, w = _grid(oracle, name, m, rng)
    ye = NOISE * (rng.uniform(0.3, 3.0, x.size) if name == "ragged_ye" else np.ones_like(x))
    _fill(oracle, m.leaves()[0], x, w, ye / 100.0 if sharp else ye, nsub, rng)
    _built[name, sharp] = (m, nsub)
    return m, nsub


def case_walkers(m, nwalkers=W):
    return _walkers(m, nwalkers, WALKER_SEED)


def _check(oracle, m, nsub, nwalkers, tag):
    import torch
    from lfit_python_amd import _native, batch
    t = batch.compile_tree(m, nsub=nsub)
    ev = batch.LnProbEvaluator(t)
    assert _native.lib().lfg_layout(ctypes.byref(ev.ctree)) == 2
    walk = case_walkers(m, nwalkers)
    lle = torch.empty((nwalkers, t.E), dtype=torch.float64, device="cuda")
    got = ev(torch.as_tensor(walk, device="cuda"), lnlike_e=lle).cpu().numpy()
    lle = lle.cpu().numpy()
    ref, rlle, _ = oracle.lnprob_batch(walk, t, nsub=nsub)
    fin = np.isfinite(ref)
    if fin.any() and np.array_equal(np.isfinite(got), fin):
        print("\n%s: %d finite; worst |gpu - oracle| / |oracle|: ln_prob %.3e, ln-like per eclipse %.3e" % (
            tag, fin.sum(), np.max(np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])),
            np.max(np.abs(lle[fin] - rlle[fin]) / np.abs(rlle[fin]))))
    assert fin.sum() >= nwalkers // 2
    _same(lle[fin], rlle[fin], LNP_RTOL)
    _same(got, ref, LNP_RTOL)


SHARP = ("spot_dense", "beam_dark", "beam_lit", "wrap_sub")
CASES = [(n, False) for n in CLASS_CASES + ("simple_long_s3", "simple_long_s1", "tiny_1", "tiny_2", "tiny_63",
                                            "tiny_64", "tiny_65", "tiny_513", "ragged_ye")]
CASES += [(n, True) for n in SHARP]


@pytest.mark.parametrize("name,sharp", CASES, ids=["%s%s" % (n, "-sharp" if s else "") for n, s in CASES])
def test_long_edge_case_matches_oracle(oracle, name, sharp):
    m, nsub = build_case(oracle, name, sharp)
    _check(oracle, m, nsub, W, name + ("-sharp" if sharp else ""))


def test_long_mixed_tree_matches_oracle(oracle):
    """E = 3, S = 3, leaves of 1 500, 40 and 513 (shuffled) points: max_n sends
    the whole tree to LONG, the 40-point leaf leaves seven waves empty"""
    from lfit_python_amd import synthetic
    from lfit_python_amd.synthetic import NOISE, phase_grid
    rng = np.random.default_rng(31)
    m = synthetic.config_tree(1, 300, nsub=3)
    leaves = m.leaves()
    assert len(leaves) == 3
    for lf, n in zip(leaves, (1500, 40, 513)):
        x, w = phase_grid(n)
        if n == 513:
            p = rng.permutation(n)
            x, w = x[p], w[p]
        _fill(oracle, lf, x, w, NOISE * np.ones_like(x), 3, rng)
    _check(oracle, m, 3, 24, "mixed_tree")
