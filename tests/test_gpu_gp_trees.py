"""GPU: the GP likelihood of a tree (k_pair<true> or k_lnlike<2, .>, k_gp_dcp,
k_gp_like) on the synthetic trees of tests/gp_trees.py, against the oracle's
dense Cholesky likelihood: fewer points than k_gp_like has segments, a
segment cut on a block's first point, tied phases, three blocks, eclipses
over one tile, sub-bins, one eclipse per walker, a lone pair.

A case's walkers go through in chunks of gp_trees.CALL_W[case] per call, so
that the launch has the case's walker count while every case holds its five
designated rows (tests/gp_trees.py)."""
import ctypes

import numpy as np
import pytest

from tests import gp_smoother as gs
from tests import gp_trees
from tests.test_gpu_lnprob import LAYOUTS, LNP_RTOL, _same, layout  # noqa: F401  (layout: the fixture)

pytestmark = pytest.mark.gpu
GP_BAR = 1e-9   # the project's GP bar, relative to max(1, |ref|); tests/gp_trees.py says what it rests on here


@pytest.fixture(scope="module")
def cases(oracle):
    """case -> (tree, nsub, walkers, the oracle's ln_prob and lnlike_e), once"""
    from lfit_python_amd import batch
    out = {}

    def get(name):
        if name not in out:
            m, nsub, walk = gp_trees.case(oracle, name)
            t = batch.compile_tree(m, nsub=nsub)
            ref, lle, _ = oracle.lnprob_batch(walk, t, nsub=nsub)
            gp_trees.check_case(name, walk, ref)
            out[name] = (m, t, nsub, walk, ref, lle)
        return out[name]
    return get


def _layout_of(ev):
    from lfit_python_amd import _native
    return _native.lib().lfg_layout(ctypes.byref(ev.ctree))


def _lnprob(ev, name, walk):
    """ln_prob [W] and lnlike_e [W, E], CALL_W[name] walkers per call"""
    import torch
    E = ev.tree.E
    lnp, lle = np.empty(len(walk)), np.empty((len(walk), E))
    for sl in gp_trees.chunks(name, len(walk)):
        l = torch.empty((sl.stop - sl.start, E), dtype=torch.float64, device="cuda")
        lnp[sl] = ev(torch.as_tensor(walk[sl], device="cuda"), lnlike_e=l).cpu().numpy()
        lle[sl] = l.cpu().numpy()
    return lnp, lle


def _predict(ev, name, walk):
    import torch
    parts = [ev.predict(torch.as_tensor(walk[sl], device="cuda")) for sl in gp_trees.chunks(name, len(walk))]
    return {k: np.concatenate([p[k].cpu().numpy() for p in parts]) for k in ("flux", "gp_mean", "gp_var", "status")}


@pytest.fixture(scope="module")
def runs(cases):
    """case -> (ln_prob, lnlike_e, predict's arrays) on the default layout, once"""
    from lfit_python_amd import batch
    out = {}

    def get(name):
        if name not in out:
            m, t, nsub, walk, ref, lle = cases(name)
            ev = batch.LnProbEvaluator(t)
            out[name] = _lnprob(ev, name, walk) + (_predict(ev, name, walk),)
        return out[name]
    return get


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if np.size(a) else 0.0


@LAYOUTS
@pytest.mark.parametrize("name", gp_trees.CASES)
def test_gp_tree_matches_oracle(cases, name, layout):
    from lfit_python_amd import batch
    m, t, nsub, walk, ref, lle_ref = cases(name)
    ev = batch.LnProbEvaluator(t)
    # the routing is part of the contract
    assert _layout_of(ev) == (0 if name in gp_trees.TWO_KERNEL else layout)
    got, lle = _lnprob(ev, name, walk)
    fin = np.isfinite(ref)
    print("%s layout %d (kernels %d): ln_prob %.2e, lnlike_e %.2e relative to max(1, |ref|); %d of %d finite"
          % (name, layout, _layout_of(ev), _rel(got[fin], ref[fin]), _rel(lle[fin], lle_ref[fin]), fin.sum(),
             len(ref)))
    _same(got, ref, LNP_RTOL)
    assert np.all(np.isfinite(lle_ref[fin]))
    _same(lle[fin], lle_ref[fin], LNP_RTOL)


@pytest.mark.parametrize("name", gp_trees.CASES)
def test_gp_filter_alone(oracle, cases, runs, name):
    """The likelihood kernels fed their own residuals: tree.y - predict()'s
    flux through the dense oracle with the oracle's blocks, so that flux
    parity is out of the comparison."""
    m, t, nsub, walk, ref, lle_ref = cases(name)
    got, lle, pred = runs(name)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(pred["status"] == 0, fin)
    worst = 0.0
    for i in np.flatnonzero(fin):
        for e in range(t.E):
            sl = slice(t.offsets[e], t.offsets[e + 1])
            res = t.y[sl] - pred["flux"][i, sl]
            want = oracle.gp_lnlike(t.x[sl], res, t.ye[sl], *gp_trees.hyper(t, e, walk[i]),
                                    gp_trees.blocks(oracle, t, e, walk[i]))
            err = abs(lle[i, e] - want) / max(1.0, abs(want))
            worst = max(worst, err)
            assert err <= GP_BAR, (name, i, e, lle[i, e], want, err)
    print("%s: k_gp_like on its own residuals, largest error %.2e relative to max(1, |ref|)" % (name, worst))


@pytest.mark.parametrize("name", ["cycles", "subbin"])
def test_gp_tree_predict(oracle, cases, runs, name):
    """k_gp_smooth_tree on residuals and block indices that k_lnlike<2, .>
    wrote across tiles and with sub-bins, against the dense conditional."""
    m, t, nsub, walk, ref, lle_ref = cases(name)
    got, lle, pred = runs(name)
    fin = np.isfinite(ref)
    assert np.array_equal(pred["status"] == 0, fin)
    for k in ("flux", "gp_mean", "gp_var"):
        assert pred[k].shape == (len(walk), t.offsets[-1])
        assert np.isnan(pred[k][~fin]).all() and np.isfinite(pred[k][fin]).all()
    for i in np.flatnonzero(fin):
        for e in range(t.E):
            sl = slice(t.offsets[e], t.offsets[e + 1])
            st, flux = oracle.flux(gp_trees.eclipse_pars(t, e, walk[i]), t.x[sl], t.w[sl], nsub=nsub)
            assert st == 0
            assert np.max(np.abs(pred["flux"][i, sl] - flux)) <= 1e-9 * np.max(np.abs(flux)), (i, e)
            res = t.y[sl] - pred["flux"][i, sl]   # the flux just checked: the smoother's own input
            gs.check(pred["gp_mean"][i, sl], pred["gp_var"][i, sl], t.x[sl], t.ye[sl], res,
                     gp_trees.hyper(t, e, walk[i]), gp_trees.blocks(oracle, t, e, walk[i]), t.x[sl])


@LAYOUTS
def test_gp_tree_e1_spec_chain(cases, layout):
    """One eclipse per walker: k_gp_like itself runs combine_walker and the
    stretch move's acceptance.  The speculative half-step equals the plain
    one bit for bit, and the stored ln_prob is the ln_prob of the stored
    positions, bit for bit."""
    import torch
    from lfit_python_amd import batch, sampler
    m, t, nsub, walk, ref, lle_ref = cases("cuts")
    assert t.E == 1
    ev = batch.LnProbEvaluator(t)
    assert _layout_of(ev) == layout
    p0 = np.array(m.dynasty_par_vals)
    W = 2 * len(p0) + 2
    init = sampler.initialise_walkers(p0, sampler.comp_scatter(m.dynasty_par_names, 0.1), W,
                                      lambda p: ev(torch.as_tensor(p, device="cuda")).cpu().numpy())
    out = []
    for spec in (False, True):
        S = sampler.EnsembleSampler(W, t.ndim, ev, seed=9)
        S.spec = spec
        S.run_mcmc(init, 3)
        out.append((S.chain_dev.cpu().numpy(), S.lnprob_dev.cpu().numpy(), S.naccept.cpu().numpy()))
        again = ev(S.chain_dev[-1].contiguous()).cpu().numpy()
        np.testing.assert_array_equal(again, out[-1][1][-1])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(out[0][1])) and out[0][2].sum() > 0   # moves were accepted: the acceptance ran
