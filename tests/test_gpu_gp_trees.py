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


# ------------------------------------------------------------ the rule family
@pytest.fixture(scope="module")
def rule_cases(oracle):
    """case -> (tree, walkers, the double's dist_cp values, the host reference
    lnlike_e from the double's blocks, the oracle's ln_prob), once"""
    from lfit_python_amd import batch
    out = {}

    def get(name):
        if name not in out:
            m, walk = gp_trees.rule_case(oracle, name)
            t = batch.compile_tree(m)
            dcp = gp_trees.rule_dcp()
            lnp, _, _ = oracle.lnprob_batch(walk, t)
            out[name] = (t, walk, dcp, gp_trees.rule_reference(oracle, t, walk, dcp), lnp)
        return out[name]
    return get


@LAYOUTS
@pytest.mark.parametrize("name", gp_trees.RULE_CASES)
def test_gp_rule_edges(oracle, rule_cases, name, layout):
    """MODEL_SPEC 10.3's cache rule just either side of base / 2.2, above the
    base, with two parameters tripped, and the device's own dist_cp of every
    tripped walker, through lnlike_e: data sit 1e-8 .. 1e-4 either side of
    every edge the double's dist_cp gives (tests/gp_trees.py), so a dist_cp
    off by 1e-8 or the wrong side of the rule moves lnlike_e by 100 bars or
    more (tests/test_gp_trees.py::test_rule_case_is_sound).  rule_e3 goes
    through 7 walkers a call: 21 pairs, tripped and cached ones in one
    k_gp_dcp block, the last block partial."""
    import torch
    from lfit_python_amd import batch
    t, walk, dcp, ref, lnp_ref = rule_cases(name)
    ev = batch.LnProbEvaluator(t)
    assert (_layout_of(ev) != 0) == (layout == 1)
    k = gp_trees.RULE_CALL_W[name]
    lnp, lle = np.empty(len(walk)), np.empty((len(walk), t.E))
    for i in range(0, len(walk), k):
        l = torch.empty((len(walk[i:i + k]), t.E), dtype=torch.float64, device="cuda")
        lnp[i:i + k] = ev(torch.as_tensor(walk[i:i + k], device="cuda"), lnlike_e=l).cpu().numpy()
        lle[i:i + k] = l.cpu().numpy()
    fin = np.isfinite(lnp_ref)
    assert np.array_equal(np.isfinite(lnp), fin) and fin[:-1].all() and np.isneginf(lnp[-1])
    rel = np.abs(lle[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    for rname, r in zip(gp_trees.RULE_ROWS, rel):
        print("%s layout %d %-10s lnlike_e against the double's blocks: %.2e" % (name, layout, rname, r.max()))
    assert rel.max() <= GP_BAR, (name, layout, rel)
    _same(lnp, lnp_ref, LNP_RTOL)


def test_gp_rule_predict(oracle, rule_cases):
    """predict() on a tripped row and on the row just short of tripping: the
    smoother on the blocks the double's rule gives"""
    import torch
    from lfit_python_amd import batch
    t, walk, dcp, ref, lnp_ref = rule_cases("rule_e1")
    rows = [gp_trees.RULE_ROWS.index(n) for n in ("trip_rwd", "keep_rwd", "two")]
    ev = batch.LnProbEvaluator(t)
    pred = {k: v.cpu().numpy() for k, v in ev.predict(torch.as_tensor(walk[rows], device="cuda")).items()
            if k in ("flux", "gp_mean", "gp_var", "status")}
    assert (pred["status"] == 0).all()
    for j, i in enumerate(rows):
        st, flux = oracle.flux(gp_trees.eclipse_pars(t, 0, walk[i]), t.x, t.w)
        assert st == 0 and np.max(np.abs(pred["flux"][j] - flux)) <= 1e-9 * np.max(np.abs(flux))
        gs.check(pred["gp_mean"][j], pred["gp_var"][j], t.x, t.ye, t.y - pred["flux"][j],
                 gp_trees.hyper(t, 0, walk[i]), gp_trees.rule_blocks(t, 0, walk[i], dcp), t.x)
