"""GPU: the prior lanes of k_setup (prior_lane, bspot_lane and the setup
lane's Roche checks in lfg_k_setup.hpp: setup_any) at every prior's edges, per prior type,
against the host double tests/prior_double.py, which tests/test_prior_double.py
pins against the reference's own ln_prior first.

Every case goes through lfg_lnprior twice: as LnProbEvaluator builds the tree
(prior_c set: the chunked formula, one log per 16 parameters) and with
prior_c = NULL (each term from prior_lnprob, include/lfg.h).  Finiteness is
exact; values at rtol 1e-13, atol 1e-11, what
test_gpu_lnprob.test_lnprior_tiny_log_uniform_products holds the same lanes
to.  The Roche cases sit 100x or more outside the agreement the suite pins
between the device's and the oracle's primitives (prior_double.MARGIN)."""
import ctypes
import dataclasses
import json
import os

import numpy as np
import pytest

from tests import prior_double as pd
from tests.test_gpu_lnprob import LAYOUTS, LNP_RTOL, _flux_fn, layout  # noqa: F401 (layout: a fixture)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
RTOL, ATOL = 1e-13, 1e-11


def _device(tree, walkers, no_types=False):
    """lfg_lnprior of the walkers with prior_c set and with prior_c = NULL"""
    import torch
    from lfit_python_amd import batch
    ev = batch.LnProbEvaluator(tree)
    if no_types:
        ev.ctree.prior_type = None
    x = torch.as_tensor(np.ascontiguousarray(walkers), device="cuda")
    with_c = ev.ln_prior(x).cpu().numpy()
    ev.ctree.prior_c = None
    return with_c, ev.ln_prior(x).cpu().numpy()


def _check(got, ref, names=None, band=None, label=""):
    """same finiteness (-inf, never NaN or +inf) as the reference; its values
    outside `band`"""
    got, ref = np.asarray(got), np.asarray(ref)
    fg, fr = np.isfinite(got), np.isfinite(ref)
    wrong = np.nonzero(fg != fr)[0]
    assert wrong.size == 0, (label, wrong[:10], [names[w] for w in wrong[:10]] if names else None,
                             got[wrong[:10]], ref[wrong[:10]])
    assert np.all(np.isneginf(got[~fg])), label
    cmp = fr if band is None else fr & ~band
    np.testing.assert_allclose(got[cmp], ref[cmp], rtol=RTOL, atol=ATOL, err_msg=label)


def _check_both(tree, walkers, ref, names=None, band=None, no_types=False):
    with_c, null_c = _device(tree, walkers, no_types)
    _check(with_c, ref, names, band, "prior_c")
    _check(null_c, ref, names, band, "prior_c = NULL")
    both = np.isfinite(with_c) & np.isfinite(null_c)
    if band is not None:
        both &= ~band
    np.testing.assert_allclose(with_c[both], null_c[both], rtol=RTOL, atol=ATOL)
    return with_c, null_c


@pytest.fixture(scope="module")
def single():
    from lfit_python_amd import batch, synthetic
    m = synthetic.config_single(32, flux_fn=_flux_fn)
    return batch.compile_tree(m), np.array(m.dynasty_par_vals)


@pytest.fixture(scope="module")
def roche_single(oracle, single):
    """the one-eclipse tree with widened boxes, the Roche limit walkers and
    their reference (computed once, shared, left unchanged)"""
    t = pd.widen(single[0])
    names, walk = pd.roche_limit_walkers(oracle, t, single[1])
    ref, parts = pd.ln_prior(oracle, t, walk)
    pd.assert_clear_of_limits(parts, names)
    lnp, _, _ = oracle.lnprob_batch(walk, t)
    return t, names, walk, ref, parts, lnp


# ------------------------------------------------- a. golden edge values, every type
def test_golden_prior_values_on_the_device(single):
    """Every case of tests/golden/priors.json (the reference's own
    Prior.ln_prob at its edges) as a one-parameter prior table: the first
    device evaluation of gaussPos, and of every type through prior_lnprob."""
    from lfit_python_amd.tree import Prior
    base, p0 = single
    g = json.load(open(os.path.join(GOLD, "priors.json")))
    seen = set()
    for case in g["cases"]:
        pr = Prior(case["type"], case["p1"], case["p2"])
        t = pd.table_tree(base, p0, [pr.code], [pr.p1], [pr.p2])
        ref = np.array(case["ln_prob"], np.float64)
        assert ref.min() == -np.inf and (np.isfinite(ref) & (ref < pd.LN_NORMAL_MIN)).sum() == 0
        _check_both(t, np.array(case["vals"])[:, None], ref, names=case["vals"])
        seen.add(pr.code)
    assert seen == set(range(5))


# ------------------------------------------------------------ b. chunk and lane edges
@pytest.mark.parametrize("case", pd.CHUNK_IDS)
def test_chunk_and_lane_edges(oracle, single, case):
    """ndim around the chunks of 16 parameters, the five types mixed in every
    chunk (and 16 log_uniform / 16 gauss in one), every dimension at every edge
    of its type; W = 1, 5, 64, 257 and the whole set (k_setup's lane bounds)."""
    base, p0 = single
    types, p1, p2, walk = pd.chunk_case(case)
    t = pd.table_tree(base, p0, types, p1, p2)
    ref, parts = pd.ln_prior(oracle, t, walk)
    pd.assert_chunk_case_balanced(types, walk, ref, parts)
    # no finite term of these tables is a denormal pdf: every value is compared
    assert not (np.isfinite(parts["box"]) & (parts["box"] < pd.LN_NORMAL_MIN)).any()
    for W in pd.LANE_W + (len(walk),):
        W = min(W, len(walk))
        _check_both(t, walk[:W], ref[:W])


# --------------------------------------------------- 3. the Gaussian underflow rule
def test_gaussian_underflow_rule(oracle, single):
    """MODEL_SPEC 8: a gauss / gaussPos term is -inf once exp(-z^2/2)/sqrt(2 pi)
    or its quotient by p2 underflows, on both device paths, for p2 below and
    above 1.  Values are compared where the reference's pdf is a normal
    number; where it is a denormal (UNDERFLOW_BAND_ROWS deliberately placed
    rows) the reference's log(pdf) is coarse and only finiteness is."""
    base, p0 = single
    types, p1, p2, walk, e = pd.underflow_case()
    t = pd.table_tree(base, p0, types, p1, p2)
    ref, parts = pd.ln_prior(oracle, t, walk)
    d = np.argmax(np.isfinite(e), 1)
    term = parts["box"][np.arange(len(d)), d]
    band = np.isfinite(term) & (term < pd.LN_NORMAL_MIN)
    assert band.sum() == pd.UNDERFLOW_BAND_ROWS
    fin = np.isfinite(ref)
    assert 10 <= fin.sum() <= len(ref) - 10
    # the distance of every point from the rule's threshold: tests/test_prior_double.py
    names = ["p2=%g z2/2=%g" % (p2[k], -e[w, k] - pd.LN_SQRT_2PI) for w, k in enumerate(d)]
    _check_both(t, walk, ref, names=names, band=band)


# ------------------------------------------------------ c. Roche priors at their limits
def test_roche_priors_at_their_limits(roche_single):
    """rdisc xl1 = 0.46, scale = 3 rwd and rwd / 3 (and the exact doubles, which
    pass), the azimuth window, dphi = findphi(q, 90) - 1e-6 across the q table
    (patch middles, patch boundaries, its ends) and through the solver beyond
    it, q <= 0 and non-finite, and a failing bspot: the reference decides the
    side of each."""
    t, names, walk, ref, parts, _ = roche_single
    fin = np.isfinite(ref)
    assert fin.sum() >= 20 and (~fin).sum() >= 20
    _check_both(t, walk, ref, names=names)


# --------------------------------------------------------- d. attribution in a tree
def test_tree_attribution(oracle):
    """E = 3: a Roche violation in one eclipse, a box violation in a band-level
    or an eclipse-level parameter reject exactly their own walkers; an invalid
    fixed parameter rejects all."""
    from lfit_python_amd import batch, synthetic
    m = synthetic.config_tree(1, 32)   # ln_prior alone: the light curves are not read
    t = pd.widen(batch.compile_tree(m))
    assert t.E == 3
    names, walk, where = pd.tree_attribution_walkers(oracle, t, np.array(m.dynasty_par_vals))
    ref, parts = pd.ln_prior(oracle, t, walk)
    pd.assert_clear_of_limits(parts, names)
    for w, tgt in enumerate(where):
        want = [] if tgt is None or np.isfinite(ref[w]) else ["%s[%d]" % tgt]
        assert pd.rejected_by(parts, w) == want, names[w]
    assert np.isfinite(ref[0]) and (~np.isfinite(ref)).sum() >= 3 * 6 + 2
    _check_both(t, walk, ref, names=names)
    bad = dataclasses.replace(t, fixed_invalid=True)
    for got in _device(bad, walk):
        assert np.all(np.isneginf(got))


# ------------------------------------------------------------------- e. no priors
def test_no_prior_table(oracle, roche_single):
    """prior_type = NULL: exactly 0.0 without the Roche priors, the Roche terms
    alone with them"""
    t, names, walk, _, _, _ = roche_single
    keep = np.isfinite(walk).all(1)      # without a box prior nothing but the Roche terms sees a NaN
    walk, names = walk[keep], [n for n, k in zip(names, keep) if k]
    bare = dataclasses.replace(t, prior_type=None)
    for got in _device(dataclasses.replace(t, roche_priors=False), walk, no_types=True):
        assert np.all(got == 0.0) and not np.any(np.signbit(got))
    ref, _ = pd.ln_prior(oracle, bare, walk)
    assert set(ref) == {0.0, -np.inf}
    with_c, null_c = _check_both(t, walk, ref, names=names, no_types=True)
    assert np.all(with_c[np.isfinite(ref)] == 0.0)


# --------------------------------------- f. the prior decides ln_prob on every layout
def _lnprob_follows_prior(tree, walk, names, prior, lnp_ref, want_layout):
    import torch
    from lfit_python_amd import _native, batch
    ev = batch.LnProbEvaluator(tree)
    assert _native.lib().lfg_layout(ctypes.byref(ev.ctree)) == want_layout
    got = ev(torch.as_tensor(walk, device="cuda")).cpu().numpy()
    fg, fr = np.isfinite(got), np.isfinite(lnp_ref)
    assert not np.any(fr & ~np.isfinite(prior))          # a finite ln_prob has a finite prior
    wrong = np.nonzero(fg != fr)[0]
    assert wrong.size == 0, ([names[w] for w in wrong], got[wrong], lnp_ref[wrong])
    assert np.all(np.isneginf(got[~fg]))
    assert fr.sum() >= 20 and (~fr).sum() >= 20
    np.testing.assert_allclose(got[fr], lnp_ref[fr], rtol=LNP_RTOL, atol=1e-9)


@LAYOUTS
def test_prior_decides_lnprob(roche_single, layout):
    """the Roche limit walkers through lfg_lnprob: -inf exactly where the
    reference prior is -inf or the oracle's model fails (prior_rejects in
    k_pair, and in k_elements + k_lnlike), the oracle's ln_prob elsewhere.
    The walkers at q = 3.4, 5 and 6 (i = 89.9 degrees) are where the oracle's
    ray minimum once stopped at the start of the chord (MODEL_SPEC 4.2).
    At the walker dphi_above- (q = 6) oracle and device both once had the
    egress of two elements of the outermost disc ring 2.3e-4 early in phase,
    the same way, so this comparison could not see it; the arbiter of
    tests/contact_double.py decided, and ln_prob there moved by 1.2e-7."""
    t, names, walk, ref, _, lnp = roche_single
    _lnprob_follows_prior(t, walk, names, ref, lnp, layout)


def test_prior_decides_lnprob_long(oracle, single):
    """the same on a 600-point eclipse (k_pair's LONG variant)"""
    from lfit_python_amd import batch, synthetic
    m = synthetic.config_single(600, flux_fn=_flux_fn)
    t = pd.widen(batch.compile_tree(m))
    names, walk = pd.roche_limit_walkers(oracle, t, np.array(m.dynasty_par_vals))
    assert len(walk) <= 64
    ref, _ = pd.ln_prior(oracle, t, walk)
    lnp, _, _ = oracle.lnprob_batch(walk, t)
    _lnprob_follows_prior(t, walk, names, ref, lnp, 2)
