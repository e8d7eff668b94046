"""The host double of the prior lanes (tests/prior_double.py) against the
reference's own ln_prior, its golden prior values and the oracle's ln_prob,
and the construction of the edge cases tests/test_gpu_priors.py runs on the
device: everything the device is compared with is pinned here first."""
import json
import os

import numpy as np
import pytest

from lfit_python_amd import batch, cvmodel, synthetic
from lfit_python_amd.tree import Prior
from tests import prior_double as pd

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _same(a, b, rtol, atol=1e-13):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), np.nonzero(np.isfinite(a) != np.isfinite(b))
    assert np.all(np.isneginf(a[~np.isfinite(a)])) and np.all(np.isneginf(b[~np.isfinite(b)]))
    f = np.isfinite(a)
    np.testing.assert_allclose(a[f], b[f], rtol=rtol, atol=atol)


def _oracle_flux_fn(oracle):
    def flux_fn(p, x, w, nsub):
        st, f = oracle.flux(p, x, w, nsub=nsub)
        assert st == 0
        return f
    return flux_fn


@pytest.fixture(scope="module")
def single(oracle):
    m = synthetic.config_single(32, flux_fn=_oracle_flux_fn(oracle))
    return batch.compile_tree(m), np.array(m.dynasty_par_vals)


@pytest.fixture(scope="module")
def tree3(oracle):
    m = synthetic.config_tree(1, 32, flux_fn=_oracle_flux_fn(oracle))
    return batch.compile_tree(m), np.array(m.dynasty_par_vals)


@pytest.mark.parametrize("tag", ["tree", "simple", "gp"])
def test_ln_prior_matches_reference_tree(oracle, tag, tmp_path):
    """ln_prior of the reference's own trees on the golden walkers, at the
    tolerance test_lnprior_matches_reference holds the device to"""
    from tests.helpers import golden_tree
    if tag == "gp":
        d = np.load(os.path.join(GOLD, "lnprob_gp.npz"))
        m = cvmodel.construct_model(os.path.join(GOLD, "ref_test_data", "mcmc_input.dat"))
    else:
        d, m = golden_tree(tag, tmp_path)
    t = batch.compile_tree(m)
    got, parts = pd.ln_prior(oracle, t, d["walkers"])
    _same(got, d["ln_prior"], 1e-10)
    for w in np.nonzero(~np.isfinite(got))[0]:
        assert pd.rejected_by(parts, w), w


def test_ln_prior_matches_golden_prior_values(oracle, single):
    """every case of priors.json as a one-parameter prior table"""
    base, p0 = single
    g = json.load(open(os.path.join(GOLD, "priors.json")))
    seen = set()
    for case in g["cases"]:
        pr = Prior(case["type"], case["p1"], case["p2"])
        t = pd.table_tree(base, p0, [pr.code], [pr.p1], [pr.p2])
        got, _ = pd.ln_prior(oracle, t, np.array(case["vals"])[:, None])
        _same(got, case["ln_prob"], 1e-12)
        seen.add(pr.code)
    assert seen == set(range(5))


def test_roche_limit_walkers_are_clear_and_decide_ln_prob(oracle, single):
    """The Roche limit cases: none lies within the device / oracle agreement
    of its limit, both sides of every limit occur, and a finite oracle
    ln_prob is exactly a finite prior (the model fails for none of them)."""
    base, p0 = single
    t = pd.widen(base)
    names, walk = pd.roche_limit_walkers(oracle, t, p0)
    assert len(walk) <= 64
    ref, parts = pd.ln_prior(oracle, t, walk)
    pd.assert_clear_of_limits(parts, names)
    assert np.isfinite(ref[0])
    fin = dict(zip(names, np.isfinite(ref)))
    # each limit is decided by its own term alone: the two sides differ.  Below
    # q ~ 0.01 no disc radius passes both bspot and rdisc xl1 <= 0.46, so the
    # dphi limit cannot decide there (prior_double.roche_limit_walkers)
    undecided = {"dphi_mid0", "dphi_qlo", "dphi_below"}
    for n in names:
        if n.endswith("-") and n[:-1] + "+" in fin:
            if n[:-1] in undecided:
                assert not fin[n] and not fin[n[:-1] + "+"], n
            else:
                assert fin[n] != fin[n[:-1] + "+"], n
    assert fin["scale_hi="] and fin["scale_lo="]   # the inequalities are strict
    for k in ("dphi", "rdisc", "scale", "bspot", "az"):
        assert parts[k].any(), k
    lnp, _, _ = oracle.lnprob_batch(walk, t)
    model_fails = [n for n, a, b in zip(names, np.isfinite(ref), np.isfinite(lnp)) if a and not b]
    assert not np.any(np.isfinite(lnp) & ~np.isfinite(ref))
    assert model_fails == []


@pytest.mark.parametrize("case", pd.CHUNK_IDS)
def test_chunk_cases_are_balanced(oracle, single, case):
    base, p0 = single
    types, p1, p2, walk = pd.chunk_case(case)
    t = pd.table_tree(base, p0, types, p1, p2)
    ref, parts = pd.ln_prior(oracle, t, walk)
    pd.assert_chunk_case_balanced(types, walk, ref, parts)
    if case == "nd17":  # all-constant gather: the model is the truth's for every row
        lnp, _, _ = oracle.lnprob_batch(walk[:40], t)
        assert np.array_equal(np.isfinite(lnp), np.isfinite(ref[:40]))


def test_underflow_points_follow_the_rule(oracle, single):
    """MODEL_SPEC 8: a Gaussian term is finite while min(e, e - ln p2) lies
    above ln of half the smallest denormal, e = -z^2/2 - ln sqrt(2 pi).  No
    point lies within 1.0 of that threshold, but for (p2 = 100, z^2/2 = 740),
    0.39 below it: there the reference divides a pdf of 33 denormal units by
    100, which no rounding of the 33 brings up to the half unit that survives."""
    base, p0 = single
    types, p1, p2, walk, e = pd.underflow_case()
    t = pd.table_tree(base, p0, types, p1, p2)
    ref, parts = pd.ln_prior(oracle, t, walk)
    d = np.argmax(np.isfinite(e), 1)
    ee = e[np.arange(len(d)), d]
    key = np.minimum(ee, ee - np.log(p2[d]))
    ln_half_denorm = pd.LN_DENORM_MIN - np.log(2.0)
    assert abs(ln_half_denorm - (-745.1332191019412)) < 1e-12
    assert np.array_equal(np.isfinite(ref), key > ln_half_denorm)
    dist = np.abs(key - ln_half_denorm)
    near = dist < 1.0
    assert near.sum() == 2 and np.all(p2[d[near]] == 100.0) and np.all(dist[near] > 0.3)
    fin = np.isfinite(ref)
    assert 10 <= fin.sum() <= len(ref) - 10
    band = fin & (parts["box"][np.arange(len(d)), d] < pd.LN_NORMAL_MIN)
    assert band.sum() == pd.UNDERFLOW_BAND_ROWS
    # outside the band the reference's value is the exact e - ln p2 plus the other terms
    rest = np.array([parts["box"][w, np.arange(len(types)) != d[w]].sum() for w in range(len(ref))])
    np.testing.assert_allclose(ref[fin & ~band], (ee - np.log(p2[d]) + rest)[fin & ~band], rtol=1e-13)


def test_tree_attribution(oracle, tree3):
    """every Roche violation lands on its own eclipse, every box violation on
    its own parameter; ln_prob is finite exactly where the prior is"""
    base, p0 = tree3
    t = pd.widen(base)
    assert t.E == 3
    names, walk, where = pd.tree_attribution_walkers(oracle, t, p0)
    ref, parts = pd.ln_prior(oracle, t, walk)
    pd.assert_clear_of_limits(parts, names)
    assert np.isfinite(ref[0]) and (~np.isfinite(ref)).sum() >= 3 * 6 + 2
    for w, tgt in enumerate(where):
        rej = pd.rejected_by(parts, w)
        if tgt is None or np.isfinite(ref[w]):
            assert rej == [], (names[w], rej)
        else:
            assert rej == ["%s[%d]" % tgt], (names[w], rej)
    lnp, _, _ = oracle.lnprob_batch(walk, t)
    assert np.array_equal(np.isfinite(lnp), np.isfinite(ref))
    import dataclasses
    bad, _ = pd.ln_prior(oracle, dataclasses.replace(t, fixed_invalid=True), walk)
    assert np.all(np.isneginf(bad))
