"""The synthetic GP trees of tests/gp_trees.py on the CPU: the cases are sound
(finite shares, designated rows, no datum on a changepoint) and the host
port's serial Kalman filter (cpu_baseline) agrees with the oracle's dense GP
likelihood on every one of them, at test_port_gp_tree_matches_reference's bar."""
import numpy as np
import pytest

from lfit_python_amd import batch
from tests import gp_trees


@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    path = cpu.build(out=str(tmp_path_factory.mktemp("cpu") / "liblfg_cpu.so"))
    return cpu.CpuPort(path)


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}

    def get(name):
        if name not in out:
            m, nsub, walk = gp_trees.case(oracle, name)
            t = batch.compile_tree(m, nsub=nsub)
            ref, lle, _ = oracle.lnprob_batch(walk, t, nsub=nsub, nthreads=4)
            out[name] = (t, nsub, walk, ref, lle)
        return out[name]
    return get


@pytest.mark.parametrize("name", gp_trees.CASES)
def test_case_is_sound(oracle, cases, name):
    t, nsub, walk, ref, lle = cases(name)
    assert t.gp and t.nsub == nsub and len(walk) == gp_trees.TOTAL_W[name]
    gp_trees.check_case(name, walk, ref)
    for e in range(t.E):
        assert np.all(np.diff(t.x[t.offsets[e]:t.offsets[e + 1]]) >= 0)
    assert gp_trees.edge_clearance(oracle, t, walk) >= 0.99 * gp_trees.EDGE_GAP
    n = np.diff(t.offsets)
    shape = {"tiny": [1, 2, 7, 9], "cuts": [64], "seam": [513, 40], "cycles": [1100], "subbin": [300, 600],
             "sharp": [64], "one": [64]}[name]
    assert list(n) == shape
    if name != "tiny":   # (a handful of points need not straddle phase 0: one block, or two)
        assert [tuple(g) for g in t.gp_ecl] == [(0, 2) if name == "cycles" else (0, 1)] * t.E
    if name in ("cuts", "sharp", "one"):
        # block 1 opens on point 32, a segment's first point, for every walker
        # on the cached dist_cp; ties across the cut at 40
        for i in (gp_trees.ROW_HYPER, gp_trees.ROW_OUT, 5):
            b = gp_trees.blocks(oracle, t, 0, walk[i])
            assert t.x[31] < b[1, 0] < t.x[32] and abs(t.x[32] - b[1, 0]) < 1.01 * gp_trees.EDGE_GAP
            assert t.x[12] < b[0, 1] < t.x[13] and t.x[13] - t.x[12] < 2.02 * gp_trees.EDGE_GAP
        assert t.x[39] == t.x[40] == t.x[41]
        assert 'phi0_0' not in t.names
    # the rows that trip the cache rule get blocks of their own
    base = gp_trees.blocks(oracle, t, 0, walk[gp_trees.ROW_HYPER])
    for row in (gp_trees.ROW_DPHI, gp_trees.ROW_Q, gp_trees.ROW_RWD):
        assert np.max(np.abs(gp_trees.blocks(oracle, t, 0, walk[row]) - base)) > 1e-4


@pytest.mark.parametrize("name", gp_trees.CASES)
def test_port_matches_oracle_on_gp_trees(oracle, port, cases, name):
    t, nsub, walk, ref, lle = cases(name)
    got, _ = port.lnprob_batch(walk, t, nthreads=4)
    assert np.array_equal(np.isfinite(got), np.isfinite(ref))
    gp_trees.check_case(name, walk, got)
    fin = np.isfinite(ref)
    err = np.max(np.abs(got[fin] - ref[fin]) / np.abs(ref[fin]))
    print("%s: port against oracle, largest relative error %.2e, %d of %d finite" % (name, err, fin.sum(), len(ref)))
    np.testing.assert_allclose(got[fin], ref[fin], rtol=1e-9)


def test_filter_restatements_on_cuts(oracle, cases):
    """The segment form of tests/gp_kalman.py (8 segments, k_gp_like's) on the
    oracle's own residuals of the cuts tree: a segment cut on a block's first
    point, ties across a cut, points 1e-7 either side of an edge."""
    from tests.gp_kalman import gp_lnlike_kalman_jordan, gp_lnlike_segments
    t, nsub, walk, ref, lle = cases("cuts")
    for i in np.flatnonzero(np.isfinite(ref)):
        p = gp_trees.eclipse_pars(t, 0, walk[i])
        st, f = oracle.flux(p, t.x, t.w, nsub=nsub)
        assert st == 0
        args = (t.x, t.y - f, t.ye, *gp_trees.hyper(t, 0, walk[i]), gp_trees.blocks(oracle, t, 0, walk[i]))
        dense = oracle.gp_lnlike(*args)
        assert abs(dense - lle[i, 0]) <= 1e-12 * abs(dense)
        for got in (gp_lnlike_kalman_jordan(*args), gp_lnlike_segments(*args, K=8)):
            assert abs(dense - got) <= 1e-10 * max(1.0, abs(dense)), (i, dense, got)


# ------------------------------------------------------------ the rule family
RULE_BAR = 1e-9          # tests/test_gpu_gp_trees.py's GP_BAR
EDGE_MOVE = 1.5e-8       # past the ladder's smallest rung


@pytest.fixture(scope="module")
def rule_cases(oracle):
    out = {}

    def get(name):
        if name not in out:
            m, walk = gp_trees.rule_case(oracle, name)
            t = batch.compile_tree(m)
            dcp = gp_trees.rule_dcp()
            out[name] = (t, walk, dcp, gp_trees.rule_reference(oracle, t, walk, dcp))
        return out[name]
    return get


def _moved(which, sign):
    """rule_blocks with one edge of the data's two (0: -dcp + phi0, block 0's
    end; 1: dcp + phi0, block 1's start) moved by sign * EDGE_MOVE"""
    def fn(tree, e, v, dcp):
        b = gp_trees.rule_blocks(tree, e, v, dcp)
        b[which, 1 - which] += sign * EDGE_MOVE
        return b
    return fn


@pytest.mark.parametrize("name", gp_trees.RULE_CASES)
def test_rule_case_is_sound(oracle, rule_cases, name):
    """The conditions on the rule family, on the reference alone: the rows
    trip or keep the rule as designated, and every finite row's lnlike_e
    moves by at least 100 bars when any edge inside its data moves past the
    ladder's first rung, in either direction; a row just short of tripping
    evaluated at its own dist_cp instead of the cache's misses by as much."""
    from tests import wdphases_double as wd
    t, walk, dcp, ref = rule_cases(name)
    rows = gp_trees.RULE_ROWS
    assert t.gp and len(walk) == len(rows) == 12 and t.E == len(gp_trees.RULE_LEAVES[name])
    assert [tuple(g) for g in t.gp_ecl] == [(0, 1)] * t.E
    lnp, _, _ = oracle.lnprob_batch(walk, t, nthreads=4)
    fin = np.isfinite(lnp)
    # check_case's finite-share rule, the designated rows
    assert 4 * fin.sum() >= 3 * len(lnp) and fin[:-1].all() and np.isneginf(lnp[rows.index("out")])
    assert np.isfinite(ref[:-1]).all()
    base = tuple(t.gp_base[0, :3]) + (dcp["base"],)
    for i, rname in enumerate(rows):
        p = gp_trees.eclipse_pars(t, 0, walk[i])
        trip = wd.tripped(base, p[4], p[5], p[8])
        assert trip == (rname in gp_trees.RULE_TRIPPED), rname
        # no row within 1e-6 relative of the threshold v = B / 2.2
        for B, v in zip(base[:3], (p[4], p[5], p[8])):
            assert abs(abs(B - v) / v - wd.RULE) > 1e-6 * wd.RULE, rname
        if rname.startswith("high_"):
            assert max(p[4] / base[0], p[5] / base[1], p[8] / base[2]) > 1.5
    # every tripped row has a dist_cp of its own, well away from the cache's and from each other's
    own = sorted(dcp[n] for n in ("base",) + gp_trees.RULE_TRIPPED)
    assert np.min(np.diff(own)) > 3e-4
    worst = np.inf
    for which in (0, 1):
        for sign in (-1.0, 1.0):
            got = gp_trees.rule_reference(oracle, t, walk[:-1], dcp, blocks_fn=_moved(which, sign))
            rel = np.abs(got - ref[:-1]) / np.maximum(1.0, np.abs(ref[:-1]))
            worst = min(worst, rel.min())
            assert rel.min() >= 100.0 * RULE_BAR, (name, which, sign, rel)
    # an untripped row at its own dist_cp instead of the cache's
    keep = [rows.index(n) for n in ("keep_q", "keep_dphi", "keep_rwd")]

    def own_blocks(tree, e, v, d):
        p = gp_trees.eclipse_pars(tree, e, v)
        mine = [d[n] for n, val in gp_trees.rule_values().items() if val == (p[4], p[5], p[8])][0]
        return np.array(wd.blocks_of(mine, p[13], 0, 1))
    got = gp_trees.rule_reference(oracle, t, walk[keep], dcp, blocks_fn=own_blocks)
    rel = np.abs(got - ref[keep]) / np.maximum(1.0, np.abs(ref[keep]))
    print("%s: an edge moved by %.1e changes lnlike_e by at least %.2e relative; the cache's dist_cp swapped for "
          "the row's own by at least %.2e" % (name, EDGE_MOVE, worst, rel.min()))
    assert rel.min() >= 100.0 * RULE_BAR, (name, rel)


@pytest.mark.parametrize("name", gp_trees.RULE_CASES)
def test_rule_oracle_and_port(oracle, port, rule_cases, name):
    """the oracle's and the host port's own rule and dist_cp against the
    double's blocks, at the GPU test's bar"""
    t, walk, dcp, ref = rule_cases(name)
    lnp, lle, _ = oracle.lnprob_batch(walk, t, nthreads=4)
    fin = np.isfinite(lnp)
    rel = np.abs(lle[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))
    got, _ = port.lnprob_batch(walk, t, nthreads=4)
    assert np.array_equal(np.isfinite(got), fin)
    prior = lnp[fin] - lle[fin].sum(axis=1)
    relp = np.abs(got[fin] - (prior + ref[fin].sum(axis=1))) / np.maximum(1.0, np.abs(got[fin]))
    print("%s: oracle lnlike_e %.2e, port ln_prob %.2e relative to the double's blocks" % (name, rel.max(), relp.max()))
    assert rel.max() <= RULE_BAR and relp.max() <= RULE_BAR


def test_rule_slip_is_caught(oracle, rule_cases):
    """a deliberate slip: the cached dist_cp used on a tripped row misses by far more than the bar"""
    from tests import wdphases_double as wd
    t, walk, dcp, ref = rule_cases("rule_e1")
    rows = [gp_trees.RULE_ROWS.index(n) for n in gp_trees.RULE_TRIPPED]

    def cached(tree, e, v, d):
        return np.array(wd.blocks_of(d["base"], gp_trees.eclipse_pars(tree, e, v)[13], 0, 1))
    got = gp_trees.rule_reference(oracle, t, walk[rows], dcp, blocks_fn=cached)
    rel = np.abs(got - ref[rows]) / np.maximum(1.0, np.abs(ref[rows]))
    assert rel.min() >= 100.0 * RULE_BAR, rel
