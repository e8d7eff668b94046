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
