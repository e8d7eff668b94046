"""The changepoint distance of MODEL_SPEC 10.2-10.3 on the CPU: the oracle's
wdphases and gp_base_dcp and the host twin's gp_dcp against the independent
double of tests/wdphases_double.py, as recorded in
tests/golden/wdphases_double.npz (tools/make_wdphases_golden.py).

The double takes its limb points' egress phases from the contact arbiter
(dense chords, bisection), takes the extremes in a plain loop over the eclipsed
points, and shares no code with what it checks.  The bar is MODEL_SPEC 9's
PHASE_ATOL; a contact the arbiter cannot place to that in FP64
(contact_double.resolved) is left out of the phase comparison, never out of
the status comparison.  Measured worst cases: profiles/gp_dcp/README.md."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import flux_double as fd
from tests import wdphases_double as wd

PHASE_ATOL = 1e-10   # MODEL_SPEC 9
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "wdphases_double.npz")
RECHECK_SEED, RECHECK_ROWS = 5, 8


def load():
    d = dict(np.load(GOLDEN))
    d["ok"] = d["status"] == 0
    d["resolved"] = d["ok"] & d["resolved3"] & d["resolved4"]
    d["main"] = d["ntheta"] == wd.NTHETA
    return d


@pytest.fixture(scope="module")
def gold():
    return load()


@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    path = cpu.build(out=str(tmp_path_factory.mktemp("cpu") / "liblfg_cpu.so"))
    return cpu.CpuPort(path)


def compare(gold, p3, p4, status, what):
    """status and failure rows exactly; phi3, phi4 to PHASE_ATOL on the resolved rows"""
    assert np.array_equal(status, gold["status"]), (what, np.flatnonzero(status != gold["status"]))
    bad = ~gold["ok"]
    assert np.isnan(p3[bad]).all() and np.isnan(p4[bad]).all(), what
    assert np.isfinite(p3[gold["ok"]]).all() and np.isfinite(p4[gold["ok"]]).all(), what
    r = gold["resolved"]
    e3, e4 = np.abs(p3[r] - gold["phi3"][r]), np.abs(p4[r] - gold["phi4"][r])
    part = (gold["count"] < gold["ntheta"])[r]
    print("%s: %d rows, %d compared; worst |phi3| %.2e, |phi4| %.2e; rows with part of the limb eclipsed: "
          "%.2e, %.2e" % (what, len(r), r.sum(), e3.max(), e4.max(), e3[part].max(), e4[part].max()))
    assert e3.max() <= PHASE_ATOL and e4.max() <= PHASE_ATOL, (what, e3.max(), e4.max())


def test_population(gold):
    """what keeps the comparisons from passing empty, asserted from the file"""
    n = len(gold["q"])
    main, ok = gold["main"], gold["ok"]
    seeded = gold["name"] == "seeded"
    assert (seeded & main).sum() == 160 and 170 <= main.sum()
    for nt in (1, 2, 3, 7, 16):
        assert (gold["ntheta"] == nt).sum() == 24
    q = gold["q"][seeded]
    assert q.min() >= 0.003 and q.max() <= 8.0 and q.min() < 0.01 and q.max() > 4.0 and (q > 1.0).sum() >= 20
    r1 = gold["r1"][seeded]
    assert r1.min() >= 1e-3 and r1.max() <= 0.1
    # at least 10 % with only part of the limb eclipsed, overall and at ntheta = 10
    part = ok & (gold["count"] < gold["ntheta"])
    assert part.sum() >= 0.10 * n and (part & main).sum() >= 0.10 * main.sum()
    # at most 5 % unresolved at 1e-10
    assert (ok & ~gold["resolved"]).sum() <= 0.05 * n
    # the edge rows
    row = lambda name: np.flatnonzero((gold["name"] == name) & main)[0]  # noqa: E731
    assert gold["inc"][row("inc_90")] == 90.0 and ok[row("inc_90")] and gold["count"][row("inc_90")] == 10
    assert gold["inc"][row("inc_90_q_above_1")] == 90.0 and ok[row("inc_90_q_above_1")]
    for name in ("below_grazing", "below_grazing_q_above_1"):
        assert gold["status"][row(name)] == wd.ST_BAD_DPHI
    for name in ("r1_zero", "r1_negative", "r1_nan"):
        assert gold["status"][row(name)] == wd.ST_BAD_GEOMETRY
    assert gold["r1"][row("r1_zero")] == 0.0 and gold["r1"][row("r1_negative")] < 0.0
    assert np.isnan(gold["r1"][row("r1_nan")])
    assert gold["phi3"][row("phi3_negative")] < 0.0 and (ok & (gold["phi3"] < 0.0)).sum() >= 5
    assert gold["count"][row("partial_6")] == 6 and gold["count"][row("partial_5")] == 5
    assert (gold["count"][ok] >= 1).all() and (gold["phi3"][ok] <= gold["phi4"][ok]).all()
    # one limb point: phi3 = phi4, the egress of the point r1 u1
    one = ok & (gold["ntheta"] == 1)
    assert one.sum() >= 20 and np.array_equal(gold["phi3"][one], gold["phi4"][one])


def test_file_is_the_doubles(gold):
    """a seeded subsample recomputed with the double: bit for bit"""
    rng = np.random.default_rng(RECHECK_SEED)
    ok = np.flatnonzero(gold["ok"])
    rows = list(rng.choice(ok, RECHECK_ROWS - 2, replace=False))
    rows += [np.flatnonzero(gold["name"] == "r1_nan")[0], np.flatnonzero(gold["name"] == "below_grazing")[0]]
    assert len({int(gold["ntheta"][k]) for k in rows}) >= 3
    for k in rows:
        st, p3, p4, count, _, _ = wd.solve(float(gold["q"][k]), float(gold["inc"][k]), float(gold["r1"][k]),
                                           int(gold["ntheta"][k]))
        assert (st, count) == (gold["status"][k], gold["count"][k]), k
        assert np.array_equal(np.array([p3, p4]), np.array([gold["phi3"][k], gold["phi4"][k]]), equal_nan=True), k
    # the recorded inclination is the double's findi of the recorded dphi
    k = int(rows[0]) if math.isfinite(gold["dphi"][rows[0]]) else int(np.flatnonzero(gold["name"] == "seeded")[0])
    assert fd.findi(float(gold["q"][k]), float(gold["dphi"][k])) == gold["inc"][k]


def oracle_rows(oracle, gold):
    n = len(gold["q"])
    p3, p4, st = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, dtype=np.int32)
    rc = oracle.lib.lfo_wdphases  # the status itself, which Oracle.wdphases folds into an exception
    for k in range(n):
        a, b = ctypes.c_double(), ctypes.c_double()
        st[k] = rc(float(gold["q"][k]), float(gold["inc"][k]), float(gold["r1"][k]), int(gold["ntheta"][k]),
                   ctypes.byref(a), ctypes.byref(b))
        if st[k] == 0:
            p3[k], p4[k] = a.value, b.value
    return p3, p4, st


def test_oracle_wdphases(oracle, gold):
    p3, p4, st = oracle_rows(oracle, gold)
    compare(gold, p3, p4, st, "oracle.wdphases")
    # Oracle.wdphases raises where the status is not zero
    k = int(np.flatnonzero(~gold["ok"])[0])
    with pytest.raises(ValueError):
        oracle.wdphases(gold["q"][k], gold["inc"][k], gold["r1"][k], int(gold["ntheta"][k]))


def dcp_rows(gold):
    """rows that came from a dphi (inc = findi(q, dphi)) at ntheta = 10: the double's dist_cp"""
    rows = np.flatnonzero(gold["main"] & np.isfinite(gold["dphi"]))
    ref = (gold["dphi"][rows] + gold["phi4"][rows] - gold["phi3"][rows]) / 2.0
    return rows, ref


def compare_dcp(gold, got, what):
    rows, ref = dcp_rows(gold)
    assert len(rows) >= 165
    assert np.array_equal(np.isnan(got), ~gold["ok"][rows]), what
    r = gold["resolved"][rows]
    err = np.abs(got[r] - ref[r])
    print("%s: dist_cp of %d rows, worst %.2e" % (what, r.sum(), err.max()))
    assert err.max() <= PHASE_ATOL, (what, err.max())


def test_oracle_gp_base_dcp(oracle, gold):
    rows, _ = dcp_rows(gold)
    got = np.full(len(rows), np.nan)
    for j, k in enumerate(rows):
        try:
            got[j] = oracle.gp_base_dcp(gold["q"][k], gold["dphi"][k], gold["r1"][k])
        except ValueError:
            pass
    compare_dcp(gold, got, "oracle.gp_base_dcp")


def test_port_gp_dcp(port, gold):
    rows, _ = dcp_rows(gold)
    got = np.array([port.gp_dcp(gold["q"][k], gold["dphi"][k], gold["r1"][k]) for k in rows])
    compare_dcp(gold, got, "cpu_baseline gp_dcp")


def test_all_points_slip_is_caught(gold):
    """the deliberate slip of taking the extremes over every limb point
    instead of the eclipsed ones moves phi3 of a partly eclipsed row by far
    more than the bar (the arbiter's empty interval has b = -1)"""
    k = int(np.flatnonzero((gold["name"] == "partial_6") & gold["main"])[0])
    st, p3, p4 = wd.solve(float(gold["q"][k]), float(gold["inc"][k]), float(gold["r1"][k]), 10, all_points=True)[:3]
    assert st == 0 and p4 == gold["phi4"][k] and abs(p3 - gold["phi3"][k]) > 1e6 * PHASE_ATOL


def test_rule():
    """the Python restatement of 10.3's rule: strict, relative to the walker's value"""
    base = (0.1, 0.04, 0.02, 0.021)
    assert not wd.tripped(base, 0.1, 0.04, 0.02)
    for j in range(3):
        v = list(base[:3])
        v[j] = base[j] / (2.2 * (1.0 + 1e-3))     # |B - v| / v = B / v - 1 = 1.2022
        assert wd.tripped(base, *v)
        v[j] = base[j] / (2.2 * (1.0 - 1e-3))     # 1.1978
        assert not wd.tripped(base, *v)
        v[j] = base[j] * 50.0           # above the base: |B - v| / v < 1, never
        assert not wd.tripped(base, *v)
    assert wd.blocks(base, 0.1, 0.04, 0.02, 0.001, 0, 1) == [[-1 + 0.021 + 0.001, -0.021 + 0.001],
                                                            [0.021 + 0.001, (1 - 0.021) + 0.001]]
    assert wd.blocks(base, 0.1, 0.04 / 2.3, 0.02, 0.0, 0, 0, own=0.0125) == [[-1 + 0.0125, -0.0125]]
    assert wd.blocks(base, 0.1, 0.04 / 2.3, 0.02, 0.0, 0, 0, own=math.nan) is None
