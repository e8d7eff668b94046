"""GPU: lfg_wdphases (k_wdphases; roche.wdphases) against the independent
double of MODEL_SPEC 10.2 as recorded in tests/golden/wdphases_double.npz
(tests/wdphases_double.py, tools/make_wdphases_golden.py): the seeded
population over q in [0.003, 8], the edge rows (inc = 90, just below grazing,
r1 = 0, r1 < 0, r1 = NaN, phi3 < 0, part of the limb never eclipsed) and
ntheta = 1, 2, 3, 7, 16.  Status exactly, failed rows NaN, phi3 and phi4 to
PHASE_ATOL; a batch gives the bits of its rows run alone.
Measured: profiles/gp_dcp/README.md."""
import ctypes

import numpy as np
import pytest

from tests.test_wdphases_double import PHASE_ATOL, compare, load

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 130)   # a lane, a wave less one, a wave, two blocks, three with the last partial


@pytest.fixture(scope="module")
def gold():
    return load()


def run(q, inc, r1, ntheta):
    """lfg_wdphases itself: (phi3, phi4, status, return code); the outputs start as 7.0 / 77"""
    import torch
    from lfit_python_amd import _native
    L = _native.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)  # noqa: E731
    qt, it, rt = t(q), t(inc), t(r1)
    n = qt.shape[0]
    p3 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    p4 = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    st = torch.full((n,), 77, dtype=torch.int32, device=dev)
    vp = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    rc = L.lfg_wdphases(vp(qt), vp(it), vp(rt), n, int(ntheta), vp(p3), vp(p4), vp(st), _native.stream_ptr(dev))
    torch.cuda.synchronize()
    return p3.cpu().numpy(), p4.cpu().numpy(), st.cpu().numpy(), rc


def test_wdphases_matches_double(gold):
    n = len(gold["q"])
    p3, p4, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
    for nt in np.unique(gold["ntheta"]):
        rows = np.flatnonzero(gold["ntheta"] == nt)
        a, b, s, rc = run(gold["q"][rows], gold["inc"][rows], gold["r1"][rows], nt)
        assert rc == 0
        p3[rows], p4[rows], st[rows] = a, b, s
    compare(gold, p3, p4, st, "lfg_wdphases")
    # include/lfg.h: r1 <= 0 or NaN is LFG_ST_BAD_GEOMETRY, a centre that is
    # not eclipsed LFG_ST_BAD_DPHI, q <= 0 or NaN LFG_ST_BAD_Q before either
    k = int(np.flatnonzero(gold["name"] == "r1_zero")[0])
    a, b, s, rc = run([-0.1, np.nan, gold["q"][k]], [gold["inc"][k]] * 3, [0.0, 0.0187, 0.0187], 10)
    assert rc == 0 and list(s) == [1, 1, 0] and np.isnan(a[:2]).all() and np.isnan(b[:2]).all()
    assert abs(a[2] - gold["phi3"][gold["name"] == "example"][0]) <= PHASE_ATOL


def test_ntheta_below_one_is_refused(gold):
    """include/lfg.h: LFG_E_ARGS, nothing written"""
    for nt in (0, -3):
        a, b, s, rc = run(gold["q"][:3], gold["inc"][:3], gold["r1"][:3], nt)
        assert rc == -1 and (a == 7.0).all() and (b == 7.0).all() and (s == 77).all()


def test_batches_are_their_rows(gold):
    """n = 1, 63, 64, 65, 130: bit for bit the rows run alone (failed rows included)"""
    rows = np.flatnonzero(gold["main"])
    # failed and partly eclipsed rows first, so that every batch size holds some
    rows = np.concatenate([rows[~gold["ok"][rows]], rows[gold["ok"][rows]]])[:max(BATCHES)]
    assert (~gold["ok"][rows[:63]]).sum() >= 5 and (gold["count"][rows] < 10).sum() >= 13
    q, inc, r1 = gold["q"][rows], gold["inc"][rows], gold["r1"][rows]
    alone = [run(q[k:k + 1], inc[k:k + 1], r1[k:k + 1], 10) for k in range(len(rows))]
    assert all(r[3] == 0 for r in alone)
    alone = [np.concatenate([r[j] for r in alone]) for j in range(3)]
    for n in BATCHES:
        a, b, s, rc = run(q[:n], inc[:n], r1[:n], 10)
        assert rc == 0
        for got, ref in zip((a, b, s), alone):
            assert got.tobytes() == ref[:n].tobytes(), n


def test_roche_wdphases(gold):
    """the Python entry: arrays give (phi3, phi4) with NaN rows, a failed scalar call raises"""
    from lfit_python_amd import roche
    rows = np.flatnonzero(gold["main"])[-20:]
    p3, p4 = roche.wdphases(gold["q"][rows], gold["inc"][rows], gold["r1"][rows], 10)
    a, b, _, _ = run(gold["q"][rows], gold["inc"][rows], gold["r1"][rows], 10)
    assert p3.tobytes() == a.tobytes() and p4.tobytes() == b.tobytes()
    assert np.isnan(p3).sum() >= 5
    k = int(np.flatnonzero(gold["name"] == "below_grazing")[0])
    with pytest.raises(roche.RocheError):
        roche.wdphases(float(gold["q"][k]), float(gold["inc"][k]), float(gold["r1"][k]), 10)
    k = int(np.flatnonzero((gold["name"] == "partial_5") & gold["main"])[0])
    got = roche.wdphases(float(gold["q"][k]), float(gold["inc"][k]), float(gold["r1"][k]))
    assert max(abs(got[0] - gold["phi3"][k]), abs(got[1] - gold["phi4"][k])) <= PHASE_ATOL
