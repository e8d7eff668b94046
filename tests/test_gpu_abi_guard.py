"""GPU: where the entry points of include/lfg.h read and write.

Every case below is one valid use of the header, written once as a function
of an allocator (tests/abi_guard.py) and run
  (a) on plain torch.empty buffers,
  (b) in the guarded arena with the scratch poisoned with all-ones bytes,
  (c) with the scratch zeroed,
  (d) with the scratch left over from another case's call,
  (e) as (b) under a side stream (torch.cuda.stream(torch.cuda.Stream())).
Scratch is passed at exactly the size function's value and outputs have
exactly the header's shape.  Asserted: the guards around every buffer are
intact (after every call of a chain), const inputs are bit-unchanged, the
outputs of (b)-(e) are bit-identical to (a)'s (the kernels are
bit-deterministic), (a) meets the oracle at the project's tolerances, and no
output element the header defines still holds poison.  One further run per
scratch-taking entry point passes ws_bytes one byte short: the header's error
code comes back and every output and the scratch stay poisoned (the size
check precedes every launch).

Shapes are the smallest that cross the kernels' internal edges: N of 1, 65,
512, 513 (one point, one past a wave, a full tile, one past it: LONG) and 0,
W of 1, 5, 65 (k_setup's lane bounds), nsub of 1 and 3, P of 14 and 18."""
import ctypes
import re

import numpy as np
import pytest

from tests import abi_guard as ag
from tests.abi_guard import ptr
from tests.helpers import random_pars
from tests.test_gpu_lnprob import LNP_RTOL, _same, layout  # noqa: F401  (layout: the fixture)
from tests.test_gpu_parity import FLUX_RTOL, assert_geo_matches
from tests.test_native_abi import declared_functions

pytestmark = pytest.mark.gpu

E_ARGS, E_WORKSPACE = -1, -2
CASES = {}     # name -> Case
_DATA = {}     # name -> host data of the case (built once)
_PLAIN = {}    # (name, layout) -> run (a)'s result bytes


class Case:
    def __init__(self, name, fn, data, covers, verify=None, both_layouts=False, short=None, unwritten=None):
        """unwritten(D) -> {output name: bool mask}: the elements lfg.h says a call leaves alone"""
        self.name, self.fn, self.data, self.covers, self.verify = name, fn, data, tuple(covers), verify
        self.both_layouts, self.short, self.unwritten = both_layouts, short, unwritten


def add(name, fn, data, covers, **kw):
    assert name not in CASES
    CASES[name] = Case(name, fn, data, covers, **kw)


def data_of(name, oracle):
    if name not in _DATA:
        _DATA[name] = CASES[name].data(oracle)
    return _DATA[name]


def lib():
    from lfit_python_amd import _native
    return _native.lib()


def f64():
    import torch
    return torch.float64


def i32():
    import torch
    return torch.int32


# ------------------------------------------------------------------ flat batch
def _grid(N):
    if N == 0:
        return np.zeros(0), np.zeros(0)
    if N == 1:
        return np.array([0.013]), np.array([0.001])
    x = np.linspace(-0.3, 0.3, N)
    return x, np.mean(np.diff(x)) * np.ones_like(x) / 2.0


def _flat_data(W, P, N, nsub, wnull, seed):
    def build(oracle):
        pars = random_pars(W, complex_bs=(P == 18), seed=seed)
        if W > 1:
            pars[1, 4] = -0.2          # an invalid mass ratio: a failed set among the W
        x, w = _grid(N)
        wo = np.zeros_like(x) if wnull else w
        ref = []
        for p in pars:
            st, out = oracle.flux(p, x, wo, nsub=nsub, components=True) if N else (oracle.elements(p)[0], None)
            ref.append((st, out))
        rng = np.random.default_rng(seed + 5)
        st0, f0 = oracle.flux(pars[0], x, wo, nsub=nsub) if N else (0, np.zeros(0))
        ye = 1e-3 * np.ones(N)
        y = f0 + ye * rng.standard_normal(N)
        return dict(pars=pars, x=x, w=None if wnull else w, y=y, ye=ye, ref=ref, W=W, P=P, N=N, nsub=nsub)
    return build


def _flux_case(comps):
    def fn(A, D, short=0):
        L = lib()
        W, P, N = D["W"], D["P"], D["N"]
        pars, x = A.inp("pars", D["pars"]), A.inp("x", D["x"])
        w = A.inp("w", D["w"]) if D["w"] is not None else None
        flux = A.out("flux", (W, N), f64())
        cm = A.out("comps", (4, W, N), f64()) if comps else None
        st = A.out("status", (W,), i32())
        nb = L.lfg_workspace_size(W, 1)
        ws = A.ws("ws", nb)
        return [("lfg_flux", L.lfg_flux(ptr(pars), W, P, ptr(x) if N else None, ptr(w), N, D["nsub"], ptr(flux),
                                        ptr(cm), ptr(st), ptr(ws), nb - short, A.stream_ptr()))]
    return fn


def _flux_verify(D, A):
    flux, st = A.tensor("flux").cpu().numpy(), A.tensor("status").cpu().numpy()
    cm = A.tensor("comps").cpu().numpy() if "comps" in A.bufs else None
    for i, (ost, out) in enumerate(D["ref"]):
        assert st[i] == ost, (i, st[i], ost)
        if ost != 0:   # a failed set: NaN flux (and components), by the header
            assert np.all(np.isnan(flux[i])) and (cm is None or np.all(np.isnan(cm[:, i])))
            continue
        if D["N"] == 0:
            continue
        scale = np.max(np.abs(out[0]))
        assert np.max(np.abs(flux[i] - out[0])) / scale < FLUX_RTOL
        if cm is not None:
            for k in range(4):
                assert np.max(np.abs(cm[k, i] - out[1 + k])) / scale < FLUX_RTOL
    assert sum(1 for ost, _ in D["ref"] if ost == 0) >= max(1, D["W"] - 1)


def _lnlike_case(A, D, short=0):
    L = lib()
    W, P, N = D["W"], D["P"], D["N"]
    pars, x = A.inp("pars", D["pars"]), A.inp("x", D["x"])
    w = A.inp("w", D["w"]) if D["w"] is not None else None
    y, ye = A.inp("y", D["y"]), A.inp("ye", D["ye"])
    ll = A.out("lnlike", (W,), f64())
    st = A.out("status", (W,), i32())
    nb = L.lfg_workspace_size(W, 1)
    ws = A.ws("ws", nb)
    z = lambda t: ptr(t) if N else None
    return [("lfg_lnlike", L.lfg_lnlike(ptr(pars), W, P, z(x), ptr(w), N, D["nsub"], z(y), z(ye), ptr(ll), ptr(st),
                                        ptr(ws), nb - short, A.stream_ptr()))]


def _lnlike_verify(D, A):
    ll, st = A.tensor("lnlike").cpu().numpy(), A.tensor("status").cpu().numpy()
    ref = np.empty(D["W"])
    for i, (ost, out) in enumerate(D["ref"]):
        assert st[i] == ost
        ref[i] = -0.5 * np.sum(((D["y"] - out[0]) / D["ye"]) ** 2) if (ost == 0 and D["N"]) else (0.0 if ost == 0 else -np.inf)
    _same(ll, ref, LNP_RTOL)   # -inf where status != LFG_ST_OK, by the header


def _elements_case(A, D, short=0):
    from lfit_python_amd import _native as nt
    L = lib()
    W, P = D["W"], D["P"]
    pars = A.inp("pars", D["pars"])
    a, b, wg = (A.out(k, (W, nt.NEL), f64()) for k in ("a", "b", "wgt"))
    don = A.out("donor", (W, nt.NDONOR, 3), f64())
    geo = A.out("geo", (W, nt.NGEO), f64())
    st = A.out("status", (W,), i32())
    nb = L.lfg_workspace_size(W, 1)
    ws = A.ws("ws", nb)
    return [("lfg_elements", L.lfg_elements(ptr(pars), W, P, ptr(a), ptr(b), ptr(wg), ptr(don), ptr(geo), ptr(st),
                                            ptr(ws), nb - short, A.stream_ptr()))]


def _elements_data(W, P, seed):
    def build(oracle):
        pars = random_pars(W, complex_bs=(P == 18), seed=seed)
        if W > 1:
            pars[1, 4] = -0.2
        return dict(pars=pars, W=W, P=P, ref=[oracle.elements(p) for p in pars])
    return build


def _elements_unwritten(D):
    """lfg.h: the a, b, wgt and donor rows of a set whose status is not LFG_ST_OK are left unwritten"""
    from lfit_python_amd import _native as nt
    failed = np.array([r[0] != 0 for r in D["ref"]])
    row = lambda *shape: np.broadcast_to(failed.reshape((-1,) + (1,) * len(shape)), (len(failed),) + shape).copy()
    return {"a": row(nt.NEL), "b": row(nt.NEL), "wgt": row(nt.NEL), "donor": row(nt.NDONOR, 3)}


# lfg_device.hpp's enum Geo: G_BSVX, G_BSVY (18, 19) and G_GP_AIN .. G_GP_RWD (41 .. 47)
GEO_UNDEFINED = [18, 19] + list(range(41, 48))
# G_Q, G_ULIMB, G_DEXP, G_FIS, G_PHI0, G_WDF, G_DF, G_SF, G_RSF: the parameters q, ulimb, dexp, fis,
# phi0 and the four fluxes, kept as given
GEO_CARRIED = [0, 14, 15, 32, 33, 34, 35, 36, 37]


def _elements_verify(D, A):
    get = lambda k: A.tensor(k).cpu().numpy()
    st, wg, geo = get("status"), get("wgt"), get("geo")
    for i, (ost, oa, ob, ow, odon, ogeo) in enumerate(D["ref"]):
        assert st[i] == ost
        # lfg.h: the slots no flat call defines (the stream's velocity at the spot, the GP
        # likelihood's seven) are 0 in every row, as is whatever a failed set did not reach
        assert np.all(geo[i, GEO_UNDEFINED] == 0.0), (i, geo[i, GEO_UNDEFINED])
        if ost != 0:
            assert np.count_nonzero(geo[i]) < np.count_nonzero(geo[0]), i     # it stopped early
            continue
        # and a valid set's record is otherwise filled: the geometry both sides export (checked
        # against the oracle below) and the inputs it carries along
        assert np.all(geo[i, GEO_CARRIED] == D["pars"][i][[4, 7, 12, 11, 13, 0, 1, 2, 3]]), i
        np.testing.assert_allclose(wg[i], ow, rtol=1e-12)
        assert_geo_matches(geo[i], ogeo, "set %d" % i)


for _W, _P, _N, _S, _wnull, _comps in ((1, 18, 1, 1, False, False), (5, 14, 65, 3, False, True),
                                       (65, 18, 512, 1, True, False), (5, 18, 513, 1, False, True),
                                       (5, 18, 0, 1, False, False)):
    _n = "W%d_P%d_N%d_S%d%s" % (_W, _P, _N, _S, "_points" if _wnull else "")
    add("flux_" + _n + ("_comps" if _comps else ""), _flux_case(_comps), _flat_data(_W, _P, _N, _S, _wnull, 41),
        ["lfg_flux"], verify=_flux_verify, short=E_WORKSPACE)
for _W, _P, _N, _S, _wnull in ((1, 14, 1, 1, False), (5, 18, 65, 3, False), (65, 18, 512, 1, True),
                               (5, 14, 513, 1, False), (5, 18, 0, 1, False), (5, 14, 0, 3, False)):
    add("lnlike_W%d_P%d_N%d_S%d%s" % (_W, _P, _N, _S, "_points" if _wnull else ""), _lnlike_case,
        _flat_data(_W, _P, _N, _S, _wnull, 43), ["lfg_lnlike"], verify=_lnlike_verify, both_layouts=True,
        short=E_WORKSPACE)
for _W, _P in ((1, 14), (5, 18), (65, 18)):
    add("elements_W%d_P%d" % (_W, _P), _elements_case, _elements_data(_W, _P, 47), ["lfg_elements"],
        verify=_elements_verify, short=E_WORKSPACE, unwritten=_elements_unwritten)


# ------------------------------------------------------------------ roche, wdphases
def _roche_data(oracle):
    q = np.array([0.05, 0.1037, 0.2, 0.5, -1.0])     # the last: an invalid mass ratio
    inc = np.array([84.0, 86.9, 90.0, 85.0, 85.0])
    dphi = np.array([oracle.findphi(v, 85.0) for v in q[:4]] + [0.05])
    rad = np.array([0.55 * oracle.xl1(v) for v in q[:4]] + [0.3])
    ref = {0: [oracle.xl1(v) for v in q[:4]], 1: [oracle.findphi(v, i) for v, i in zip(q[:4], inc)],
           2: [oracle.findi(v, d) for v, d in zip(q[:4], dphi)], 3: [oracle.bspot(v, r) for v, r in zip(q[:4], rad)]}
    r1 = np.array([0.01, 0.02, 0.015, 0.03, 0.02])
    wd = [oracle.wdphases(v, i, r, 10) for v, i, r in zip(q[:4], inc, r1)]
    return dict(q=q, b={0: None, 1: inc, 2: dphi, 3: rad}, ref=ref, r1=r1, inc=inc, wd=wd)


def _roche_case(A, D, short=0):
    L, n = lib(), 5
    q = A.inp("q", D["q"])
    rcs = []
    for op in range(4):
        b = A.inp("b%d" % op, D["b"][op]) if op else None
        out = A.out("out%d" % op, (4 * n if op == 3 else n,), f64())
        st = A.out("status%d" % op, (n,), i32())
        rcs.append(("lfg_roche", L.lfg_roche(op, ptr(q), ptr(b), n, ptr(out), ptr(st), A.stream_ptr())))
    inc, r1 = A.inp("inc", D["inc"]), A.inp("r1", D["r1"])
    p3, p4 = A.out("phi3", (n,), f64()), A.out("phi4", (n,), f64())
    st = A.out("wd_status", (n,), i32())
    rcs.append(("lfg_wdphases", L.lfg_wdphases(ptr(q), ptr(inc), ptr(r1), n, 10, ptr(p3), ptr(p4), ptr(st),
                                               A.stream_ptr())))
    return rcs


def _roche_verify(D, A):
    get = lambda k: A.tensor(k).cpu().numpy()
    # the roche tests' own tolerances (tests/test_gpu_parity.py), none looser than 1e-9
    tol = {0: dict(rtol=1e-13, atol=0), 1: dict(rtol=0, atol=1e-11), 2: dict(rtol=0, atol=1e-9),
           3: dict(rtol=1e-9, atol=1e-11)}
    for op in range(4):
        st, out = get("status%d" % op), get("out%d" % op)
        assert np.all(st[:4] == 0) and st[4] != 0     # q < 0: a failed row, its status says so
        assert np.all(np.isnan(out.reshape(5, -1)[4]))   # lfg.h: NaN where the status is not LFG_ST_OK
        got = out.reshape(5, -1)[:4]
        np.testing.assert_allclose(got, np.asarray(D["ref"][op]).reshape(4, -1), **tol[op])
    assert np.all(get("wd_status")[:4] == 0) and get("wd_status")[4] != 0
    assert np.isnan(get("phi3")[4]) and np.isnan(get("phi4")[4])   # lfg.h: NaN where the status is not LFG_ST_OK
    np.testing.assert_allclose(np.stack([get("phi3"), get("phi4")], 1)[:4], np.asarray(D["wd"]), rtol=1e-9, atol=1e-11)


add("roche_wdphases_n5", _roche_case, _roche_data, ["lfg_roche", "lfg_wdphases"], verify=_roche_verify)


# ------------------------------------------------------------------ components
COMP_GRIDS = {0: (0, 0), 1: (5, 7), 2: (9, 0), 3: (5, 7)}


def _comp_data(kind, fail=False):
    def build(oracle):
        from tests.helpers import ECL1, TRUTH18
        from tests.test_components import _split
        N = 65
        x, w = _grid(N)
        sets = [_split(TRUTH18), _split(ECL1)]
        q = np.array([s[0] for s in sets])
        if fail:
            q[1] = -0.1           # an invalid mass ratio: a failed set beside a valid one
        inc = np.array([oracle.findi(s[0], s[1]) for s in sets])
        cp = np.array([s[4][kind] for s in sets], dtype=np.float64).reshape(2, -1)
        ref = [oracle.component(kind, cp[i], q[i], inc[i], x, w, *COMP_GRIDS[kind]) for i in range(2)]
        return dict(kind=kind, x=x, w=w, q=q, inc=inc, cp=cp, ref=ref, fail=fail)
    return build


def _comp_case(A, D, short=0):
    L, kind, W, N = lib(), D["kind"], 2, 65
    n1, n2 = COMP_GRIDS[kind]
    ncp = D["cp"].shape[1]
    cp = A.inp("cpars", D["cp"]) if ncp else None
    q, inc, x, w = (A.inp(k, D[k]) for k in ("q", "inc", "x", "w"))
    out, st = A.out("out", (W, N), f64()), A.out("status", (W,), i32())
    nb = L.lfg_component_workspace_size(kind, W, n1, n2)
    ws = A.ws("ws", nb)
    return [("lfg_component", L.lfg_component(kind, ptr(cp), ncp, ptr(q), ptr(inc), W, n1, n2, ptr(x), ptr(w), N,
                                              ptr(out), ptr(st), ptr(ws), nb - short, A.stream_ptr()))]


def _comp_verify(D, A):
    out, st = A.tensor("out").cpu().numpy(), A.tensor("status").cpu().numpy()
    for i, (ost, ref) in enumerate(D["ref"]):
        assert st[i] == ost
        if ost != 0:              # lfg.h: the out row of a failed set is NaN
            assert np.all(np.isnan(out[i]))
            continue
        np.testing.assert_allclose(out[i], ref, rtol=1e-9, atol=1e-12)
    assert [ost for ost, _ in D["ref"]].count(0) == (1 if D["fail"] else 2)


for _k in range(4):
    add("component_kind%d" % _k, _comp_case, _comp_data(_k), ["lfg_component"], verify=_comp_verify,
        short=E_WORKSPACE)
    add("component_kind%d_failed_set" % _k, _comp_case, _comp_data(_k, fail=True), ["lfg_component"],
        verify=_comp_verify)


# ------------------------------------------------------------------ GP filter and smoother
def _gp_data(N):
    def build(oracle):
        rng = np.random.default_rng(1000 + N)
        W, nb = 3, 2
        x = np.sort(rng.uniform(-0.2, 0.3, N))
        ye = rng.uniform(0.003, 0.006, N)
        res = 0.004 * rng.standard_normal((W, N))
        hyp = np.stack([np.exp(rng.uniform(-11, -8, W)), np.exp(rng.uniform(-11, -8, W)),
                        np.exp(rng.uniform(-6.9, -2, W))], axis=1)
        d = rng.uniform(0.01, 0.05, W)
        blocks = np.stack([np.stack([-1 + d, -d], 1), np.stack([d, 1 - d], 1)], axis=1)
        ref = [oracle.gp_lnlike(x, res[i], ye, *hyp[i], blocks[i]) for i in range(W)]
        return dict(x=x, ye=ye, res=res, hyp=hyp, blocks=blocks, ref=np.array(ref), N=N, W=W, nb=nb)
    return build


def _gp_case(A, D, short=0):
    L = lib()
    x, ye, res, hyp, bl = (A.inp(k, D[k]) for k in ("x", "ye", "res", "hyp", "blocks"))
    out = A.out("lnlike", (D["W"],), f64())
    return [("lfg_gp_lnlike", L.lfg_gp_lnlike(ptr(x), ptr(ye), ptr(res), D["W"], D["N"], ptr(hyp), ptr(bl), D["nb"],
                                              ptr(out), A.stream_ptr()))]


def _gp_verify(D, A):
    got = A.tensor("lnlike").cpu().numpy()
    assert np.all(np.abs(got - D["ref"]) <= 1e-9 * np.abs(D["ref"])), (got, D["ref"])


for _N in (1, 63, 65, 300):
    add("gp_lnlike_N%d" % _N, _gp_case, _gp_data(_N), ["lfg_gp_lnlike"], verify=_gp_verify)


def _smooth_data(oracle):
    from tests import gp_smoother as gs
    W, N, nb = 3, 65, 2
    cases = [gs.make_case(77 + 1000 * k, N, nb) for k in range(W)]
    x, ye, t = cases[0][0], cases[0][1], cases[0][5]
    res, hyp = np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases])
    blocks = np.stack([c[4] for c in cases])
    n = N + t.size
    z = np.concatenate([x, t])
    order = np.argsort(z, kind="stable")
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    rm, yem = np.zeros((W, n)), np.zeros(n)
    rm[:, inv[:N]] = res
    yem[inv[:N]] = ye
    return dict(x=z[order], ye=yem, obs=(order < N).astype(np.int32), res=rm, hyp=hyp, blocks=blocks, W=W, n=n, nb=nb,
                it=inv[N:], raw=(x, ye, res, t))


def _predict_case(with_var):
    def fn(A, D, short=0):
        L, W, n = lib(), D["W"], D["n"]
        x, ye, obs, res, hyp, bl = (A.inp(k, D[k]) for k in ("x", "ye", "obs", "res", "hyp", "blocks"))
        mean = A.out("mean", (W, n), f64())
        var = A.out("var", (W, n), f64()) if with_var else None
        st = A.out("status", (W,), i32())
        nb = L.lfg_gp_predict_workspace_size(W, n)
        ws = A.ws("ws", nb)
        return [("lfg_gp_predict", L.lfg_gp_predict(ptr(x), ptr(ye), ptr(obs), ptr(res), W, n, ptr(hyp), ptr(bl),
                                                    D["nb"], ptr(mean), ptr(var), ptr(st), ptr(ws), nb - short,
                                                    A.stream_ptr()))]
    return fn


def _predict_verify(D, A):
    from tests import gp_smoother as gs
    x, ye, res, t = D["raw"]
    mean = A.tensor("mean").cpu().numpy()
    var = A.tensor("var").cpu().numpy() if "var" in A.bufs else None
    assert np.all(A.tensor("status").cpu().numpy() == 0)
    for k in range(D["W"]):
        gs.check(mean[k][D["it"]], None if var is None else var[k][D["it"]], x, ye, res[k], D["hyp"][k], D["blocks"][k], t)


def _sample_case(A, D, short=0):
    L, W, n, S = lib(), D["W"], D["n"], 3
    x, ye, obs, res, hyp, bl = (A.inp(k, D[k]) for k in ("x", "ye", "obs", "res", "hyp", "blocks"))
    out = A.out("draws", (W, S, n), f64())
    st = A.out("status", (W,), i32())
    nb = L.lfg_gp_sample_workspace_size(W, n, S)
    ws = A.ws("ws", nb)
    rcs = [("lfg_gp_sample", L.lfg_gp_sample(ptr(x), ptr(ye), ptr(obs), ptr(res), W, n, ptr(hyp), ptr(bl), D["nb"],
                                             S, 12345, 2, ptr(out), ptr(st), ptr(ws), nb - short, A.stream_ptr()))]
    # the batch cut: rows 1 .. W - 1 alone, first = the index of their row 0 (lfg.h: the same bits)
    res1, hyp1, bl1 = A.inp("res.tail", D["res"][1:]), A.inp("hyp.tail", D["hyp"][1:]), A.inp("blocks.tail", D["blocks"][1:])
    out1 = A.out("draws.tail", (W - 1, S, n), f64())
    st1 = A.out("status.tail", (W - 1,), i32())
    nb1 = L.lfg_gp_sample_workspace_size(W - 1, n, S)
    ws1 = A.ws("ws.tail", nb1)
    rcs.append(("lfg_gp_sample", L.lfg_gp_sample(ptr(x), ptr(ye), ptr(obs), ptr(res1), W - 1, n, ptr(hyp1), ptr(bl1),
                                                 D["nb"], S, 12345, 3, ptr(out1), ptr(st1), ptr(ws1), nb1 - short,
                                                 A.stream_ptr())))
    return rcs


def _sample_verify(D, A):
    from tests import gp_smoother as gs
    draws = A.tensor("draws").cpu().numpy()
    assert np.all(A.tensor("status").cpu().numpy() == 0) and np.all(A.tensor("status.tail").cpu().numpy() == 0)
    assert np.all(np.isfinite(draws))
    np.testing.assert_array_equal(A.tensor("draws.tail").cpu().numpy(), draws[1:])   # keyed by first + vector
    # every draw is a path of its own, and each lies within the prior's reach of the smoother's
    # mean (checked against the dense GP by the gp_predict cases): |draw - mean| <= 8 sqrt(ampin + ampout)
    flat = draws.reshape(-1, draws.shape[-1])
    assert len({row.tobytes() for row in flat}) == len(flat)
    x, ye, res, t = D["raw"]
    for k in range(D["W"]):
        mu, _ = gs.dense_predict(x, ye, res[k], *D["hyp"][k], D["blocks"][k], t)
        reach = 8.0 * np.sqrt(D["hyp"][k][0] + D["hyp"][k][1])
        assert np.max(np.abs(draws[k][:, D["it"]] - mu[None, :])) <= reach, k
    # draw for draw against the host double (tests/gp_sample_double.py) on the whole merged grid, at the GP
    # bar: row k of the first call is keyed 2 + k, row k of the tail 3 + k
    from tests import gp_sample_double as gd
    if "double" not in D:
        D["double"] = np.stack([gd.draws(D["x"], D["ye"], D["obs"], D["res"][k], D["hyp"][k], D["blocks"][k], 3, 12345,
                                         2, k) for k in range(D["W"])])
        tail = np.stack([gd.draws(D["x"], D["ye"], D["obs"], D["res"][k], D["hyp"][k], D["blocks"][k], 3, 12345, 3,
                                  k - 1) for k in range(1, D["W"])])
        assert np.array_equal(tail, D["double"][1:])
    tail_draws = A.tensor("draws.tail").cpu().numpy()
    for k in range(D["W"]):
        bar = gs.BAR * np.sqrt(D["hyp"][k][0] + D["hyp"][k][1])
        assert np.max(np.abs(draws[k] - D["double"][k])) <= bar, k
        if k:
            assert np.max(np.abs(tail_draws[k - 1] - D["double"][k])) <= bar, k


# the GP posterior entry points answer a short scratch with LFG_E_ARGS (the header's rule for them)
add("gp_predict_var", _predict_case(True), _smooth_data, ["lfg_gp_predict"], verify=_predict_verify, short=E_ARGS)
add("gp_predict_mean_only", _predict_case(False), _smooth_data, ["lfg_gp_predict"], verify=_predict_verify,
    short=E_ARGS)
add("gp_sample_S3_first2", _sample_case, _smooth_data, ["lfg_gp_sample"], verify=_sample_verify, short=E_ARGS)


# ------------------------------------------------------------------ parallel tempering
def _pt_data(oracle):
    rng = np.random.default_rng(9)
    T, W, nd = 3, 6, 3
    pos = rng.standard_normal((T, W, nd))
    return dict(pos=pos, lnl=-0.5 * np.sum(pos[..., :2] ** 2, -1), lnpr=-0.5 * pos[..., 2] ** 2 / 9.0,
                betas=np.array([1.0, 0.5, 0.0]), T=T, W=W, nd=nd)


def _pt_case(A, D, short=0):
    import torch
    L, T, W, nd = lib(), D["T"], D["W"], D["nd"]
    n = T * (W // 2)
    pos, lnl, lnpr = A.io("pos", D["pos"]), A.io("lnl", D["lnl"]), A.io("lnpr", D["lnpr"])
    betas = A.inp("betas", D["betas"])
    nacc = A.io("naccept", np.zeros((T, W), np.int32))
    rcs = []
    if not short:
        for half in (0, 1):
            q, zf = A.out("q%d" % half, (n, nd), f64()), A.out("zfac%d" % half, (n,), f64())
            rcs.append(("lfg_pt_propose", L.lfg_pt_propose(ptr(pos), T, W, nd, half, 2.0, 5, 3, ptr(q), ptr(zf),
                                                           A.stream_ptr())))
            lle, lnew = A.out("lle%d" % half, (n, 2), f64()), A.out("lnew%d" % half, (n,), f64())
            lle.copy_(-0.5 * q[:, :2] ** 2)
            lnew.copy_(lle.sum(1) - 0.5 * q[:, 2] ** 2 / 9.0)
            if half == 1:
                lnew[1] = float("-inf")   # rejected whatever lnlike_e holds
            rcs.append(("lfg_pt_accept", L.lfg_pt_accept(ptr(pos), ptr(lnl), ptr(lnpr), T, W, nd, half, ptr(betas),
                                                         ptr(q), ptr(zf), ptr(lnew), ptr(lle), 2, 5, 3,
                                                         ptr(nacc) if half == 0 else None, A.stream_ptr())))
    pos_out = A.out("pos_out", (T, W, nd), f64())
    nswap = A.io("nswap", np.zeros((T, 2), np.int64))
    nb = L.lfg_pt_workspace_size(T, W)
    ws = A.ws("ws", nb)
    rcs.append(("lfg_pt_swap", L.lfg_pt_swap(ptr(pos), ptr(pos_out), ptr(lnl), ptr(lnpr), T, W, nd, ptr(betas), 5, 3,
                                             ptr(nswap), ptr(ws), nb - short, A.stream_ptr())))
    return rcs


def _pt_verify(D, A):
    from tests import pt_double as pd
    T, W = D["T"], D["W"]
    # replay on the host double from the device's own proposals and ln_probs (draw for draw)
    pos, lnl, lnpr = D["pos"].copy(), D["lnl"].copy(), D["lnpr"].copy()
    nacc = np.zeros((T, W), np.int32)
    for half in (0, 1):
        g = lambda k: A.tensor("%s%d" % (k, half)).cpu().numpy()
        q, zf = pd.propose(pos, half, 2.0, 5, 3)
        np.testing.assert_allclose(g("q"), q.reshape(g("q").shape), rtol=1e-14)
        dummy = np.zeros((T, W), np.int32)
        pd.accept(pos, lnl, lnpr, half, D["betas"], g("q").reshape(q.shape), g("zfac").reshape(zf.shape),
                  g("lnew").reshape(zf.shape), g("lle").reshape(zf.shape + (2,)), 5, 3, nacc if half == 0 else dummy)
    nswap = np.zeros((T, 2), np.int64)
    pd.swap(pos, lnl, lnpr, D["betas"], 5, 3, nswap)
    get = lambda k: A.tensor(k).cpu().numpy()
    np.testing.assert_array_equal(get("nswap"), nswap)          # exact; row 0 unused
    np.testing.assert_array_equal(get("naccept"), nacc)
    np.testing.assert_array_equal(get("pos_out"), pos)
    np.testing.assert_array_equal(get("lnl"), lnl)
    np.testing.assert_array_equal(get("lnpr"), lnpr)


add("pt_T3_W6_nd3", _pt_case, _pt_data, ["lfg_pt_propose", "lfg_pt_accept", "lfg_pt_swap"], verify=_pt_verify,
    short=E_WORKSPACE)


# ------------------------------------------------------------------ trees
def guarded_evaluator(A, tree, scratch=None):
    """an LnProbEvaluator whose tree arrays are const inputs of the allocator"""
    from lfit_python_amd import batch
    ev = batch.LnProbEvaluator(tree)
    ev.relocate(lambda k, t: A.inp("tree." + k, t.cpu().numpy()))
    if scratch is not None:
        ev.use_scratch(scratch)
    return ev


def _tree_data(kind):
    def build(oracle):
        from lfit_python_amd import batch, synthetic
        from lfit_python_amd.synthetic import phase_grid
        from tests import gp_trees
        from tests import test_gpu_pair_runscan as rs
        nsub = 1
        if kind in ("one65", "ragged", "rejected"):
            key = {"one65": ("grid", 65), "ragged": ("ragged", 0), "rejected": ("rejected", 65)}[kind]
            t, walk, bad, ref, rlle = rs._case(key, oracle)
        elif kind in ("one65_W1", "one65_W65"):     # k_setup's lane bounds: one walker, one past a wave
            t, walk8, _, _, _ = rs._case(("grid", 65), oracle)
            W = int(kind.split("W")[1])
            walk = walk8[:1].copy() if W == 1 else walk8[0] * (
                1.0 + 0.01 * np.random.default_rng(29).standard_normal((W, walk8.shape[1])))
            ref, rlle, _ = oracle.lnprob_batch(walk, t)
            bad = ~np.isfinite(ref)
        elif kind == "long":       # 513 / 40 / 70 points, three sub-bins: k_pair LONG or the two kernels
            nsub = 3
            rng = np.random.default_rng(3)
            m = synthetic.config_tree(1, 300, nsub=nsub)
            for lf, k in zip(m.leaves(), (513, 40, 70)):
                rs._set_lc(lf, *phase_grid(k), oracle, rng)
            t = batch.compile_tree(m, nsub=nsub)
            p0 = np.array(m.dynasty_par_vals)
            walk = p0 * (1.0 + 0.01 * np.random.default_rng(23).standard_normal((5, p0.size)))
            ref, rlle, _ = oracle.lnprob_batch(walk, t, nsub=nsub)
            bad = ~np.isfinite(ref)
        else:                      # GP trees: "cuts" E = 1, "tiny" E = 4
            m, nsub, walk = gp_trees.case(oracle, kind)
            t = batch.compile_tree(m, nsub=nsub)
            ref, rlle, _ = oracle.lnprob_batch(walk, t, nsub=nsub)
            gp_trees.check_case(kind, walk, ref)
            bad = ~np.isfinite(ref)
        assert (~bad).sum() >= min(3, len(ref))
        return dict(tree=t, walk=walk, bad=bad, ref=ref, rlle=rlle, nsub=nsub, oracle=oracle)
    return build


def _lnprob_case(A, D, short=0):
    L, t = lib(), D["tree"]
    W = D["walk"].shape[0]
    ev = guarded_evaluator(A, t)
    walk = A.inp("walkers", D["walk"])
    nb = L.lfg_workspace_size_tree(W, ctypes.byref(ev.ctree))
    events = (ctypes.c_void_p * 4)()    # LFG_NEV NULL entries: skipped
    rcs = []
    # a chi^2 tree's ln_prob needs lfg_workspace_size(W, E) (no candidates): one byte short of that is refused
    given = L.lfg_workspace_size(W, t.E) - 1 if short else nb
    for tag in ("full", "lnp_only", "timed", "timed_lnp_only"):
        lnp = A.out("lnp." + tag, (W,), f64())
        lle = A.out("lle." + tag, (W, t.E), f64()) if "only" not in tag else None
        ws = A.ws("ws." + tag, nb)
        if tag.startswith("timed"):
            rc = L.lfg_lnprob_timed(ptr(walk), W, ctypes.byref(ev.ctree), ptr(lnp), ptr(lle), ptr(ws), given,
                                    A.stream_ptr(), events)
            rcs.append(("lfg_lnprob_timed", rc))
        else:
            rc = L.lfg_lnprob(ptr(walk), W, ctypes.byref(ev.ctree), ptr(lnp), ptr(lle), ptr(ws), given,
                              A.stream_ptr())
            rcs.append(("lfg_lnprob", rc))
    lpr = A.out("lnprior", (W,), f64())
    ws = A.ws("ws.prior", nb)
    rcs.append(("lfg_lnprior", L.lfg_lnprior(ptr(walk), W, ctypes.byref(ev.ctree), ptr(lpr), ptr(ws), given,
                                             A.stream_ptr())))
    return rcs


def _lnprob_verify(D, A):
    get = lambda k: A.tensor(k).cpu().numpy()
    ok = ~D["bad"]
    for tag in ("full", "lnp_only", "timed", "timed_lnp_only"):
        _same(get("lnp." + tag), D["ref"], LNP_RTOL)
        np.testing.assert_array_equal(get("lnp." + tag), get("lnp.full"))
    for tag in ("full", "timed"):
        lle = get("lle." + tag)
        _same(lle[ok], D["rlle"][ok], LNP_RTOL)
        # the header: every lnlike_e element of a walker whose ln_prob is -inf is -inf or that
        # eclipse's ln_like; none is left unwritten (the poison check) or NaN
        assert not np.any(np.isnan(lle))
    lpr = get("lnprior")
    with np.errstate(invalid="ignore"):       # (rejected walkers: -inf - -inf, not compared)
        prior_ref = D["ref"] - D["rlle"].sum(1)
    _same(lpr[ok], prior_ref[ok], LNP_RTOL)
    assert np.all(np.isneginf(lpr[D["bad"]]) | np.isfinite(lpr[D["bad"]]))


for _kind in ("one65", "one65_W1", "one65_W65", "ragged", "long", "rejected", "cuts", "tiny"):
    add("lnprob_" + _kind, _lnprob_case, _tree_data(_kind), ["lfg_lnprob", "lfg_lnprior", "lfg_lnprob_timed"],
        verify=_lnprob_verify, both_layouts=True, short=E_WORKSPACE if _kind not in ("cuts", "tiny") else None)


def _predict_tree_case(A, D, short=0):
    L, t = lib(), D["tree"]
    W, ntot = D["walk"].shape[0], int(D["tree"].offsets[-1])
    ev = guarded_evaluator(A, t)
    walk = A.inp("walkers", D["walk"])
    nb = L.lfg_gp_predict_tree_workspace_size(W, ctypes.byref(ev.ctree))
    rcs = []
    for tag in ("all", "mean_only"):
        flux, var = (A.out(k + "." + tag, (W, ntot), f64()) if tag == "all" else None for k in ("flux", "var"))
        mean, st = A.out("mean." + tag, (W, ntot), f64()), A.out("status." + tag, (W,), i32())
        ws = A.ws("ws." + tag, nb)
        rcs.append(("lfg_gp_predict_tree", L.lfg_gp_predict_tree(ptr(walk), W, ctypes.byref(ev.ctree), ptr(flux),
                                                                 ptr(mean), ptr(var), ptr(st), ptr(ws), nb - short,
                                                                 A.stream_ptr())))
    return rcs


def _predict_tree_verify(D, A):
    get = lambda k: A.tensor(k).cpu().numpy()
    st = get("status.all")
    np.testing.assert_array_equal(st, get("status.mean_only"))
    np.testing.assert_array_equal(get("mean.all"), get("mean.mean_only"))
    assert np.array_equal(st != 0, D["bad"])
    for k in ("flux.all", "mean.all", "var.all"):
        v = get(k)
        assert np.all(np.isnan(v[D["bad"]])) and np.all(np.isfinite(v[~D["bad"]]))   # the header: NaN rows
    # the model flux y - res of the accepted walkers against the oracle's flux
    t, flux = D["tree"], get("flux.all")
    from tests import gp_trees
    o = D["oracle"]
    for w in np.nonzero(~D["bad"])[0][:2]:
        for e in range(t.E):
            sl = slice(t.offsets[e], t.offsets[e + 1])
            s, f = o.flux(gp_trees.eclipse_pars(t, e, D["walk"][w]), t.x[sl], t.w[sl], nsub=D["nsub"])
            assert s == 0 and np.max(np.abs(flux[w, sl] - f)) / np.max(np.abs(f)) < FLUX_RTOL


for _kind in ("cuts", "tiny"):
    add("gp_predict_tree_" + _kind, _predict_tree_case, _tree_data(_kind), ["lfg_gp_predict_tree"],
        verify=_predict_tree_verify, both_layouts=True, short=E_ARGS)


# ------------------------------------------------------------------ the stretch family
SEED, ASTRETCH, ITERS, WCHAIN = 7, 2.0, 3, 10
SHARDS = ((0, 2), (2, 3))     # (lo, n) of the two ranks' shards of a half of 5
FLAVOURS = {
    "separate": ["lfg_stretch_propose", "lfg_lnprob", "lfg_stretch_accept"],
    "dev": ["lfg_stretch_propose_dev", "lfg_stretch_accept_dev"],
    "lnprob_accept": ["lfg_stretch_lnprob_accept"],
    "step_half": ["lfg_stretch_step_half"],
    "step_half_spec": ["lfg_stretch_step_half_spec"],
    "shard": ["lfg_stretch_step_shard", "lfg_stretch_accept_regen"],
    "shard_spec": ["lfg_stretch_step_shard_spec", "lfg_stretch_accept_regen_spec"],
    "fold": ["lfg_stretch_step_shard_fold", "lfg_stretch_apply_verdicts"],
}


def _chain_data(kind):
    def build(oracle):
        D = dict(data_of("lnprob_" + kind, oracle))
        t = D["tree"]
        rng = np.random.default_rng(61)
        p0 = D["walk"][0]
        init = p0 * (1.0 + 2e-3 * rng.standard_normal((WCHAIN, p0.size)))
        lnp0, _, _ = oracle.lnprob_batch(init, t)
        assert np.isfinite(lnp0).sum() >= WCHAIN - 2
        D.update(init=init, oracle=oracle)
        return D
    return build


# where each speculative entry point takes spec_in (include/lfg.h)
SPEC_IN_ARG = {"lfg_stretch_step_half_spec": 12, "lfg_stretch_step_shard_spec": 12, "lfg_stretch_step_shard_fold": 16}


class _SpecSpy:
    """The library as an evaluator sees it, recording the spec_in each
    speculative call is really given: 1 means the call skips k_setup and
    reads the candidates the call before left in the scratch."""

    def __init__(self, L):
        self._L, self.spec_in = L, []

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if name not in SPEC_IN_ARG:
            return f

        def call(*args):
            self.spec_in.append(int(args[SPEC_IN_ARG[name]]))
            return f(*args)
        return call


def _chain_case(flavour):
    def fn(A, D, short=0):
        import torch
        L, t = lib(), D["tree"]
        W, ns, nd = WCHAIN, WCHAIN // 2, D["tree"].ndim
        ev0 = guarded_evaluator(A, t)
        T = ctypes.byref(ev0.ctree)
        nb = L.lfg_workspace_size_tree(ns, T)     # the header: every stretch entry point works in this
        sp = A.stream_ptr
        rank_flavour = flavour in ("shard_spec", "fold")
        R = len(SHARDS) if rank_flavour else 1
        # the ensemble (per rank where every rank applies the moves itself) and its first ln_prob
        pos = [A.io("pos%d" % r, D["init"]) for r in range(R)]
        lnp = [A.io("lnp%d" % r, np.zeros(W)) for r in range(R)]
        nacc = [A.io("naccept%d" % r, np.zeros(W, np.int32)) for r in range(R)]
        ws0 = A.ws("ws.first", L.lfg_workspace_size_tree(W, T))
        for r in range(R):
            assert L.lfg_lnprob(ptr(pos[r]), W, T, ptr(lnp[r]), None, ptr(ws0), ws0.numel(), sp()) == 0
        A.check()
        nws = len(SHARDS) if flavour in ("shard", "shard_spec", "fold") else 1
        wss = [A.ws("ws%d" % r, nb) for r in range(nws)]    # poisoned once: the scratch carries state by contract
        evs = [guarded_evaluator(_Shared(A, ev0), t, scratch=w) for w in wss]
        for e in evs:
            e.L = _SpecSpy(e.L)
        if flavour in ("shard", "shard_spec", "fold"):
            q = [A.out("q%d" % r, (n, nd), f64()) for r, (lo, n) in enumerate(SHARDS)]
            zf = [A.out("zfac%d" % r, (n,), f64()) for r, (lo, n) in enumerate(SHARDS)]
            lsh = [A.out("lnp_new%d" % r, (n,), f64()) for r, (lo, n) in enumerate(SHARDS)]
            vsh = [A.out("verdict%d" % r, (n,), f64()) for r, (lo, n) in enumerate(SHARDS)] if flavour == "fold" else None
            # The gathered vectors (what the exchange hands every rank) are the caller's own and
            # live outside the arena: all arena buffers are views of one tensor and share its
            # version counter, so a torch write into one of them between two calls would look to
            # the evaluator like a write to pos and make it drop its candidates.  They are const
            # inputs of the calls; gathered() checks them after use.
            gath = [torch.empty(ns, dtype=f64(), device=A.device) for h in (0, 1)]
        else:
            q, zf, lnew = A.out("q", (ns, nd), f64()), A.out("zfac", (ns,), f64()), A.out("lnp_new", (ns,), f64())
        step_dev = A.io("step_dev", np.zeros(1, np.int64)) if flavour == "dev" else None
        rcs = []
        rc = lambda name, code: rcs.append((name, code))
        V, kept = [None, None], [None, None]

        def unchanged(half, parts):
            same = torch.equal(gath[half].view(torch.int64), torch.cat(parts).view(torch.int64))   # bits: NaN verdicts
            assert same, "a call changed its gathered (const) input"
        for it in range(ITERS):
            for half in (0, 1):
                if flavour in ("separate", "dev", "lnprob_accept"):
                    if flavour == "dev":
                        rc("lfg_stretch_propose_dev", L.lfg_stretch_propose_dev(
                            ptr(pos[0]), W, nd, half, ASTRETCH, SEED, ptr(step_dev), ptr(q), ptr(zf), sp()))
                    else:
                        rc("lfg_stretch_propose", L.lfg_stretch_propose(ptr(pos[0]), W, nd, half, ASTRETCH, SEED, it,
                                                                        ptr(q), ptr(zf), sp()))
                    A.check()
                    if flavour == "lnprob_accept":
                        evs[0].lnprob_accept(q, pos[0], lnp[0], half, zf, SEED, it, nacc[0], lnp_new=lnew)
                    else:
                        rc("lfg_lnprob", L.lfg_lnprob(ptr(q), ns, T, ptr(lnew), None, ptr(wss[0]), nb, sp()))
                        A.check()
                        if flavour == "dev":
                            rc("lfg_stretch_accept_dev", L.lfg_stretch_accept_dev(
                                ptr(pos[0]), ptr(lnp[0]), W, nd, half, ptr(q), ptr(zf), ptr(lnew), SEED,
                                ptr(step_dev), ptr(nacc[0]), sp()))
                        else:
                            rc("lfg_stretch_accept", L.lfg_stretch_accept(ptr(pos[0]), ptr(lnp[0]), W, nd, half, ptr(q),
                                                                          ptr(zf), ptr(lnew), SEED, it, ptr(nacc[0]),
                                                                          sp()))
                elif flavour in ("step_half", "step_half_spec"):
                    evs[0].step_half(pos[0], lnp[0], half, ASTRETCH, SEED, it, q, zf, nacc[0], lnp_new=lnew,
                                     spec=flavour.endswith("spec"))
                elif flavour == "shard":
                    for r, (lo, n) in enumerate(SHARDS):
                        evs[r].step_shard(pos[0], half, ASTRETCH, SEED, it, lo, q[r], zf[r], lsh[r])
                        A.check()
                    gath[half].copy_(torch.cat(lsh))
                    rc("lfg_stretch_accept_regen", L.lfg_stretch_accept_regen(
                        ptr(pos[0]), ptr(lnp[0]), W, nd, half, ASTRETCH, SEED, it, ptr(gath[half]), ptr(nacc[0]), sp()))
                    A.check()
                    unchanged(half, lsh)
                elif flavour == "shard_spec":
                    for r, (lo, n) in enumerate(SHARDS):
                        evs[r].step_shard(pos[r], half, ASTRETCH, SEED, it, lo, q[r], zf[r], lsh[r], spec=True)
                        A.check()
                    gath[half].copy_(torch.cat(lsh))
                    for r, (lo, n) in enumerate(SHARDS):
                        evs[r].accept_regen(pos[r], lnp[r], half, ASTRETCH, SEED, it, gath[half], nacc[r], n)
                        A.check()
                    unchanged(half, lsh)
                else:   # fold
                    for r, (lo, n) in enumerate(SHARDS):
                        evs[r].step_shard_fold(pos[r], lnp[r], half, ASTRETCH, SEED, it, lo, q[r], zf[r], lsh[r],
                                               V[1 - half], vsh[r], nacc[r])
                        A.check()
                    if V[1 - half] is not None:
                        unchanged(1 - half, kept[1 - half])       # verdict_prev is a const input
                    gath[half].copy_(torch.cat(vsh))
                    kept[half] = [v.clone() for v in vsh]
                    V[half] = gath[half]
                A.check()
            if flavour == "dev":
                step_dev += 1     # the caller advances *step_dev after half 1
        if flavour == "fold":
            for r in range(R):
                evs[r].apply_verdicts(pos[r], lnp[r], 1, ASTRETCH, SEED, ITERS - 1, V[1], nacc[r])
            A.check()
        # every speculative half-step after the chain's first ran on the candidates the call
        # before left in this (poisoned, zeroed or left-over) scratch, on every rank
        if flavour in ("step_half_spec", "shard_spec", "fold"):
            for r, e in enumerate(evs):
                assert e.L.spec_in == [0] + [1] * (2 * ITERS - 1), (flavour, r, e.L.spec_in)
        return rcs
    return fn


class _Shared:
    """An allocator view that hands out the tree arrays another evaluator
    already placed (the ranks of one process share the tree)."""

    def __init__(self, A, ev):
        self.ev = ev

    def inp(self, name, array):
        return self.ev.arrays()[name[len("tree."):]]


def _chain_verify(D, A):
    get = lambda k: A.tensor(k).cpu().numpy()
    pos, lnp = get("pos0"), get("lnp0")
    ref, _, _ = D["oracle"].lnprob_batch(pos, D["tree"])
    _same(lnp, ref, LNP_RTOL)
    assert get("naccept0").sum() >= 3 and not np.array_equal(pos, D["init"])
    for r in (1,):
        if "pos%d" % r in A.bufs:     # every rank holds the same ensemble
            for k in ("pos", "lnp", "naccept"):
                np.testing.assert_array_equal(get("%s%d" % (k, r)), get(k + "0"))


for _kind in ("one65", "ragged"):
    for _fl, _cov in FLAVOURS.items():
        add("chain_%s_%s" % (_fl, _kind), _chain_case(_fl), _chain_data(_kind), _cov, verify=_chain_verify,
            both_layouts=True)


def _short_stretch(name):
    """One call of a scratch-taking stretch entry point with ws_bytes one byte
    below what it works in: lfg_workspace_size_tree(W/2, tree) for the calls
    that keep candidates (here with n = W/2: a smaller shard needs less), the
    chi^2 tree's lfg_workspace_size(W/2, E) for the others."""
    def fn(A, D, short=1):
        L, t = lib(), D["tree"]
        W, ns, nd = WCHAIN, WCHAIN // 2, D["tree"].ndim
        ev0 = guarded_evaluator(A, t)
        nb = L.lfg_workspace_size_tree(ns, ctypes.byref(ev0.ctree))
        plain = name in ("lfg_stretch_lnprob_accept", "lfg_stretch_step_half", "lfg_stretch_step_shard")
        need = L.lfg_workspace_size(ns, t.E) if plain else nb
        assert 0 < need <= nb
        ws = A.ws("ws", nb)
        ev = guarded_evaluator(_Shared(A, ev0), t, scratch=ws[:need - 1])
        pos, lnp = A.inp("pos", D["init"]), A.inp("lnp", np.zeros(W))
        nacc = A.inp("naccept", np.zeros(W, np.int32))
        qin, zin = A.inp("q_in", D["init"][:ns]), A.inp("zfac_in", np.zeros(ns))
        q, zf, lnew = A.out("q", (ns, nd), f64()), A.out("zfac", (ns,), f64()), A.out("lnp_new", (ns,), f64())
        vd = A.out("verdict", (ns,), f64())
        calls = {
            "lfg_stretch_lnprob_accept": lambda: ev.lnprob_accept(qin, pos, lnp, 0, zin, SEED, 0, nacc, lnp_new=lnew),
            "lfg_stretch_step_half": lambda: ev.step_half(pos, lnp, 0, ASTRETCH, SEED, 0, q, zf, nacc, lnp_new=lnew),
            "lfg_stretch_step_half_spec": lambda: ev.step_half(pos, lnp, 0, ASTRETCH, SEED, 0, q, zf, nacc,
                                                               lnp_new=lnew, spec=True),
            "lfg_stretch_step_shard": lambda: ev.step_shard(pos, 0, ASTRETCH, SEED, 0, 0, q, zf, lnew),
            "lfg_stretch_step_shard_spec": lambda: ev.step_shard(pos, 0, ASTRETCH, SEED, 0, 0, q, zf, lnew, spec=True),
            "lfg_stretch_accept_regen_spec": lambda: ev.accept_regen(pos, lnp, 0, ASTRETCH, SEED, 0, zin, nacc, ns),
            "lfg_stretch_step_shard_fold": lambda: ev.step_shard_fold(pos, lnp, 0, ASTRETCH, SEED, 0, 0, q, zf, lnew,
                                                                      None, vd, nacc),
        }
        with pytest.raises(RuntimeError, match=re.escape("%s failed with code %d" % (name, E_WORKSPACE))):
            calls[name]()
        return []
    return fn


SHORT_STRETCH = ("lfg_stretch_lnprob_accept", "lfg_stretch_step_half", "lfg_stretch_step_half_spec",
                 "lfg_stretch_step_shard", "lfg_stretch_step_shard_spec", "lfg_stretch_accept_regen_spec",
                 "lfg_stretch_step_shard_fold")


# ------------------------------------------------------------------ the tests
def _params(pred=lambda c: True):
    out = []
    for name, c in CASES.items():
        if pred(c):
            for lay in ((1, 0) if c.both_layouts else (1,)):
                out.append(pytest.param(name, lay, id="%s-%s" % (name, "pair" if lay else "two_kernel")))
    return out


def _run(case, A, D, short=0):
    rcs = case.fn(A, D, short) if short else case.fn(A, D)
    A.check()
    return rcs


def _plain(case, D, lay):
    """run (a), once per case and layout: checked against the oracle, its bytes kept"""
    key = (case.name, lay)
    if key not in _PLAIN:
        A = ag.Plain()
        rcs = _run(case, A, D)
        assert rcs is not None and all(rc == 0 for _, rc in rcs), rcs
        if case.verify:
            case.verify(D, A)
        _PLAIN[key] = A.result()
    return _PLAIN[key]


def _assert_same_bytes(got, want, label):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape, (label, k)
        if not np.array_equal(got[k], want[k]):
            first = int(np.nonzero(got[k] != want[k])[0][0])
            raise AssertionError("%s: output %r differs from the plain run's from byte %d of %d"
                                 % (label, k, first, want[k].size))


def _assert_no_poison(A, label, case=None, D=None):
    """every output element is written, but for those lfg.h says the call leaves alone: exactly those still
    hold the poison"""
    leave = case.unwritten(D) if case is not None and case.unwritten else {}
    for n in A.order:
        if A.bufs[n][0] == "out":
            left = A.poisoned(n)
            want = leave.get(n, np.zeros(left.shape, bool))
            bad = left != want
            assert not bad.any(), "%s: %d of %d elements of %r %s (first %s)" % (
                label, int(bad.sum()), left.size, n,
                "were never written" if (left & ~want).any() else "were written although lfg.h leaves them alone",
                tuple(int(v[0]) for v in np.nonzero(bad)))


@pytest.fixture(scope="module")
def arena():
    return ag.Arena()


@pytest.mark.parametrize("name,layout", _params(), indirect=["layout"])
def test_guarded_runs_match_plain(oracle, arena, name, layout):
    case = CASES[name]
    D = data_of(name, oracle)
    want = _plain(case, D, layout)
    for label, fill in (("scratch all-ones", ag.POISON), ("scratch zeroed", 0)):
        arena.reset(fill)
        rcs = _run(case, arena, D)
        assert all(rc == 0 for _, rc in rcs), rcs
        _assert_no_poison(arena, "%s (%s)" % (name, label), case, D)
        _assert_same_bytes(arena.result(), want, "%s (%s)" % (name, label))
    # (d): the scratch zone as another case's call left it
    names = list(CASES)
    other = CASES[names[(names.index(name) + 7) % len(names)]]
    arena.reset(ag.POISON)
    _run(other, arena, data_of(other.name, oracle))
    arena.reset(None)
    rcs = _run(case, arena, D)
    assert all(rc == 0 for _, rc in rcs), rcs
    _assert_no_poison(arena, "%s (left-over scratch)" % name, case, D)
    _assert_same_bytes(arena.result(), want, "%s (scratch left by %s)" % (name, other.name))


@pytest.mark.parametrize("name,layout", _params(), indirect=["layout"])
def test_guarded_runs_on_a_side_stream(oracle, arena, name, layout):
    """nothing depends on the default stream: the library takes the stream as an argument"""
    import torch
    case = CASES[name]
    D = data_of(name, oracle)
    want = _plain(case, D, layout)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        arena.reset(ag.POISON)
        rcs = _run(case, arena, D)
        assert all(rc == 0 for _, rc in rcs), rcs
        _assert_no_poison(arena, name, case, D)
        _assert_same_bytes(arena.result(), want, "%s (side stream)" % name)
    torch.cuda.synchronize()


def _assert_all_poisoned(A, label):
    for n in A.order:
        role = A.bufs[n][0]
        if role in ("out", "ws"):
            raw = A.raw(n)
            assert bool((raw == ag.POISON).all()), "%s: %r was written although the call was refused" % (label, n)


@pytest.mark.parametrize("name,layout", _params(lambda c: c.short is not None), indirect=["layout"])
def test_one_byte_short_scratch_is_refused_before_any_launch(oracle, arena, name, layout):
    case = CASES[name]
    arena.reset(ag.POISON)
    rcs = _run(case, arena, data_of(name, oracle), short=1)
    assert rcs and all(rc == case.short for _, rc in rcs), rcs
    _assert_all_poisoned(arena, name)


@pytest.mark.parametrize("entry", SHORT_STRETCH)
@pytest.mark.parametrize("kind", ["one65", "ragged"])
def test_one_byte_short_scratch_is_refused_by_the_stretch_family(oracle, arena, entry, kind):
    D = data_of("chain_step_half_" + kind, oracle)
    arena.reset(ag.POISON)
    _short_stretch(entry)(arena, D)
    arena.check()
    _assert_all_poisoned(arena, entry)


@pytest.mark.parametrize("kind", ["one65", "ragged"])
@pytest.mark.parametrize("lay", [1, 0])
def test_every_stretch_path_gives_the_same_chain(oracle, kind, lay):
    """the header's "same chain as": the eight ways through the stretch family end bit-identical"""
    L = lib()
    prev = L.lfg_set_layout(lay)
    try:
        ends = {}
        for fl in FLAVOURS:
            name = "chain_%s_%s" % (fl, kind)
            r = _plain(CASES[name], data_of(name, oracle), lay)
            ends[fl] = {k: r[k + "0"] for k in ("pos", "lnp", "naccept")}
        for fl, e in ends.items():
            _assert_same_bytes(e, ends["separate"], "%s against separate kernels (%s)" % (fl, kind))
    finally:
        L.lfg_set_layout(prev)


def test_arena_reports_a_stray_write():
    """the helper itself: a byte written one past a payload, or into a const input, is reported"""
    import torch
    A = ag.Arena(nbytes=16 * 1024 * 1024)
    x = A.inp("x", np.arange(5.0))
    out = A.out("out", (3,), torch.float64)
    assert out.data_ptr() % 256 == 0 and out.data_ptr() % 512 != 0
    A.check()
    assert A.poisoned("out").all()
    out[1] = 2.0
    assert list(A.poisoned("out")) == [True, False, True]
    A.raw("out")    # (a view; the write below goes through the arena's own memory)
    k = A.base + A.spans[-1][2] + 24
    A.mem[k] = 0
    with pytest.raises(AssertionError, match="after buffer 'out': first at byte 24"):
        A.check()
    A.mem[k] = ag.GUARD_BYTE
    A.check()
    x[2] = -1.0
    with pytest.raises(AssertionError, match="const input 'x' was changed"):
        A.check()


# lfg.h's functions without a [dev] pointer: size functions, event helpers, switches
HOST_ONLY = {"lfg_workspace_size", "lfg_workspace_size_tree", "lfg_pt_workspace_size",
             "lfg_gp_predict_workspace_size", "lfg_gp_sample_workspace_size", "lfg_gp_predict_tree_workspace_size",
             "lfg_component_workspace_size", "lfg_event_create", "lfg_event_destroy", "lfg_event_elapsed_ms",
             "lfg_version", "lfg_layout", "lfg_set_layout"}


def test_every_entry_point_has_a_guarded_case():
    """a new entry point of lfg.h cannot be added without a guarded case"""
    covered = set()
    for c in CASES.values():
        covered.update(c.covers)
    declared = set(declared_functions())
    assert HOST_ONLY <= declared
    assert covered == declared - HOST_ONLY, (sorted(declared - HOST_ONLY - covered), sorted(covered - declared))
    # and every scratch-taking one its one-byte-short run
    short = {e for c in CASES.values() if c.short is not None for e in c.covers} | set(SHORT_STRETCH)
    text = re.sub(r"/\*.*?\*/", "", open(__import__("tests.test_native_abi", fromlist=["HEADER"]).HEADER).read(),
                  flags=re.S)
    takes_ws = set(re.findall(r"\b(lfg_[a-z_]+)\s*\([^;]*?size_t ws_bytes", text))
    assert len(takes_ws) >= 15 and takes_ws <= short, takes_ws - short
