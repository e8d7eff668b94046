"""GPU: chain_prod.txt's numbers read on the device (include/lfg_chainparse.h,
MODEL_SPEC section 18) against Python's float() (tests/chainparse_cases.py),
in guarded buffers (tests/abi_guard.py): the token lists of the CPU test, the
texts at the kernels' seams and at every alignment, raggedness, the memory
contract, refusals, the round trip through lfg_chain_text, and the Python
layer up to fit_summary.

Every value comparison is equality of the 8 bytes, NaN against NaN.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import abi_guard as ag
from tests import chainparse_cases as cc
from tests import chaintext_double as ct
from tests.abi_guard import ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from lfit_python_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def arena():
    return ag.Arena(nbytes=96 * 1024 * 1024)


@pytest.fixture(scope="module")
def tile(L):
    return int(L.lfg_chain_parse_tile_bytes())


def call(L, A, text, ncol, skip=0, extra_rows=0, count_only=False, ws_short=0, rows_short=0):
    """both entry points in allocator A's buffers: the text in a block of
    exactly its size (read from byte `skip` on), `out` of exactly rows +
    extra_rows rows, poisoned -> (rc of count, rc of parse, info after count,
    info after parse, out as float64 [rows + extra_rows][ncol])"""
    import torch
    raw = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    n = raw.size - skip
    t = A.inp("text", raw) if raw.size else None
    info = A.out("info", 8, torch.int64)
    need = L.lfg_chain_parse_workspace_size(n)
    assert need > 0
    ws = A.ws("ws", need)
    tp = ctypes.c_void_p(t.data_ptr() + skip) if t is not None else ctypes.c_void_p(ws.data_ptr())
    rc1 = L.lfg_chain_parse_count(tp, n, ncol, ptr(info), ptr(ws), need - ws_short, A.stream_ptr())
    A.check()
    i1 = info.cpu().numpy().copy()
    if rc1 != 0 or count_only:
        return rc1, None, i1, None, None
    rows = int(i1[0])
    cap = max(rows + extra_rows - rows_short, 0)
    out = A.out("out", (max(rows + extra_rows, 1), ncol), torch.float64)
    rc2 = L.lfg_chain_parse(tp, n, ncol, ptr(out), cap, ptr(info), ptr(ws), need, A.stream_ptr())
    A.check()
    return rc1, rc2, i1, info.cpu().numpy().copy(), out.cpu().numpy()[:rows + extra_rows]


def good(got, want, refused=0):
    """a text read without a complaint: the values, info, and out untouched behind the rows"""
    rc1, rc2, i1, i2, out = got
    rows, ncol = want.shape
    assert rc1 == 0 and rc2 == 0
    assert list(i1) == [rows, rows * ncol, 0, 0, 0, -1, 0, 0], i1
    assert list(i2) == [rows, rows * ncol, 0, refused, 0, -1, 0, 0], i2
    bad = cc.same(out[:rows], want)
    assert bad.size == 0, (bad[:5], out[:rows].reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])
    assert (out[rows:].view(np.uint8) == ag.POISON).all()   # out beyond rows * ncol is not written


def test_sizes(L, tile):
    from lfit_python_amd import _native, chainparse
    assert tile == chainparse.twin().lfg_cpu_chain_parse_tile_bytes() and tile % 16 == 0
    assert L.lfg_chain_parse_workspace_size(-1) == 0 and L.lfg_chain_parse_workspace_size(2 ** 47) == 0
    assert L.lfg_chain_parse_workspace_size(0) > 0
    assert L.lfg_chain_parse_workspace_size(10 * tile) % 256 == 0
    assert _native.CHAIN_PARSE_MAX_NCOL >= _native.CHAIN_TEXT_MAX_NDIM + 2 and _native.CHAIN_PARSE_MAX_TOKEN >= 32
    assert cc.MAX_TOKEN == _native.CHAIN_PARSE_MAX_TOKEN and cc.MAX_NCOL == _native.CHAIN_PARSE_MAX_NCOL


@pytest.mark.parametrize("name", ["roundtrip", "digits17_19", "ties", "edges"])
def test_token_lists(L, arena, name):
    """every token the rule says the device decides: nothing refused, every value float()'s"""
    text, want, _ = cc.list_case(name)
    arena.reset()
    good(call(L, arena, text, 1, extra_rows=3), want)


def test_token_lists_as_rows_of_seven(L, arena):
    text, want, _ = cc.list_case("digits17_19", 7)
    arena.reset()
    good(call(L, arena, text, 7, extra_rows=1), want)


def test_long_tokens_are_right_or_refused(L, arena):
    text, want, tokens = cc.list_case("long")
    arena.reset()
    rc1, rc2, i1, i2, out = call(L, arena, text, 1)
    assert rc1 == 0 and rc2 == 0 and list(i2[[0, 1, 2, 4, 5]]) == [len(tokens), len(tokens), 0, 0, -1]
    may = np.array([cc.may_refuse(t) for t in tokens])
    got = out.reshape(-1)
    wrong = cc.same(got, want.reshape(-1))
    # a refused field holds NaN; what differs from float() must be such a field the rule allows
    assert np.isnan(got[wrong]).all() and may[wrong].all(), [tokens[i] for i in wrong if not may[i]][:5]
    assert 0 < int(i2[3]) <= int(may.sum())
    assert int(i2[3]) >= wrong.size and int(i2[3]) - wrong.size <= int(np.isnan(want).sum())


def test_structure(L, arena, tile):
    for name, text, ncol, want in cc.structure_cases(tile):
        if ncol is None:
            continue   # (finding ncol is the Python layer's: below)
        arena.reset()
        good(call(L, arena, text, ncol, extra_rows=2), want)


def test_every_seam_and_alignment(L, arena, tile):
    """the 3-tile text behind 0 .. MAX_TOKEN + 1 blanks, read from every
    alignment modulo 16 of the base pointer"""
    for shift in range(cc.MAX_TOKEN + 2):
        text, want = cc.shifted(tile, shift)
        arena.reset()
        good(call(L, arena, b" " * 16 + text, 2, skip=(5 * shift) % 17, extra_rows=1), want)


def test_ragged_rows(L, arena):
    for name, text, ncol, row in cc.ragged_cases():
        arena.reset()
        rc1, rc2, i1, i2, out = call(L, arena, text, ncol, extra_rows=2)
        assert rc1 == 0 and rc2 == 0, name
        assert i1[4] != 0 and i1[5] == row, (name, i1)
        assert list(i2) == list(i1), name              # parse adds nothing
        assert (out.view(np.uint8) == ag.POISON).all(), name   # and writes nothing but info


def test_bad_tokens(L, arena):
    for tok, text, row in cc.bad_files():
        arena.reset()
        rc1, rc2, i1, i2, out = call(L, arena, text, 3)
        assert rc1 == 0 and rc2 == 0
        assert list(i1) == [5, 15, 0, 0, 0, -1, 0, 0], (tok, i1)
        assert list(i2) == [5, 15, 1, 0, 0, row, 0, 0], (tok, i2)
        col = {0: 0, 2: 1, 4: 2}[row]
        assert np.isnan(out[row, col]) and np.isnan(out).sum() == 1, tok


def test_results_do_not_depend_on_ws_or_out(L, tile):
    """ws poisoned, zeroed, and left over from a different text: equal results"""
    text, want = cc.exact_size(3 * tile + 5, 3, 99)
    other, _ = cc.exact_size(5 * tile, 7, 98)
    A = ag.Arena(nbytes=32 * 1024 * 1024)
    seen = []
    for fill in (ag.POISON, 0, None):
        if fill is None:
            A.reset(ag.POISON)
            call(L, A, other, 7)
        A.reset(fill)
        got = call(L, A, text, 3, extra_rows=1)
        good(got, want)
        seen.append((got[2].tobytes(), got[3].tobytes(), got[4].tobytes()))
    assert seen[0] == seen[1] == seen[2]
    # parse a second time with the same ws: the same info and values
    import torch
    A.reset(ag.POISON)
    raw = A.inp("text", np.frombuffer(text, np.uint8).copy())
    info = A.out("info", 8, torch.int64)
    need = L.lfg_chain_parse_workspace_size(len(text))
    ws = A.ws("ws", need)
    out = A.out("out", want.shape, torch.float64)
    assert L.lfg_chain_parse_count(ptr(raw), len(text), 3, ptr(info), ptr(ws), need, A.stream_ptr()) == 0
    for _ in range(2):
        assert L.lfg_chain_parse(ptr(raw), len(text), 3, ptr(out), want.shape[0], ptr(info), ptr(ws), need,
                                 A.stream_ptr()) == 0
        A.check()
        assert list(info.cpu().numpy()) == [want.shape[0], want.size, 0, 0, 0, -1, 0, 0]
        assert cc.same(out.cpu().numpy(), want).size == 0


def test_short_capacity_is_found_on_the_device(L, arena, tile):
    text, want = cc.exact_size(tile + 3, 3, 5)
    arena.reset()
    rc1, rc2, i1, i2, out = call(L, arena, text, 3, rows_short=1)
    assert rc1 == 0 and rc2 == 0 and i2[6] == 1 and list(i2[:6]) == [want.shape[0], want.size, 0, 0, 0, -1]
    assert (out.view(np.uint8) == ag.POISON).all()


def test_refused_arguments_write_nothing(L, arena, tile):
    import torch
    text, want = cc.exact_size(tile, 3, 6)
    n = len(text)
    arena.reset()
    raw = arena.inp("text", np.frombuffer(text, np.uint8).copy())
    info = arena.out("info", 8, torch.int64)
    need = L.lfg_chain_parse_workspace_size(n)
    ws = arena.ws("ws", need)
    out = arena.out("out", want.shape, torch.float64)
    st = arena.stream_ptr()
    rows = want.shape[0]
    from lfit_python_amd import _native
    E = -1   # LFG_E_ARGS
    for a in ((None, n, 3, ptr(info), ptr(ws), need), (ptr(raw), -1, 3, ptr(info), ptr(ws), need),
              (ptr(raw), n, 0, ptr(info), ptr(ws), need), (ptr(raw), n, _native.CHAIN_PARSE_MAX_NCOL + 1, ptr(info),
                                                           ptr(ws), need),
              (ptr(raw), n, 3, None, ptr(ws), need), (ptr(raw), n, 3, ptr(info), None, need),
              (ptr(raw), n, 3, ptr(info), ptr(ws), need - 1), (ptr(raw), 2 ** 47, 3, ptr(info), ptr(ws), need)):
        assert L.lfg_chain_parse_count(*a, st) == E, a
        assert L.lfg_chain_parse(a[0], a[1], a[2], ptr(out), rows, a[3], a[4], a[5], st) == E, a
    for o, r in ((None, rows), (ptr(out), -1)):
        assert L.lfg_chain_parse(ptr(raw), n, 3, o, r, ptr(info), ptr(ws), need, st) == E
    arena.check()
    assert arena.poisoned("info").all() and arena.poisoned("out").all()
    assert (arena.raw("ws") == ag.POISON).all()


def test_side_stream(L, tile):
    import torch
    text, want = cc.exact_size(2 * tile + 1, 3, 8)
    A = ag.Plain()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = call(L, A, text, 3)
    good(got, want)


@pytest.mark.parametrize("steps,W,ndim", [(7, 5, 18), (2, 3, 87)])
def test_round_trip_on_the_device(L, steps, W, ndim):
    """lfg_chain_text of a chain with non-finite values sprinkled in, parsed
    back on the device: bit-equal, and the walker numbers are regular"""
    import torch
    from lfit_python_amd import chaintext
    chain, lnp = ct.block_case(steps, W, ndim, seed=3)
    chain, lnp = chain.copy(), -np.abs(ct.device_ok(lnp))
    lnp[np.abs(lnp) >= 1e13] = -0.5     # ('%f' of more than 19 digits may be refused)
    chain.reshape(-1)[::11] = np.tile([np.inf, -np.inf, np.nan, -0.0], chain.size)[:chain.reshape(-1)[::11].size]
    lnp[0, 0], lnp[-1, -1] = -np.inf, np.nan
    dc, dl = torch.from_numpy(chain).cuda(), torch.from_numpy(lnp).cuda()
    text, nbytes = chaintext.device_rows(dc, dl)
    total, refused = nbytes.tolist()
    assert refused == 0
    from lfit_python_amd import chainparse
    out, info = chainparse.parse_device(text[:total], ndim + 2)
    assert info[:6] == [steps * W, steps * W * (ndim + 2), 0, 0, 0, -1]
    got = out.cpu().numpy().reshape(steps, W, ndim + 2)
    assert (got[:, :, 0] == np.arange(W)).all()
    assert cc.same(got[:, :, 1:-1], chain).size == 0
    assert cc.same(got[:, :, -1], np.array([[float("%f" % v) for v in r] for r in lnp])).size == 0


# ---- the Python layer --------------------------------------------------------------------------
def test_parse_text_on_the_device(tile):
    import torch
    from lfit_python_amd import chainparse
    for name, text, ncol, want in cc.structure_cases(tile)[:16]:
        for data in (text, torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()):
            out = chainparse.parse_text(data, ncol, device="cuda")
            assert out.is_cuda and tuple(out.shape) == want.shape, name
            assert cc.same(out.cpu().numpy(), want).size == 0, name
    for name, text, ncol, row in cc.ragged_cases():
        with pytest.raises(ValueError, match="row %d " % row):
            chainparse.parse_text(text, ncol, device="cuda")
    for tok, text, row in cc.bad_files()[:12]:
        with pytest.raises(ValueError, match="row %d " % row):
            chainparse.parse_text(text, 3, device="cuda")


def test_one_refused_field_falls_back_to_the_twin():
    from lfit_python_amd import chainparse
    toks = ["1.5", "2.5", "9007199254740993.0000000000001", "-3", "0." + "0" * 70 + "1", "4"]
    text, want = cc.table(toks, 3)
    _, info = chainparse.parse_device(__import__("torch").from_numpy(np.frombuffer(text, np.uint8).copy()).cuda(), 3)
    assert info[3] >= 1 and info[2] == 0
    out = chainparse.parse_text(text, device="cuda")
    assert out.is_cuda and cc.same(out.cpu().numpy(), want).size == 0


@pytest.fixture(scope="module")
def chain_file(tmp_path_factory):
    from lfit_python_amd import sampler
    chain, lnp = ct.block_case(40, 12, 6, seed=11)
    chain = 1.0 + 1e-3 * np.random.default_rng(5).standard_normal(chain.shape) + np.arange(6)
    lnp = -np.abs(ct.device_ok(lnp)) % 1e6
    path = str(tmp_path_factory.mktemp("chainparse") / "chain_prod.txt")
    names = ["p%d" % i for i in range(6)]
    sampler.write_chain(path, names, chain, lnp)
    return path, names, chain, lnp


def test_read_chain_on_the_device_and_chainstats(chain_file):
    from lfit_python_amd import chainparse, chainstats, sampler
    path, names, chain, lnp = chain_file
    dev, got_names = chainparse.read_chain(path, device="cuda")
    assert dev.is_cuda and tuple(dev.shape) == (40, 12, 7) and got_names == names + ["ln_prob"]
    host = sampler.read_chain(path)                       # [W][steps][7]
    assert cc.same(dev.cpu().numpy(), host.transpose(1, 0, 2)).size == 0
    assert cc.same(host[:, :, :6].transpose(1, 0, 2), chain).size == 0
    a = chainstats.stats(dev, quantiles=(0.16, 0.5, 0.84), rhat=True)
    b = chainstats.stats(host, quantiles=(0.16, 0.5, 0.84), rhat=True, walker_major=True)
    for k in ("n", "n_bad", "min", "max", "quant", "ostat"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    # the same [steps][W] view at other strides: include/lfg_chain.h fixes the order of
    # summation by (step, walker), not by address, so the moments are equal as well
    for k in ("mean", "m2", "rhat"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_fit_summary_reads_on_the_device(tmp_path, monkeypatch, capsys):
    """python -m lfit_python_amd.fit_summary on a small written chain: the same
    modparams.csv through the device reader as through the host reader"""
    from lfit_python_amd import chainparse, cvmodel, fit_summary, sampler
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_test_data", "mcmc_input.dat")
    model = cvmodel.construct_model(golden)
    names = list(model.dynasty_par_names)
    rng = np.random.default_rng(13)
    x = np.array(model.dynasty_par_vals) * (1.0 + 1e-3 * rng.normal(size=(12, 40, len(names))))
    path = str(tmp_path / "chain_prod.txt")
    sampler.write_chain(path, names, x, -1e3 * rng.random((12, 40)))
    seen = []
    real = chainparse.read_chain
    monkeypatch.setattr(chainparse, "read_chain", lambda *a, **k: (seen.append(k), real(*a, **k))[1])
    outs = []
    for route in (True, False):
        monkeypatch.setattr(chainparse, "DEVICE_ROUTE", route)
        d = tmp_path / ("dev" if route else "host")
        d.mkdir()
        assert fit_summary.main([path, golden, "--dir", str(d)]) == 0
        outs.append(open(os.path.join(str(d), "modparams.csv"), "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 50
    assert seen == [{"device": "cuda"}, {}]     # the device route once, the host reader's own parse once
