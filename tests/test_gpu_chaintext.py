"""GPU: chain_prod.txt's rows from the device (include/lfg_chaintext.h,
MODEL_SPEC section 17) against Python's own formatting (tests/
chaintext_double.py), in guarded buffers (tests/abi_guard.py): the value
lists of the CPU test, the shapes at the kernels' seams, strided views, the
memory contract, refusals, and the Python layer up to run_mcmc_save.

Every comparison is byte equality.
"""
import ctypes

import numpy as np
import pytest

from tests import abi_guard as ag
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


def call(L, A, buf, lbuf, steps, W, ndim, sld, wld, lsld, lwld, off=0, loff=0, walker0=0, out_short=0, ws_short=0,
         out_shift=0):
    """lfg_chain_text in allocator A's buffers: `out` of exactly the bound
    (shifted by out_shift bytes for an unaligned start), poisoned
    -> (rc, bytes up to the total, [total, refused], the rest of out)"""
    import torch
    bound = L.lfg_chain_text_bound(steps, W, ndim, walker0)
    assert bound >= 0
    chain = A.inp("chain", buf)
    lnp = A.inp("lnp", lbuf)
    out = A.out("out", bound + out_shift, torch.uint8)
    nb = A.out("nbytes", 2, torch.int64)
    need = L.lfg_chain_text_workspace_size(steps, W, ndim)
    assert need > 0
    ws = A.ws("ws", need)
    rc = L.lfg_chain_text(ctypes.c_void_p(chain.data_ptr() + 8 * off), steps, W, ndim, sld, wld,
                          ctypes.c_void_p(lnp.data_ptr() + 8 * loff), lsld, lwld, walker0,
                          ctypes.c_void_p(out.data_ptr() + out_shift), bound - out_short, ptr(nb), ptr(ws),
                          need - ws_short, A.stream_ptr())
    A.check()
    n = nb.cpu().numpy()
    host = out.cpu().numpy()
    if rc != 0:
        return rc, b"", n, host
    total = int(n[0])
    assert 0 <= total <= bound
    return rc, host[out_shift:out_shift + total].tobytes(), n, np.concatenate([host[:out_shift], host[out_shift + total:]])


def flat_call(L, A, chain, lnp, walker0=0, **kw):
    steps, W, ndim = chain.shape
    return call(L, A, chain.reshape(-1), lnp.reshape(-1), steps, W, ndim, max(1, W * ndim), ndim, max(1, W), 1,
                walker0=walker0, **kw)


def check(got, want, rest=None, refused=0):
    rc, data, n, tail = got
    assert rc == 0
    assert list(n) == [len(want), refused]
    assert data == want, ct.first_difference(data, want)
    assert (tail == ag.POISON).all()   # bytes of out at and beyond the total are not written


def test_sizes(L):
    from lfit_python_amd import _native
    assert L.lfg_chain_text_tile_rows(1) == 256 and L.lfg_chain_text_tile_rows(18) == 53
    assert L.lfg_chain_text_tile_rows(87) == 11 and L.lfg_chain_text_tile_rows(_native.CHAIN_TEXT_MAX_NDIM) == 1
    assert L.lfg_chain_text_tile_rows(0) == 0 and L.lfg_chain_text_tile_rows(_native.CHAIN_TEXT_MAX_NDIM + 1) == 0
    assert L.lfg_chain_text_bound(0, 5, 3, 0) == 0 and L.lfg_chain_text_bound(5, 0, 3, 0) == 0
    assert L.lfg_chain_text_bound(2, 3, 1, 0) == 6 * (4 + 25 + 29)
    assert L.lfg_chain_text_bound(2, 3, 1, 9998) == 6 * (5 + 25 + 29)
    for bad in ((-1, 3, 1, 0), (2, -3, 1, 0), (2, 3, 0, 0), (2, 3, 1024, 0), (2, 3, 1, -1), (2 ** 62, 2 ** 10, 1, 0)):
        assert L.lfg_chain_text_bound(*bad) == -1
    assert L.lfg_chain_text_workspace_size(2, 3, 0) == 0 and L.lfg_chain_text_workspace_size(-2, 3, 1) == 0
    assert L.lfg_chain_text_workspace_size(0, 3, 1) > 0


@pytest.mark.parametrize("name", sorted(ct.LISTS))
def test_value_lists(L, arena, name):
    """every value of the CPU test's lists as a chain value and as a ln_prob
    (2^63 and beyond replaced there); nothing is refused"""
    chain, lnp, want = ct.column_case(name, True)
    arena.reset()
    check(flat_call(L, arena, chain, lnp), want)


# rows at the seams: none, one, around a wave, and one past a workgroup's tile
@pytest.mark.parametrize("ndim", [1, 18, 87])
def test_rows_at_the_seams(L, arena, ndim):
    tile = L.lfg_chain_text_tile_rows(ndim)
    for rows in (1, 63, 64, 65, tile, tile + 1, 3 * tile + 1):
        chain, lnp = ct.block_case(rows, 1, ndim, seed=rows)
        arena.reset()
        check(flat_call(L, arena, chain, lnp), ct.rows(chain, lnp))


@pytest.mark.parametrize("steps,W,ndim,walker0", [(5, 37, 18, 0), (3, 70, 1, 9960), (2, 130, 87, 9990),
                                                  (7, 3, 5, 99998), (2, 2, 1023, 0), (4, 65, 18, 123456789012)])
def test_walkers_not_a_multiple_of_64_and_the_walker_field(L, arena, steps, W, ndim, walker0):
    """W off the wave; walker0 + k crossing 9 999 -> 10 000 inside a step"""
    chain, lnp = ct.block_case(steps, W, ndim, seed=7)
    arena.reset()
    check(flat_call(L, arena, chain, lnp, walker0), ct.rows(chain, lnp, walker0))


@pytest.mark.parametrize("steps,W", [(0, 5), (5, 0), (0, 0)])
def test_no_rows(L, arena, steps, W):
    arena.reset()
    rc, data, n, tail = call(L, arena, np.zeros(4), np.zeros(4), steps, W, 3, 15, 3, 5, 1)
    assert rc == 0 and data == b"" and list(n) == [0, 0]


def test_strided_views(L, arena):
    """the cold level of a tempered chain [steps][T][W] and a thinned chain;
    in either, the last element read is the buffer's last"""
    chain, lnp = ct.block_case(6, 20, 3, seed=1)
    c4, l4 = chain.reshape(6, 4, 5, 3), lnp.reshape(6, 4, 5)
    buf, lbuf = chain.reshape(-1), lnp.reshape(-1)
    arena.reset()
    got = call(L, arena, buf, lbuf, 6, 5, 3, 60, 3, 20, 1, off=45, loff=15)     # level 3 of 4
    check(got, ct.rows(c4[:, 3], l4[:, 3]))
    arena.reset()
    got = call(L, arena, buf[:30 + 5 * 60 + 4 * 3 + 3], lbuf[:10 + 5 * 20 + 4 + 1], 6, 5, 3, 60, 3, 20, 1,
               off=30, loff=10)                                                 # level 2: the blocks end with it
    check(got, ct.rows(c4[:, 2], l4[:, 2]))
    arena.reset()
    got = call(L, arena, buf, lbuf, 2, 20, 3, 180, 3, 60, 1, off=120, loff=40)  # steps 2 and 5
    check(got, ct.rows(chain[2::3], lnp[2::3]))
    # a walker-major chain [W][steps][ndim] with ln_prob [W][steps]
    wm, lwm = np.ascontiguousarray(chain.transpose(1, 0, 2)), np.ascontiguousarray(lnp.T)
    arena.reset()
    got = call(L, arena, wm.reshape(-1), lwm.reshape(-1), 6, 20, 3, 3, 18, 1, 6)
    check(got, ct.rows(chain, lnp))


def test_unaligned_out(L, arena):
    """`out` at every offset modulo 16: the aligned wide stores and the
    ragged head and tail of every tile"""
    chain, lnp = ct.block_case(130, 1, 18, seed=3)
    want = ct.rows(chain, lnp)
    for shift in (1, 2, 3, 5, 8, 13, 15):
        arena.reset()
        check(flat_call(L, arena, chain, lnp, out_shift=shift), want)


def test_scratch_contents_do_not_matter(L, arena):
    chain, lnp = ct.block_case(9, 37, 18, seed=4)
    want = ct.rows(chain, lnp)
    for fill in (ag.POISON, 0, None, None):
        arena.reset(fill)
        check(flat_call(L, arena, chain, lnp), want)
    arena.reset()


def test_short_buffers_and_bad_arguments_are_refused_with_nothing_written(L, arena):
    chain, lnp = ct.block_case(9, 37, 18, seed=4)
    for kw in (dict(out_short=1), dict(ws_short=1)):
        arena.reset()
        rc, _, n, host = flat_call(L, arena, chain, lnp, **kw)
        assert rc == -1 and (host == ag.POISON).all() and (n == -1).all()
        assert (arena.raw("ws").cpu().numpy() == ag.POISON).all()
    for a in (dict(sld=0), dict(wld=0), dict(lsld=0), dict(lwld=0), dict(ndim=0), dict(walker0=-1)):
        arena.reset()
        p = dict(steps=9, W=37, ndim=18, sld=37 * 18, wld=18, lsld=37, lwld=1, walker0=0)
        p.update(a)
        import torch
        out = arena.out("out", 1 << 20, torch.uint8)
        nb = arena.out("nbytes", 2, torch.int64)
        ws = arena.ws("ws", 4096)
        c, l = arena.inp("chain", chain), arena.inp("lnp", lnp)
        rc = L.lfg_chain_text(ptr(c), p["steps"], p["W"], p["ndim"], p["sld"], p["wld"], ptr(l), p["lsld"], p["lwld"],
                              p["walker0"], ptr(out), 1 << 20, ptr(nb), ptr(ws), 4096, arena.stream_ptr())
        arena.check()
        assert rc == -1 and arena.poisoned("out").all() and arena.poisoned("nbytes").all()


def test_side_stream(L, arena):
    import torch
    chain, lnp = ct.block_case(9, 37, 18, seed=5)
    arena.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = flat_call(L, arena, chain, lnp)
    torch.cuda.current_stream().wait_stream(side)
    check(got, ct.rows(chain, lnp))


def test_only_two_to_the_63_and_beyond_is_refused(L, arena):
    """the refused rows are counted, every other row of the call stands;
    through format_rows those rows are the oracle's as well"""
    import torch
    from lfit_python_amd import chaintext
    big = np.array(ct.refused())
    chain, lnp = ct.block_case(4, big.size, 3, seed=6)
    lnp = lnp.copy()
    lnp[1] = big
    lnp[3, 0] = big[0]
    arena.reset()
    rc, data, n, tail = flat_call(L, arena, chain, lnp)
    assert rc == 0 and list(n)[1] == big.size + 1
    shown = np.where(np.isfinite(lnp) & (np.abs(lnp) >= ct.TWO63), 0.25, lnp)
    want = ct.rows(chain, shown).split(b"\n")
    got = data.split(b"\n")
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        s, k = divmod(r, big.size)
        if r < lnp.size and shown[s, k] != lnp[s, k]:
            assert g == w[:-len(b"0.250000")] + b"?"
        else:
            assert g == w
    out = chaintext.format_rows(torch.as_tensor(chain.copy()).cuda(), torch.as_tensor(lnp).cuda())
    assert out == ct.rows(chain, lnp)


def test_format_rows_on_device_tensors():
    import torch
    from lfit_python_amd import chaintext
    chain, lnp = ct.block_case(6, 20, 18, seed=8)
    c, l = torch.as_tensor(chain.copy()).cuda(), torch.as_tensor(lnp.copy()).cuda()
    assert chaintext.format_rows(c, l) == ct.rows(chain, lnp)
    assert chaintext.format_rows(c, l, walker0=9990) == ct.rows(chain, lnp, 9990)
    c4, l4 = c.view(6, 4, 5, 18), l.view(6, 4, 5)
    assert chaintext.format_rows(c4[:, 0], l4[:, 0]) == ct.rows(chain.reshape(6, 4, 5, 18)[:, 0],
                                                               lnp.reshape(6, 4, 5)[:, 0])
    assert chaintext.format_rows(c[1::2], l[1::2]) == ct.rows(chain[1::2], lnp[1::2])
    assert chaintext.format_rows(c.permute(1, 0, 2), l.t()) == ct.rows(chain.transpose(1, 0, 2), lnp.T)
    assert chaintext.format_rows(c[:0], l[:0]) == b""
    assert chaintext.format_rows(c, lnp) == ct.rows(chain, lnp)   # (ln_prob still on the host)
    with np.errstate(over="ignore"):
        single = chain.astype(np.float32)
    assert chaintext.format_rows(c.float(), l) == ct.rows(single, lnp)


def _flux_fn(p, x, w, nsub):
    from lfit_python_amd.lfit import flux_batch
    f, st = flux_batch(np.asarray(p)[None, :], x, w, nsub=nsub)
    return f[0].cpu().numpy()


def test_run_mcmc_save_end_to_end(tmp_path):
    """a short seeded production run, once with the chunks left on the device
    (the kernels format them) and once offloaded (the twin does): either
    file is the oracle expression over the run's chain and lnprobability"""
    import torch
    from lfit_python_amd import batch, mcmc_utils, sampler, synthetic
    m = synthetic.config_single(60, flux_fn=_flux_fn)
    t = batch.compile_tree(m)
    ev = batch.LnProbEvaluator(t)
    p0 = np.array(m.dynasty_par_vals)
    init = sampler.initialise_walkers(p0, sampler.comp_scatter(m.dynasty_par_names, 0.1), 16,
                                      lambda p: ev(torch.as_tensor(p, device="cuda")).cpu().numpy())
    names = "walker_no " + " ".join(m.dynasty_par_names) + " ln_prob"
    files = []
    for offload in (False, True):
        S = sampler.EnsembleSampler(16, t.ndim, ev, seed=23)
        S.offload = offload
        f = str(tmp_path / ("chain_%d.txt" % offload))
        mcmc_utils.run_mcmc_save(S, init, 5, None, f, col_names=names, chunk=3)
        assert all(c.device.type == ("cpu" if offload else "cuda") for c, _ in S._chunks)
        want = names.encode() + b"\n" + ct.rows(S.chain.transpose(1, 0, 2), S.lnprobability.T)
        data = open(f, "rb").read()
        assert data == want, ct.first_difference(data, want)
        files.append(data)
    assert files[0] == files[1]
