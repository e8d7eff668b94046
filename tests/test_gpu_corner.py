"""GPU: the corner-plot kernels (include/lfg_corner.h, MODEL_SPEC section 16)
against the numpy double and the case list of tests/corner_double.py, in
guarded buffers (tests/abi_guard.py): sizes, layouts, column picks, pair
tiles, bin counts, ranges, the most contended bin, the identities, the memory
contract, refusals, the levels, and the Python layer up to
fit_summary(corners=True).

Every count is compared for integer equality.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import abi_guard as ag
from tests import chain_double as cd
from tests import corner_double as co
from tests.abi_guard import ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from lfit_python_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def arena():
    return ag.Arena()


def call(L, A, buf, off, steps, W, row_len, sld, wld, cols, rng, nb, fracs=co.FRACS, ws_short=0, out_k=None,
         null=()):
    """lfg_corner_hist, then lfg_corner_levels on its h2, in allocator A's
    buffers -> (rc, rc of the levels, dict of host arrays)"""
    import torch
    K = len(cols)
    k = K if out_k is None else out_k          # (the outputs of a refused K or nb only have to exist)
    m = nb if 1 <= nb <= 64 else 4
    P = k * (k - 1) // 2
    fr = np.ascontiguousarray(fracs, dtype=np.float64)
    chain = A.inp("chain", buf)
    rdev = A.inp("range", np.ascontiguousarray(rng, dtype=np.float64).reshape(-1, 2))
    o = {"h1": A.out("h1", (k, m), torch.int64), "h2": A.out("h2", (P, m, m), torch.int64),
         "flag": A.out("flag", k, torch.int32), "levels": A.out("levels", (P, fr.size), torch.int64)}
    nbytes = L.lfg_corner_workspace_size(max(steps, 0), max(W, 0), min(max(K, 1), 64), min(max(nb, 1), 64))
    ws = A.ws("ws", nbytes)
    carr = (ctypes.c_int * max(K, 1))(*cols)
    p = {"base": ctypes.c_void_p(chain.data_ptr() + 8 * off), "cols": carr, "range": ptr(rdev), "h1": ptr(o["h1"]),
         "h2": ptr(o["h2"]) if k > 1 else None, "flag": ptr(o["flag"]), "ws": ptr(ws)}
    for name in null:
        p[name] = None
    rc = L.lfg_corner_hist(p["base"], steps, W, row_len, sld, wld, p["cols"], K, p["range"], nb, p["h1"], p["h2"],
                           p["flag"], p["ws"], nbytes - ws_short, A.stream_ptr())
    rl = None
    if rc == 0 and P:
        rl = L.lfg_corner_levels(ptr(o["h2"]), P, nb, fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), fr.size,
                                 ptr(o["levels"]), A.stream_ptr())
    A.check()
    return rc, rl, {n: t.cpu().numpy() for n, t in o.items()}


@pytest.fixture()
def device(L, arena):
    def backend(buf, off, steps, W, row_len, sld, wld, cols, rng, nb):
        arena.reset()
        rc, rl, out = call(L, arena, buf, off, steps, W, row_len, sld, wld, cols, rng, nb)
        assert rc == 0 and rl in (0, None)
        for k in out:
            assert not arena.poisoned(k).any(), k   # every output element is written
        return out
    return backend


def test_tiles(L):
    assert L.lfg_corner_tile_rows() == co.TILE_ROWS and (co.TILE_ROWS + 1, 1) in co.SIZES
    for nb, T in co.PAIR_TILE.items():
        assert L.lfg_corner_pair_tile(nb) == T
    assert L.lfg_corner_pair_tile(4) < 2016                   # K = 64 at nb = 4 is several tiles
    assert L.lfg_corner_pair_tile(0) == 0 and L.lfg_corner_pair_tile(65) == 0
    assert L.lfg_corner_workspace_size(10, 10, 65, 50) == 0 and L.lfg_corner_workspace_size(10, 10, 3, 0) == 0
    assert L.lfg_corner_workspace_size(-1, 10, 3, 50) == 0 and L.lfg_corner_workspace_size(10, 10, 3, 50) > 0


@pytest.mark.parametrize("c", co.CASES, ids=lambda c: "%dx%d-%s-C%d-K%d-nb%d-%s" % (c[0] + c[1:]))
def test_case_list(device, c):
    """sizes x layouts with unsorted, non-adjacent columns; K = 1 (h2 NULL),
    one pair tile, a tile and a remainder, several tiles, 2 016 pairs; nb of
    1, 2, 50, 64; default and cutting ranges, immobile columns, the 20-ulp
    range, the offset and the non-finite columns (corner_double.CASES)"""
    got, want = co.run_case(device, c)
    size, kind, C, K, nb, mode = c
    x, cols, rng, _ = co.case(*c)
    used = [co.bin_rule(x[:, :, cc].reshape(-1), rng[k][0], rng[k][1], nb) >= 0 if co.mobile(*rng[k])
            else np.zeros(x.shape[0] * x.shape[1], dtype=bool) for k, cc in enumerate(cols)]
    for p, (a, b) in enumerate(co.pairs(K)):
        assert got["h2"][p].sum() == int((used[a] & used[b]).sum())
        if used[b].all():
            assert np.array_equal(got["h2"][p].sum(axis=1), got["h1"][a])
        if used[a].all():
            assert np.array_equal(got["h2"][p].sum(axis=0), got["h1"][b])
    if mode == "immobile":
        assert got["flag"][1] == 1 and not got["h1"][1].any() and got["flag"][0] == 0 and got["h1"][0].any()
        assert all(not got["h2"][p].any() for p, (a, b) in enumerate(co.pairs(K)) if 1 in (a, b))


def test_default_range_from_the_device(L, arena):
    """the range as lfg_chain_stats leaves it on the device: no value makes a round trip"""
    import torch
    from lfit_python_amd import chainstats
    c = ((64, 64), "chain_dev", 10, 10, 50, "default")
    x, cols, rng, want = co.case(*c)
    t = torch.as_tensor(np.array(x)).cuda()
    r = chainstats._run(chainstats._View(t), np.empty(0))
    at = torch.as_tensor(cols, device=t.device)
    rdev = torch.stack([r["min"][at], r["max"][at]], dim=1).contiguous()
    assert np.array_equal(rdev.cpu().numpy(), rng, equal_nan=True)
    arena.reset()
    buf, off, sld, wld = cd.layout(x, "chain_dev")
    rc, rl, out = call(L, arena, buf, off, 64, 64, 10, sld, wld, cols, rdev.cpu().numpy(), 50)
    assert rc == 0 and rl == 0
    co.check(out, want, "device range")


def test_everything_in_one_bin(L, arena):
    """the most contended LDS address: 4 096 rows in one bin of each pair"""
    x = np.full((64, 64, 3), 0.25)
    x[:, :, 1] = 7.01
    buf, off, sld, wld = cd.layout(x, "chain_dev")
    arena.reset()
    rc, rl, got = call(L, arena, buf, off, 64, 64, 3, sld, wld, (2, 0, 1), [(0.0, 1.0), (0.0, 1.0), (6.0, 8.0)], 50)
    assert rc == 0 and rl == 0
    assert got["h2"][0, 12, 12] == 4096 and got["h2"].sum() == 3 * 4096 and got["h2"][1, 12, 25] == 4096
    assert got["h1"][0, 12] == 4096 and got["h1"][2, 25] == 4096 and got["h1"].sum() == 3 * 4096
    assert np.array_equal(got["levels"], np.full((3, 4), 4096))


def test_scratch_and_output_contents_and_repeats_do_not_matter(L, arena):
    import torch
    c = ((64, 64), "chain_dev", 10, 10, 50, "cut")
    x, cols, rng, want = co.case(*c)
    buf, off, sld, wld = cd.layout(x, "chain_dev")
    runs = []
    for fill in (ag.POISON, 0, None, None):
        arena.reset(fill)       # (outputs start as poison: garbage the call must overwrite in full)
        rc, rl, out = call(L, arena, buf, off, 64, 64, 10, sld, wld, cols, rng, 50)
        assert rc == 0 and rl == 0
        runs.append(arena.result())
    for other in runs[1:]:
        assert all(np.array_equal(runs[0][k], other[k]) for k in runs[0])
    # outputs pre-filled with other garbage than the arena's poison
    A = ag.Plain(ws_fill=0x5A)
    h = {}
    real_out = A.out

    def garbage_out(name, shape, dtype):
        t = real_out(name, shape, dtype)
        t.view(torch.uint8).fill_(0x3C)
        h[name] = t
        return t
    A.out = garbage_out
    rc, rl, out = call(L, A, buf, off, 64, 64, 10, sld, wld, cols, rng, 50)
    assert rc == 0 and rl == 0
    co.check(out, want, "garbage outputs")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        arena.reset()
        rc, rl, out = call(L, arena, buf, off, 64, 64, 10, sld, wld, cols, rng, 50)
        got = arena.result()
    assert rc == 0 and rl == 0 and all(np.array_equal(runs[0][k], got[k]) for k in runs[0])
    co.check(out, want, "side stream")


def test_refusals_write_nothing(L, arena):
    v = np.arange(48.0)
    ok = dict(buf=v, off=0, steps=4, W=2, row_len=3, sld=6, wld=3, cols=(2, 0), rng=[(0, 50), (0, 50)], nb=5)
    arena.reset()
    rc, rl, out = call(L, arena, **ok)
    assert rc == 0 and rl == 0 and out["h2"].sum() == 8
    cases = [dict(steps=-1), dict(W=-1), dict(row_len=0), dict(sld=0), dict(wld=0), dict(nb=0), dict(nb=65),
             dict(cols=(0, 3)), dict(cols=(-1, 0)), dict(cols=(1, 1)), dict(cols=(), rng=[(0, 1)], out_k=2),
             dict(cols=tuple(range(65)), rng=[(0, 1)] * 65, row_len=65, buf=np.zeros(8 * 65), sld=130, wld=65, out_k=2),
             dict(ws_short=1), dict(null=("base",)), dict(null=("cols",)), dict(null=("range",)), dict(null=("h1",)),
             dict(null=("h2",)), dict(null=("flag",)), dict(null=("ws",)),
             dict(cols=(1,), rng=[(0, 50)], out_k=2)]      # K = 1 with an h2 (out_k = 2 hands it one)
    for change in cases:
        arena.reset()
        args = dict(ok, **change)
        rc, _, _ = call(L, arena, **args)
        assert rc == -1, change
        for name in ("h1", "h2", "flag"):
            assert arena.poisoned(name).all(), (change, name)
    # the levels' refusals
    import torch
    for fracs, nb, P in (((), 5, 1), ((0.5,) * 9, 5, 1), ((-0.1,), 5, 1), ((1.5,), 5, 1), ((np.nan,), 5, 1),
                         ((0.5,), 0, 1), ((0.5,), 65, 1), ((0.5,), 5, -1)):
        arena.reset()
        h2 = arena.inp("h2", np.ones((1, 5, 5), dtype=np.int64))
        lev = arena.out("levels", (1, 9), torch.int64)
        fr = np.ascontiguousarray(fracs if len(fracs) else (0.0,), dtype=np.float64)
        rc = L.lfg_corner_levels(ptr(h2), P, nb, fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(fracs),
                                 ptr(lev), arena.stream_ptr())
        arena.check()
        assert rc == -1 and arena.poisoned("levels").all(), (fracs, nb, P)
    arena.reset()
    lev = arena.out("levels", (1, 1), torch.int64)
    fr = (ctypes.c_double * 1)(0.5)
    assert L.lfg_corner_levels(None, 1, 5, fr, 1, ptr(lev), arena.stream_ptr()) == -1
    assert L.lfg_corner_levels(ptr(lev), 1, 5, None, 1, ptr(lev), arena.stream_ptr()) == -1
    assert L.lfg_corner_levels(ptr(lev), 1, 5, fr, 1, None, arena.stream_ptr()) == -1
    arena.check()
    assert arena.poisoned("levels").all()
    # steps = 0 or W = 0: zeros and the flags
    for steps, W in ((0, 2), (4, 0)):
        arena.reset()
        rc, rl, out = call(L, arena, v, 0, steps, W, 3, 6, 3, (2, 0), [(0, 50), (1, 1)], 5)
        assert rc == 0 and rl == 0 and not out["h1"].any() and not out["h2"].any() and list(out["flag"]) == [0, 1]
        assert not out["levels"].any() and not arena.poisoned("h1").any() and not arena.poisoned("h2").any()


def test_levels_constructed(L, arena):
    import torch
    for h, fracs, want in co.level_cases():
        arena.reset()
        nb = h.shape[0]
        # the case twice with another histogram between: one workgroup per pair
        stack = np.stack([h, np.arange(nb * nb, dtype=np.int64).reshape(nb, nb), h])
        h2 = arena.inp("h2", stack)
        lev = arena.out("levels", (3, len(fracs)), torch.int64)
        fr = np.ascontiguousarray(fracs, dtype=np.float64)
        rc = L.lfg_corner_levels(ptr(h2), 3, nb, fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), fr.size, ptr(lev),
                                 arena.stream_ptr())
        arena.check()
        got = lev.cpu().numpy()
        assert rc == 0 and tuple(got[0]) == want and tuple(got[2]) == want, (h, fracs, got)
        assert np.array_equal(got[1], co.levels(stack[1], fracs))
    # 64 x 64 counts with many ties, eight fractions
    rng = np.random.default_rng(6)
    stack = rng.integers(0, 40, size=(5, 64, 64)).astype(np.int64)
    stack[1] = 0
    stack[2, ::2] = 0
    fracs = (0.0, 0.1, 0.393, 0.5, 0.865, 0.99, 1.0, 0.3)
    arena.reset()
    h2 = arena.inp("h2", stack)
    lev = arena.out("levels", (5, 8), torch.int64)
    fr = np.ascontiguousarray(fracs, dtype=np.float64)
    rc = L.lfg_corner_levels(ptr(h2), 5, 64, fr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 8, ptr(lev),
                             arena.stream_ptr())
    arena.check()
    assert rc == 0 and np.array_equal(lev.cpu().numpy(), np.array([co.levels(h, fracs) for h in stack]))


def test_corner_data_end_to_end(tmp_path):
    """corner_data on a device tensor [steps][W][ndim], columns by name, with
    nskip and thin; a walker-major host array; an explicit range"""
    import torch
    from lfit_python_amd import corner
    x = co.chain(37, 6, 10)
    names = ["%s_%d" % (k, i) for i, k in enumerate(co.COLUMNS)]
    pick = ["offset_1", "normal_0", "same_8", "nonfinite_6"]
    cols = [names.index(n) for n in pick]
    t = torch.as_tensor(np.array(x)).cuda()
    d = corner.corner_data(t, cols=pick, names=names, nskip=1, thin=2)
    xs = x[1::2]
    want = co.expected(xs, cols, co.ranges(xs, cols), 50, corner.DEFAULT_LEVELS)
    co.check({"h1": d.hist1d, "h2": d.hist2d, "flag": (~d.mobile).astype(np.int32), "levels": d.levels}, want)
    assert d.names == pick and list(d.cols) == cols and list(d.mobile) == [True, True, False, True]
    assert np.array_equal(d.edges[0], np.linspace(xs[:, :, 1].min(), xs[:, :, 1].max(), 51))
    assert np.isnan(d.edges[2]).all() and d.hist2d.shape == (6, 50, 50) and d.levels.shape == (6, 4)
    back = corner.CornerData.load(d.save(str(tmp_path / "d.npz")))
    assert np.array_equal(back.hist2d, d.hist2d) and back.names == pick
    # walker-major host array, indices, another bin count, an explicit range, other levels
    rng = co.ranges(x, cols, "cut")
    d = corner.corner_data(np.ascontiguousarray(x.transpose(1, 0, 2)), cols=cols, bins=7, range=rng,
                           levels=(0.5, 0.9), walker_major=True)
    want = co.expected(x, cols, rng, 7, (0.5, 0.9))
    co.check({"h1": d.hist1d, "h2": d.hist2d, "flag": (~d.mobile).astype(np.int32), "levels": d.levels}, want)
    assert d.names == ["col%d" % c for c in cols]
    for bad in (dict(cols=["nope"], names=names), dict(cols=[0, 0]), dict(cols=[10]), dict(bins=65), dict(bins=0),
                dict(levels=(1.5,)), dict(cols=list(range(10)) * 7)):
        with pytest.raises((ValueError, KeyError)):
            corner.corner_data(t, **bad)


def test_fit_summary_corners(tmp_path):
    """fit_summary(corners=True) on a short synthetic chain for the golden
    input: one .npz per eclipse whose contents equal the double's; without
    corners none is written.  (corner_plots=False: the six 21-column figures
    would take matplotlib most of a minute; thumb_plot has its own test.)"""
    from lfit_python_amd import chainstats, corner, cvmodel
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_test_data", "mcmc_input.dat")
    model = cvmodel.construct_model(golden)
    names = model.dynasty_par_names
    start = np.array(model.dynasty_par_vals)
    rng = np.random.default_rng(12)
    steps, W = 12, 40
    x = start * (1.0 + 1e-3 * rng.normal(size=(steps, W, len(names))))
    stuck = names.index("phi0_2")               # the reference's immobile variable
    x[:, :, stuck] = 0.0
    said = []
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    plain = chainstats.fit_summary(x, names, input_file=golden, out_dir=str(a), log=said.append)
    assert "corners" not in plain and not (a / "Final_figs").exists()
    out = chainstats.fit_summary(x, names, input_file=golden, out_dir=str(b), log=said.append, corners=True,
                                 corner_plots=False)
    assert open(out["modparams"], "rb").read() == open(plain["modparams"], "rb").read()
    files = sorted(p for p in out["corners"] if p.endswith(".npz"))
    assert [os.path.basename(p) for p in files] == ["test_data_%d_corners.npz" % i for i in range(6)]
    assert sorted(os.listdir(b / "Final_figs")) == sorted(os.path.basename(p) for p in out["corners"])
    for (ecl, labels), path in zip(corner.corner_columns(model, names), files):
        d = corner.CornerData.load(path)
        keep = [lab for lab in labels if lab != "phi0_2"]
        assert d.names == keep and d.mobile.all() and len(keep) == (20 if ecl.label == "2" else 21)
        cols = [names.index(lab) for lab in keep]
        want = co.expected(x, cols, co.ranges(x, cols), 50, corner.DEFAULT_LEVELS)
        co.check({"h1": d.hist1d, "h2": d.hist2d, "flag": np.zeros(len(cols), np.int32), "levels": d.levels}, want,
                 path)
        assert list(d.cols) == cols
