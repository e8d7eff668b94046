"""GPU: lfg_limbdark (include/lfg_limbdark.h; MODEL_SPEC section 15) and
lfit_python_amd.limbdark on the device.

  parity    every point of tests/golden/limbdark_ref.npz (the reference's own
            ld()) x 25 columns within 64 eps c_max, statuses exact
  tables    synthetic tables on both sides of the size at which the surfaces
            no longer fit the LDS, and at the knot limit, against the numpy form
  counts    n of 1, 63, 64, 65 and 257 and one row beyond a launch's lanes (the
            grid-stride loop's second trip): row i of any batch is bit-identical
            to the same row computed alone, and a second run to the first
  strides   a [rows][5] chain read in place (ld = 5, ld = 15) against the
            gathered columns, bit for bit
  guards    tests/abi_guard.py's arena: out is exactly [n][25], status exactly
            [n], every element written, inputs and tables unchanged, guard
            bytes intact, for n of 0, 1, 65 and 257 and on a side stream
  python    from_chain, from_normal, summary, ld(), the command line
Every out-of-range case is a clamped argument, never an out-of-bounds index.
All shapes are small: 257 rows computed alone are the reference of the counts.
"""
import ctypes
import os
import shutil

import numpy as np
import pytest

from tests import abi_guard as ag
from tests import chain_double as cd
from tests import ld_double as ldd

pytestmark = pytest.mark.gpu
COUNTS = (1, 63, 64, 65, 257)
NROWS = 257


@pytest.fixture(scope="module")
def tables():
    return ldd.tables()


@pytest.fixture(scope="module")
def rows():
    """257 rows with all three statuses: (logg, teff, golden index or -1)"""
    return ldd.mixed_rows(NROWS)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    import torch
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _coef(rows, tables, sel=slice(None)):
    from lfit_python_amd import limbdark
    return limbdark.coefficients(np.array(rows[0][sel]), np.array(rows[1][sel]), tables)


@pytest.fixture(scope="module")
def alone(rows, tables):
    """every one of the 257 rows computed alone: (table [257, 25], status)"""
    import torch
    got = [_coef(rows, tables, slice(i, i + 1)) for i in range(NROWS)]
    return tuple(torch.cat([g[k] for g in got]) for k in range(2))


def test_parity_with_the_reference(tables):
    g = ldd.golden()
    table, status = _coef((g["logg"], g["teff"]), tables)
    assert table.shape == (len(g["logg"]), 25) and status.shape == (len(g["logg"]),)
    ldd.check_rows(table.cpu().numpy(), status.cpu().numpy(), g["logg"], g["teff"], np.arange(len(g["logg"])), "device")


def test_mixed_rows_and_clamped_rows(rows, tables, alone):
    logg, teff, idx = rows
    table, status = (t.cpu().numpy() for t in alone)
    assert set(status) == {ldd.ST_OK, ldd.ST_BAD_ARGS, ldd.ST_CLAMPED}
    ldd.check_rows(table, status, logg, teff, idx, "device, rows alone")
    cl = status == ldd.ST_CLAMPED
    edge, st = _coef((np.clip(logg[cl], 5.0, 9.5), np.clip(teff[cl], 4000.0, 30000.0)), tables)
    assert bool((st == 0).all()) and edge.cpu().numpy().tobytes() == table[cl].tobytes()


@pytest.mark.parametrize("nx,ny", [(30, 30), (30, 31), (64, 64), (8, 64)])
def test_tables_of_other_sizes(nx, ny):
    """(30, 30) is the largest square table whose 25 surfaces the kernel stages into LDS, (30, 31) the first
    that stays in global memory; 64 knots are the limit, 8 the least"""
    from scipy.interpolate import RectBivariateSpline
    from lfit_python_amd import limbdark
    rng = np.random.default_rng(nx * 100 + ny)
    gx, gy = np.linspace(5.0, 9.5, nx - 4), np.sort(rng.uniform(4000.0, 30000.0, ny - 4))
    vals = rng.uniform(-1.0, 1.0, (25, nx - 4, ny - 4))
    spl = [RectBivariateSpline(gx, gy, v, kx=3, ky=3) for v in vals]
    tx, ty = spl[0].get_knots()
    assert (len(tx), len(ty)) == (nx, ny)
    T = limbdark.LDTables(gx, gy, vals, tx, ty, np.stack([s.get_coeffs() for s in spl]))
    logg = np.concatenate([rng.uniform(4.8, 9.7, 300), gx[[0, -1]], [4.0, 11.0]])
    teff = np.concatenate([rng.uniform(3500.0, 31000.0, 300), gy[[0, -1]], [30000.0, 1e6]])
    table, status = limbdark.coefficients(logg, teff, T)
    want = T.eval_numpy(logg, teff)
    outside = (logg < gx[0]) | (logg > gx[-1]) | (teff < gy[0]) | (teff > gy[-1])
    assert np.array_equal(status.cpu().numpy(), np.where(outside, ldd.ST_CLAMPED, 0)) and outside.sum() > 10
    err = np.max(np.abs(table.cpu().numpy() - want))
    bound = 64 * np.finfo(np.float64).eps * T.c_max
    print("%d x %d knots: max abs error %.3e (tolerance %.3e)" % (nx, ny, err, bound))
    assert err <= bound


@pytest.mark.parametrize("n", COUNTS)
def test_rows_do_not_depend_on_the_batch(rows, tables, alone, n):
    first = _coef(rows, tables, slice(0, n))
    assert _same(first, tuple(a[:n] for a in alone))
    assert _same(_coef(rows, tables, slice(0, n)), first)


def test_grid_stride_second_trip(rows, tables, alone):
    import torch
    from lfit_python_amd import _native
    lanes = _native.lib().lfg_limbdark_lanes()
    n = lanes + 1
    reps = -(-n // NROWS)
    big = tuple(np.tile(v, reps)[:n] for v in rows[:2])
    first = _coef(big, tables)
    want = tuple(torch.cat([a] * reps)[:n] for a in alone)
    assert _same(first, want)
    assert _same(_coef(big, tables), first)


def _raw_call(tables, logg, teff, ld, n):
    """lfg_limbdark through ctypes on device tensors: (out [n][25], status)"""
    import torch
    from lfit_python_amd import _native
    dev = logg.device
    out = torch.empty((n, 25), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    S = tables.device_struct(dev)
    rc = _native.lib().lfg_limbdark(ag.ptr(logg), ag.ptr(teff), ld, n, ctypes.byref(S), ag.ptr(out), ag.ptr(status),
                                    _native.stream_ptr(dev))
    assert rc == 0
    return out, status


def test_strided_chain_is_read_in_place(rows, tables, alone):
    import torch
    chain = np.random.default_rng(8).uniform(-5.0, 5.0, (NROWS, 5))
    chain[:, 0], chain[:, 1] = rows[1], rows[0]                  # chain_wd's order: Teff, log_g
    c = torch.as_tensor(chain, device="cuda")
    flat = c.reshape(-1)
    assert _same(_raw_call(tables, flat[1:], flat[0:], 5, NROWS), alone)
    k = -(-NROWS // 3)
    assert _same(_raw_call(tables, flat[1:], flat[0:], 15, k), tuple(a[::3] for a in alone))
    assert _same((c.cpu(),), (torch.as_tensor(chain),))           # (bitwise: the chain holds NaN rows)


# ------------------------------------------------------------------ guarded buffers
def _guarded(A, rows, tables, n):
    import torch
    from lfit_python_amd import _native
    tab = {name: A.inp("tab_" + name, a) for name, a in tables.arrays.items()}
    S = tables.struct_over(lambda name: tab[name].data_ptr())
    logg, teff = A.inp("logg", rows[0][:n]), A.inp("teff", rows[1][:n])
    out = A.out("out", (n, 25), torch.float64)
    status = A.out("status", (n,), torch.int32)
    rc = _native.lib().lfg_limbdark(ag.ptr(logg), ag.ptr(teff), 1, n, ctypes.byref(S), ag.ptr(out), ag.ptr(status),
                                    A.stream_ptr())
    assert rc == 0
    A.check()                                   # guards intact, inputs and tables unchanged
    assert not A.poisoned("out").any() and not A.poisoned("status").any()
    return out.clone(), status.clone()


@pytest.fixture(scope="module")
def arena():
    return ag.Arena(nbytes=16 * 1024 * 1024)


@pytest.mark.parametrize("n", (0, 1, 65, 257))
def test_guarded_buffers(rows, tables, alone, arena, n):
    arena.reset(ag.POISON)
    got = _guarded(arena, rows, tables, n)
    assert _same(got, tuple(a[:n] for a in alone))


def test_guarded_buffers_on_a_side_stream(rows, tables, alone, arena):
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    x = torch.full((2048, 2048), 1e-3, device="cuda")
    for _ in range(16):                          # the default stream is kept busy meanwhile
        x = x @ x
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        arena.reset(ag.POISON)
        got = _guarded(arena, rows, tables, NROWS)
        assert _same(got, alone)
    torch.cuda.synchronize()


def test_refused_arguments(rows, tables):
    import torch
    from lfit_python_amd import _native
    L = _native.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    logg, teff = (torch.as_tensor(a[:4], device=dev) for a in rows[:2])
    out = torch.full((4, 25), 123.0, dtype=torch.float64, device=dev)
    status = torch.full((4,), 99, dtype=torch.int32, device=dev)
    S = tables.device_struct(dev)
    s = _native.stream_ptr(dev)

    def call(lg=logg, tf=teff, ld=1, n=4, tab=S, o=out, st=status):
        return L.lfg_limbdark(ag.ptr(lg), ag.ptr(tf), ld, n, ctypes.byref(tab) if tab is not None else None,
                              ag.ptr(o), ag.ptr(st), s)
    assert call(lg=None) == -1 and call(tf=None) == -1 and call(o=None) == -1 and call(st=None) == -1
    assert call(tab=None) == -1 and call(n=-1) == -1 and call(ld=0) == -1
    for nx, ny in ((7, S.ny), (65, S.ny), (S.nx, 7), (S.nx, 65)):
        assert call(tab=_native.LfgLdTables(S.tx, S.ty, nx, ny, S.c)) == -1, (nx, ny)
    for field in ("tx", "ty", "c"):
        bad = _native.LfgLdTables(S.tx, S.ty, S.nx, S.ny, S.c)
        setattr(bad, field, None)
        assert call(tab=bad) == -1, field
    assert call(n=0) == 0 and call(n=0, lg=None, o=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and bool((status == 99).all())      # nothing was launched
    assert call() == 0 and not bool((status == 99).any())


# ------------------------------------------------------------------ the Python surface
NAMES = ["Teff", "log_g", "Parallax", "E(B-V)", "ln_prob"]


@pytest.fixture(scope="module")
def chain():
    """[steps][W][5] around 14300 K, logg 8.1, as lfit_python_amd.wdparams writes it"""
    rng = np.random.default_rng(12)
    c = rng.uniform(0.0, 1.0, (9, 4, 5))
    c[:, :, 0] = 14300.0 + 300.0 * rng.standard_normal((9, 4))
    c[:, :, 1] = 8.1 + 0.05 * rng.standard_normal((9, 4))
    return c


def test_from_chain_reads_the_named_columns(chain, tables):
    import torch
    from lfit_python_amd import limbdark
    flat = chain.reshape(-1, 5)
    want = limbdark.coefficients(flat[:, 1], flat[:, 0], tables)
    assert int((want[1] == 0).sum()) == 36
    dev_chain = torch.as_tensor(chain, device="cuda")
    for c in (dev_chain, chain, flat):           # the sampler's shape on the device, a host chain, a flat chain
        assert _same(limbdark.from_chain(c, NAMES, tables), want)
    t3 = chain[::3].reshape(-1, 5)               # thinned by steps
    want3 = limbdark.coefficients(t3[:, 1], t3[:, 0], tables)
    assert _same(limbdark.from_chain(dev_chain, NAMES, tables, thin=3), want3)
    f3 = flat[::3]                               # a flat chain is thinned by rows, in place
    assert _same(limbdark.from_chain(flat, NAMES, tables, thin=3), limbdark.coefficients(f3[:, 1], f3[:, 0], tables))
    s2 = chain[2::3].reshape(-1, 5)
    assert _same(limbdark.from_chain(dev_chain, NAMES, tables, nskip=2, thin=3),
                 limbdark.coefficients(s2[:, 1], s2[:, 0], tables))
    with pytest.raises(ValueError):
        limbdark.from_chain(chain, ["a", "b", "c", "d", "e"], tables)


def test_long_inputs_are_cut_into_chunks(rows, tables, alone, monkeypatch):
    """the path of more than 2^31 - 1 rows, with the limit lowered to 100 rows"""
    from lfit_python_amd import limbdark
    monkeypatch.setattr(limbdark, "MAX_ROWS", 100)
    assert _same(_coef(rows, tables), alone)                        # 257 rows: chunks of 100, 100 and 57
    chain = np.zeros((NROWS, 5))
    chain[:, 0], chain[:, 1] = rows[1], rows[0]
    assert _same(limbdark.from_chain(chain, NAMES, tables, thin=2), tuple(a[::2] for a in alone))


def test_summary_is_numpys_median_and_std(rows, tables):
    from lfit_python_amd import limbdark
    good = np.cumsum(ldd.expected_status(rows[0], rows[1]) != ldd.ST_BAD_ARGS)     # used rows among the first n
    other = max(n for n in range(1, NROWS) if good[n - 1] % 2 != good[NROWS - 1] % 2)
    for n in (NROWS, other):                     # an odd and an even count of used rows
        table, status = _coef(rows, tables, slice(0, n))
        s = limbdark.summary(table, status)
        host, st = table.cpu().numpy(), status.cpu().numpy()
        used = host[st != ldd.ST_BAD_ARGS]
        assert s["n"] == n and s["n_bad"] == int((st == ldd.ST_BAD_ARGS).sum()) > 0 and len(used) == n - s["n_bad"]
        assert s["clamped"] == (st == ldd.ST_CLAMPED).sum() / n > 0
        assert np.array_equal(s["median"], np.median(used, axis=0))
        for c in range(25):
            ref = cd.column(used[:, c], fracs=())
            want = np.sqrt(ref["m2"] / len(used))
            # m2 within chainstats' bound; the square root halves the relative error and adds its own rounding
            bound = 0.5 * cd.moment_bound(ref["m2"], ref["m2_np"]) / ref["m2"] * want + 2 * np.spacing(want)
            assert abs(s["std"][c] - want) <= bound, (c, s["std"][c], want, bound)
            assert np.isclose(s["std"][c], np.std(used[:, c]), rtol=1e-12)
    lines = limbdark.summary_lines(s)
    assert len(lines) == 31 and lines[1] == "u band LD coeff = %f +/- %f" % (np.median(used[:, 0]), np.std(used[:, 0]))


def test_from_normal_is_seeded(tables):
    import torch
    from lfit_python_amd import limbdark
    a = limbdark.from_normal(8.1, 0.05, 14300.0, 300.0, tables, size=500, seed=3)
    b = limbdark.from_normal(8.1, 0.05, 14300.0, 300.0, tables, size=500, seed=3)
    c = limbdark.from_normal(8.1, 0.05, 14300.0, 300.0, tables, size=500, seed=4)
    assert a[0].shape == (500, 25) and _same(a, b) and not torch.equal(a[0], c[0])
    fixed = limbdark.from_normal(8.1, 0.0, 14300.0, 0.0, tables, size=7)
    centre = limbdark.coefficients(8.1, 14300.0, tables)
    assert _same(fixed, (centre[0].expand(7, 25), centre[1].expand(7)))
    # the draws scatter about the centre by what 0.05 dex and 300 K can move a coefficient (0.1 at four sigma)
    assert float((a[0] - centre[0]).abs().max()) < 0.2 and float(a[0].std(dim=0).min()) > 0.0


def test_ld_has_the_references_shapes(tables):
    from lfit_python_amd import limbdark
    g = ldd.golden()
    i = int(np.flatnonzero(g["kind"] == 4)[0])
    lin = limbdark.ld("g", g["logg"][i], g["teff"][i], tables=tables)
    quad = limbdark.ld("g", g["logg"][i], g["teff"][i], law="quad", tables=tables)
    sqr = limbdark.ld("z", g["logg"][i], g["teff"][i], "sqr", tables=tables)
    assert isinstance(lin, float) and isinstance(quad, tuple) and isinstance(sqr, tuple)
    assert len(quad) == len(sqr) == 2 and all(isinstance(v, float) for v in quad + sqr)
    want = g["table"][i]
    assert np.max(np.abs(np.array([lin, *quad, *sqr]) - want[[5, 6, 7, 23, 24]])) <= ldd.tol()
    # outside the grid the reference returns the value at the edge
    assert limbdark.ld("z", 9.9, 41000.0, tables=tables) == limbdark.ld("z", 9.5, 30000.0, tables=tables)
    assert np.isnan(limbdark.ld("u", np.nan, 12000.0, tables=tables))


def test_command_line(chain, tables, tmp_path, capsys, monkeypatch):
    from lfit_python_amd import limbdark, sampler
    # the reference's form: four numbers
    assert limbdark.main(["--dir", ldd.LD_DIR, "8.1", "0.05", "14300", "300", "--size", "1000", "--seed", "2"]) == 0
    out = capsys.readouterr().out.splitlines()
    s = limbdark.summary(*limbdark.from_normal(8.1, 0.05, 14300.0, 300.0, tables, size=1000, seed=2))
    assert out == limbdark.summary_lines(s) and len(out) == 31
    # prompted, as the reference prompts
    answers = iter(["9.4 0.2", "14300 300"])
    monkeypatch.setattr("builtins.input", lambda prompt="": next(answers))
    assert limbdark.main(["--dir", ldd.LD_DIR, "--size", "400"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[:31] == limbdark.summary_lines(limbdark.summary(*limbdark.from_normal(9.4, 0.2, 14300.0, 300.0, tables,
                                                                                      size=400)))
    assert len(out) == 32 and "clamped" in out[31]              # logg 9.4 +- 0.2 leaves the grid
    # a chain, and the input file's ulimb lines
    fname = str(tmp_path / "chain_wd.txt")
    sampler.write_chain(fname, NAMES[:4], chain[:, :, :4], chain[:, :, 4])
    inp = str(tmp_path / "mcmc_input.dat")
    shutil.copy(os.path.join(ldd.ROOT, "tests", "golden", "ref_test_data", "mcmc_input.dat"), inp)
    before = open(inp, "rb").read().splitlines()
    assert limbdark.main(["--dir", ldd.LD_DIR, "--chain", fname, "--nskip", "1", "--update", inp]) == 0
    out = capsys.readouterr().out.splitlines()
    picked = chain[1:].reshape(-1, 5)
    s = limbdark.summary(*limbdark.coefficients(picked[:, 1], picked[:, 0], tables))
    assert out[:31] == limbdark.summary_lines(s) and "ulimb_g, ulimb_r" in out[31]
    after = open(inp, "rb").read().splitlines()
    changed = [a for a, b in zip(after, before) if a != b]
    assert len(after) == len(before) and len(changed) == 2
    for line, band in zip(changed, (1, 2)):
        text = ("%.4f" % s["median"][5 * band]).encode()
        assert line.split() == [b"ulimb_" + b"ugriz"[band:band + 1], b"=", text, b"gauss", text, b"0.001", b"1"]
