"""CPU: lfit_python_amd.limbdark's host side and lfg_limbdark's host twin
(MODEL_SPEC section 15) against the reference's own ld(), recorded in
tests/golden/limbdark_ref.npz by tools/make_ld_golden.py.

The loader's knots and coefficients are scipy's; the numpy path
(physpar.eval_bispline), the independent tensor-product double
(tests/ld_double.py, inside points only) and the host twin
(cpu_baseline/lfg_cpu_limbdark.cpp, lfg_limbdark.hpp compiled for the host)
meet every golden value within 64 eps c_max, with no row left out; statuses
are exact.  Then the Python surface that needs no device: summary_lines,
update_input, the loader's errors, ld()'s assertions.
"""
import os
import shutil

import numpy as np
import pytest

from tests import ld_double as ldd

ROOT = ldd.ROOT
INPUT = os.path.join(ROOT, "tests", "golden", "ref_test_data", "mcmc_input.dat")


@pytest.fixture(scope="module")
def tables():
    return ldd.tables()


@pytest.fixture(scope="module")
def port():
    from cpu_baseline import cpu
    if not os.path.exists(cpu.LIB_PATH):
        cpu.build()
    return cpu.CpuPort()


def test_golden_file_covers_what_it_should(tables):
    g = ldd.golden()
    assert g["table"].shape == (len(g["logg"]), 25) and np.all(np.isfinite(g["table"]))
    assert [int((g["kind"] == k).sum()) for k in range(5)] == [627, 576, 8, 4, 200]
    st = ldd.expected_status(g["logg"], g["teff"])
    assert np.all(st[g["kind"] == 2] == ldd.ST_CLAMPED) and np.all(st[g["kind"] <= 1] == ldd.ST_OK)
    assert np.all(st[g["kind"] == 3] == ldd.ST_OK) and set(st[g["kind"] == 4]) == {ldd.ST_OK, ldd.ST_CLAMPED}
    # the cell centres use every knot interval of both axes
    c = g["kind"] == 1
    lx = np.searchsorted(tables.tx, g["logg"][c], side="right") - 1
    ly = np.searchsorted(tables.ty, g["teff"][c], side="right") - 1
    assert set(lx) == set(range(3, len(tables.tx) - 4)) and set(ly) == set(range(3, len(tables.ty) - 4))


def test_loader_is_scipys_spline(tables):
    from scipy.interpolate import RectBivariateSpline
    from lfit_python_amd import limbdark
    assert tables.logg.shape == (19,) and tables.teff.shape == (33,) and tables.values.shape == (25, 19, 33)
    assert tables.tx.shape == (23,) and tables.ty.shape == (37,) and tables.c.shape == (25, 19 * 33)
    # not-a-knot: the second and the last but one node of each axis are no knots
    for t, nodes in ((tables.tx, tables.logg), (tables.ty, tables.teff)):
        assert np.array_equal(t[:4], [nodes[0]] * 4) and np.array_equal(t[-4:], [nodes[-1]] * 4)
        assert np.array_equal(t[4:-4], nodes[2:-2])
    for b, band in enumerate(limbdark.BANDS):
        data = np.loadtxt(os.path.join(ldd.LD_DIR, limbdark.TABLE_FILE % band))
        assert data.shape[0] == 627
        for k in range(5):
            z = data[:, 2 + k].reshape(19, 33)
            assert np.array_equal(tables.values[5 * b + k], z)
            spl = RectBivariateSpline(tables.logg, tables.teff, z, kx=3, ky=3)
            assert np.array_equal(spl.get_knots()[0], tables.tx) and np.array_equal(spl.get_knots()[1], tables.ty)
            assert np.array_equal(spl.get_coeffs(), tables.c[5 * b + k])
    assert tables.c_max == np.abs(tables.c).max() and 1.0 < tables.c_max < 2.0
    H = tables.host_struct()
    assert (H.nx, H.ny) == (23, 37) and H.tx == tables.tx.ctypes.data and H.c == tables.c.ctypes.data


def test_numpy_path_meets_the_reference(tables):
    g = ldd.golden()
    got = tables.eval_numpy(g["logg"], g["teff"])
    err = np.max(np.abs(got - g["table"]))
    print("numpy path: max abs error %.3e (tolerance %.3e)" % (err, ldd.tol()))
    assert got.shape == g["table"].shape and err <= ldd.tol()


def test_independent_double_meets_the_reference_inside():
    g = ldd.golden()
    inside = ldd.expected_status(g["logg"], g["teff"]) == ldd.ST_OK
    assert inside.sum() > 1300
    got = ldd.tensor_double(g["logg"][inside], g["teff"][inside])
    err = np.max(np.abs(got - g["table"][inside]))
    print("tensor-product double: max abs error %.3e (tolerance %.3e)" % (err, ldd.tol()))
    assert err <= ldd.tol()


def test_host_twin_meets_the_reference(tables, port):
    g = ldd.golden()
    table, status = port.limbdark(g["logg"], g["teff"], tables)
    assert table.shape == g["table"].shape
    ldd.check_rows(table, status, g["logg"], g["teff"], np.arange(len(g["logg"])), "host twin")
    # the nodes reproduce the table entries
    nodes = g["kind"] == 0
    entries = tables.values.reshape(25, -1).T
    assert np.array_equal(g["logg"][nodes], np.repeat(tables.logg, 33))
    assert np.max(np.abs(table[nodes] - entries)) <= ldd.tol()
    # one thread and several give the same bits
    again, _ = port.limbdark(g["logg"], g["teff"], tables, nthreads=1)
    assert again.tobytes() == table.tobytes()


def test_host_twin_statuses_and_strides(tables, port):
    logg, teff, idx = ldd.mixed_rows()
    table, status = port.limbdark(logg, teff, tables)
    assert set(status) == {ldd.ST_OK, ldd.ST_BAD_ARGS, ldd.ST_CLAMPED}
    ldd.check_rows(table, status, logg, teff, idx, "host twin, mixed rows")
    # a clamped row is the row at the clamped arguments
    cl = status == ldd.ST_CLAMPED
    edge, st = port.limbdark(np.clip(logg[cl], 5.0, 9.5), np.clip(teff[cl], 4000.0, 30000.0), tables)
    assert np.all(st == ldd.ST_OK) and edge.tobytes() == table[cl].tobytes()
    # just inside, on and just outside an edge
    lg = np.array([5.0, np.nextafter(5.0, 0.0), 9.5, np.nextafter(9.5, 10.0), 7.0, 7.0, 7.0, 7.0])
    tf = np.array([9000.0, 9000.0, 9000.0, 9000.0, 4000.0, np.nextafter(4000.0, 0.0), 30000.0,
                   np.nextafter(30000.0, 4e4)])
    _, st = port.limbdark(lg, tf, tables)
    assert list(st) == [0, 7, 0, 7, 0, 7, 0, 7]
    # a [rows][5] chain read in place
    chain = np.full((len(logg), 5), 3.0)
    chain[:, 0], chain[:, 1] = teff, logg
    flat = chain.reshape(-1)
    t5, s5 = port.limbdark(flat[1:], flat[0:], tables, ld=5, n=len(logg))
    assert t5.tobytes() == table.tobytes() and np.array_equal(s5, status)
    t15, s15 = port.limbdark(flat[1:], flat[0:], tables, ld=15, n=(len(logg) + 2) // 3)
    assert t15.tobytes() == table[::3].tobytes() and np.array_equal(s15, status[::3])
    # the argument checks
    H = tables.host_struct()
    for nx, ny in ((7, 37), (65, 37), (23, 7), (23, 65)):
        from lfit_python_amd import _native
        import ctypes
        bad = _native.LfgLdTables(H.tx, H.ty, nx, ny, H.c)
        out, s1 = np.empty(25), np.empty(1, np.int32)
        f = port.lib.lfg_cpu_limbdark
        rc = f(logg.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), teff.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
               1, 1, ctypes.byref(bad), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
               s1.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1)
        assert rc == -1, (nx, ny)


def test_native_registers_the_unit():
    from lfit_python_amd import _native
    assert _native.EXPORTS_LIMBDARK == ("lfg_limbdark", "lfg_limbdark_lanes")
    for other in (_native.EXPORTS, _native.EXPORTS_PHYSPAR, _native.EXPORTS_WD, _native.EXPORTS_CHAIN):
        assert not set(_native.EXPORTS_LIMBDARK) & set(other)
    path = os.path.join(_native.REPO, "include", "lfg_limbdark.h")
    text = open(path).read()
    assert path in _native.HEADERS and os.path.join(_native._HERE, "csrc", "lfg_limbdark.hpp") in _native.HEADERS
    assert any(p.endswith("lfg_limbdark.hip") for p in _native.SOURCES)
    for name, value in (("LFG_LD_NBAND", _native.LD_NBAND), ("LFG_LD_NCOEF", _native.LD_NCOEF),
                        ("LFG_LD_NCOL", _native.LD_NCOL), ("LFG_LD_MAX_KNOTS", _native.LD_MAX_KNOTS),
                        ("LFG_ST_LD_CLAMPED", _native.ST_LD_CLAMPED)):
        assert ("#define %s %d" % (name, value)) in " ".join(text.split()), name
    assert "lfg_limbdark" not in open(os.path.join(_native.REPO, "include", "lfg.h")).read()


# ------------------------------------------------------------------ the Python surface
def test_ld_asserts_as_the_reference(tables):
    from lfit_python_amd import limbdark
    with pytest.raises(AssertionError):
        limbdark.ld("KG5", 8.0, 12000.0, tables=tables)
    with pytest.raises(AssertionError):
        limbdark.ld("g", 8.0, 12000.0, law="log", tables=tables)


def test_summary_lines_are_the_references():
    from lfit_python_amd import limbdark
    rng = np.random.default_rng(2)
    s = {"median": rng.uniform(-0.3, 1.1, 25), "std": rng.uniform(0.0, 0.02, 25)}
    s["median"][7], s["std"][7] = -0.0000004, 0.0
    want = ["-------------------"]
    for b, band in enumerate(["u", "g", "r", "i", "z"]):
        m, e = s["median"][5 * b: 5 * b + 5], s["std"][5 * b: 5 * b + 5]
        want.append('%s band LD coeff = %f +/- %f' % (band, m[0], e[0]))
        want.append('%s band quad coeff a = %f +/- %f' % (band, m[1], e[1]))
        want.append('%s band quad coeff b = %f +/- %f' % (band, m[2], e[2]))
        want.append('%s band sqr coeff d = %f +/- %f' % (band, m[3], e[3]))
        want.append('%s band sqr coeff f = %f +/- %f' % (band, m[4], e[4]))
        want.append('-------------------')
    got = limbdark.summary_lines(s)
    assert got == want and len(got) == 31
    assert limbdark.linear_medians(s) == {b: s["median"][5 * k] for k, b in enumerate("ugriz")}


def test_update_input_rewrites_only_the_band_lines(tmp_path):
    from lfit_python_amd import cvmodel, limbdark
    from lfit_python_amd.tree import Param
    src = str(tmp_path / "mcmc_input.dat")
    shutil.copy(INPUT, src)
    before = open(src, "rb").read().splitlines(keepends=True)
    cfg0 = cvmodel.read_config(src)
    meds = {"u": 0.41234567, "g": 0.35678901, "r": 0.3123449, "i": 0.29, "z": 0.27}
    out = str(tmp_path / "updated.dat")
    changed = limbdark.update_input(src, meds, out=out)
    assert sorted(changed) == ["g", "r"] and open(src, "rb").read() == b"".join(before)   # the source is untouched
    after = open(out, "rb").read().splitlines(keepends=True)
    assert len(after) == len(before)
    touched = [k for k, (a, b) in enumerate(zip(before, after)) if a != b]
    assert [before[k].split(b"=")[0].strip() for k in touched] == [b"ulimb_g", b"ulimb_r"]
    cfg = cvmodel.read_config(out)
    assert set(cfg) == set(cfg0)
    for key in cfg:
        if key not in ("ulimb_g", "ulimb_r"):
            assert cfg[key] == cfg0[key], key
    for band in ("g", "r"):
        p, p0 = Param.fromString("ulimb_" + band, cfg["ulimb_" + band]), Param.fromString("x", cfg0["ulimb_" + band])
        want = float("%.4f" % meds[band])
        assert p.currVal == want and p.prior.type == "gauss" and p.prior.p1 == want
        assert p.prior.p2 == p0.prior.p2 and p.isVar == p0.isVar
    for k in touched:                      # the columns are kept
        assert len(after[k]) == len(before[k])
        assert after[k].index(b"gauss") == before[k].index(b"gauss")
    kg5 = [l for l in after if l.strip().startswith(b"ulimb_KG5")]
    assert kg5 and kg5 == [l for l in before if l.strip().startswith(b"ulimb_KG5")]
    # in place, and a prior that is not gauss keeps its p1; a text too long for its columns still parses
    text = b"ulimb_g = 0.3 uniform 0.0 1.0 0  # a comment\n   ulimb_R=0.284 gauss 0.284 0.001\nulimb_KG5 = 0.1 gauss 0.1 0.01\n"
    small = tmp_path / "small.dat"
    small.write_bytes(text)
    assert limbdark.update_input(str(small), meds) == ["g", "R"]
    lines = small.read_bytes().splitlines(keepends=True)
    assert lines[0] == b"ulimb_g = 0.3568 uniform 0.0 1.0 0  # a comment\n"
    assert lines[1] == b"   ulimb_R=0.3123 gauss 0.3123 0.001\n" and lines[2] == text.splitlines(keepends=True)[2]


def test_loader_errors(tmp_path):
    from lfit_python_amd import limbdark
    base = tmp_path / "tables"
    shutil.copytree(ldd.LD_DIR, base)
    assert limbdark.load_ld_tables(str(base)).c.tobytes() == ldd.tables().c.tobytes()
    path = base / "Gianninas13" / "ld_coeffs_i.txt"
    text = path.read_text().splitlines(keepends=True)
    path.unlink()
    with pytest.raises(FileNotFoundError) as e:
        limbdark.load_ld_tables(str(base))
    assert "ld_coeffs_i.txt" in str(e.value)
    data = [k for k, l in enumerate(text) if not l.startswith("#")]
    path.write_text("".join(text[:data[100]] + text[data[100] + 1:]))        # one row removed
    with pytest.raises(ValueError) as e:
        limbdark.load_ld_tables(str(base))
    assert "ld_coeffs_i.txt" in str(e.value)
    shifted = list(text)                                                     # a full grid, but another one
    for k in data:
        if shifted[k].split()[1] == "12000":
            shifted[k] = shifted[k].replace(" 12000 ", " 12100 ", 1)
    assert shifted != text
    path.write_text("".join(shifted))
    with pytest.raises(ValueError) as e:
        limbdark.load_ld_tables(str(base))
    assert "differs" in str(e.value)
