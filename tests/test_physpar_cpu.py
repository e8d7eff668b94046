"""CPU: physical parameters (MODEL_SPEC section 12) without a GPU: the table
loader and its packing, the host twin lfg_cpu_physpar (the text the gfx950
kernel compiles) against the numpy / scipy double of tests/physpar_double.py
on the fixed batch, and against the reference's own solve()
(tests/golden/physpar_ref.npz, tools/make_physpar_golden.py).

Tolerances.  Against the tight double (brentq, xtol = 1e-15): status and model
equal everywhere, columns to rtol 1e-11, incl to 1e-9 degrees: the project's
own pins propagated (xl1 at 1e-13 and findi at 1e-9 degrees in
tests/test_gpu_parity.py); the root's own error is ~1e-16, since f rounds at
~1e-18 and f' is ~1e-2.  Against the reference fixture, which ran brentq at
its defaults: see test_twin_matches_the_reference_fixture.
"""
import ctypes
import os
import shutil

import numpy as np
import pytest

from tests import physpar_double as ppd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, INCL_ATOL = 1e-11, 1e-9
# ten times the largest relative difference between the double at brentq's default
# tolerance and at xtol = 1e-15 on the fixed batch (3.3941e-12, in Mw and Mr)
GOLDEN_RTOL = 3.3941e-11


@pytest.fixture(scope="module")
def tables():
    from lfit_python_amd import physpar
    return physpar.load_mr_tables(ppd.WD_MODELS)


@pytest.fixture(scope="module")
def twin(tables):
    from cpu_baseline import cpu
    if not os.path.exists(cpu.LIB_PATH):
        cpu.build()
    b, _ = ppd.shared(True)
    return cpu.CpuPort().physpar(b["q"], b["dphi"], b["rw"], b["T"], b["P"], tables)


def compare(table, model, status, ref, rtol=RTOL):
    """the module docstring's comparison; returns the largest relative difference"""
    assert np.array_equal(status, ref["status"]), np.flatnonzero(status != ref["status"])[:10]
    assert np.array_equal(model, ref["model"]), np.flatnonzero(model != ref["model"])[:10]
    ok = ref["status"] == 0
    assert np.all(np.isnan(table[~ok])) and np.all(model[~ok] == -1)
    assert np.all(np.isfinite(table[ok]))
    a, r = table[ok], ref["table"][ok]
    rel = np.abs(a[:, :9] - r[:, :9]) / np.abs(r[:, :9])
    print("largest relative difference per column", rel.max(axis=0), "incl", np.abs(a[:, 9] - r[:, 9]).max())
    assert rel.max() <= rtol, rel.max(axis=0)
    assert np.abs(a[:, 9] - r[:, 9]).max() <= INCL_ATOL
    return rel.max()


# ------------------------------------------------------------------ the batch itself
def test_fixed_batch_populations():
    """before anything is trusted: every branch and status is populated, the
    edge rows sit where they were placed, and f is monotone on every row"""
    b, ref = ppd.shared(True)
    st, mo = ref["status"], ref["model"]
    valid = np.isin(st, (0, 6))
    assert 1900 <= len(st) <= 2100
    for k, name in enumerate(("wood", "panei", "hamada")):
        frac = np.mean(mo[valid] == k)
        print(name, frac)
        assert frac >= 0.05, (name, frac)
    assert np.mean(st[valid] == 6) >= 0.05
    assert set(np.unique(st)) == {0, 1, 2, 5, 6}
    assert ref["monotone"].all()
    for row, k, inside in b["edge"]:
        assert (mo[row] == k) == inside, (row, k, inside, mo[row])
        if inside:
            lo, hi = ppd.LIMITS[k][1:]
            assert min(abs(ref["table"][row, 1] - lo), abs(ref["table"][row, 1] - hi)) < 2e-6
    # the Panei gate's rows: 5000 and below 45000 inside, the others not
    gate = np.flatnonzero((b["T"] >= 4999.0) & (b["T"] <= 5001.0) | (b["T"] >= 44999.0) & (b["T"] <= 45001.0))
    gate = gate[gate >= b["n_base"]]
    assert len(gate) == 5
    for i in gate:
        assert (mo[i] == 1) == (5000.0 <= b["T"][i] < 45000.0), (i, b["T"][i], mo[i])


# ------------------------------------------------------------------ loader
def test_loader_shapes_and_units(tables):
    A = tables.arrays
    assert list(tables.wood_off) == [0, 80, 162, 247, 338, 437, 536, 635]
    assert A["wood_t"].shape == A["wood_r"].shape == (635,)
    for k in range(7):
        t = A["wood_t"][tables.wood_off[k]:tables.wood_off[k + 1]]
        r = A["wood_r"][tables.wood_off[k]:tables.wood_off[k + 1]]
        # K: every file starts cooler than the batch's 4 000 K and ends hotter than its 50 000 K
        assert np.all(np.diff(t) > 0) and t[0] < 4000.0 and t[-1] > 5e4
        assert np.all((r > 0.003) & (r < 0.1))            # R_sun: white-dwarf radii
    # radii fall with mass at a fixed temperature
    r15 = [np.interp(15000.0, A["wood_t"][a:b], A["wood_r"][a:b]) for a, b in zip(tables.wood_off, tables.wood_off[1:])]
    assert np.all(np.diff(r15) < 0)
    assert A["ham_m"].shape == A["ham_r"].shape == (1305,) and np.all(np.diff(A["ham_m"]) > 0)
    assert A["ham_m"][0] <= 0.14 and A["ham_m"][-1] >= 1.44 and 0.0005 < A["ham_r"].min() and A["ham_r"].max() < 0.05
    assert A["wood_card"].shape == (6 * 7 * 4,)
    nx, ny = A["pan_tx"].size, A["pan_ty"].size
    assert (nx, ny) == (8, 8) and A["pan_c"].size == (nx - 4) * (ny - 4)
    assert A["pan_tx"][0] == 5000.0 and A["pan_tx"][-1] == 145000.0 and A["pan_ty"][0] == 0.3 and A["pan_ty"][-1] == 1.2
    assert tables.constants == {"G": 6.67430e-11, "GMsun": 1.3271244e20, "Rsun": 6.957e8, "day": 86400.0}
    T = tables.host_struct()
    assert T.n_ham == 1305 and list(T.wood_off) == list(tables.wood_off) and T.Rsun == 6.957e8


def test_loader_cuts_the_two_non_monotone_files(tables):
    from lfit_python_amd import physpar
    assert tables.wood_cut == (0, 0, 0, 0, 1, 0, 1)          # co080 and co100: one row each at the hot end
    first = []
    for f, cut in zip(physpar.WOOD_FILES, tables.wood_cut):
        y = np.loadtxt(os.path.join(ppd.WD_MODELS, f), usecols=(6,))
        t = (10.0 ** y)[::-1]
        assert (np.sum(np.diff(t) <= 0) > 0) == (cut > 0)
        if cut:
            j = np.flatnonzero(np.diff(t) <= 0)[0]
            first.append((t[j], t[j + 1]))
    # the coolest temperature a file descends to: 126 444 K (log T is given to 1e-4)
    assert len(first) == 2 and abs(min(d for _, d in first) / 126444.0 - 1.0) < 3e-4
    # what is kept increases, and ends on the row before the descent
    for k in (4, 6):
        t = tables.arrays["wood_t"][tables.wood_off[k]:tables.wood_off[k + 1]]
        assert np.all(np.diff(t) > 0) and t[-1] in [a for a, _ in first]


def test_loader_missing_file_and_either_panei_name(tmp_path):
    from lfit_python_amd import physpar
    base = tmp_path / "wd"
    shutil.copytree(ppd.WD_MODELS, base)
    pdir = base / "Panei" / "12C-MR-H-He"
    os.rename(pdir / "12C-MR-H-He.saver", pdir / "12C-MR-H-He.dat")
    t = physpar.load_mr_tables(str(base))                   # the name the reference's code opens
    assert t.arrays["pan_c"].size == 16
    os.remove(pdir / "12C-MR-H-He.dat")
    with pytest.raises(FileNotFoundError):
        physpar.load_mr_tables(str(base))
    shutil.copy(os.path.join(ppd.WD_MODELS, "Panei", "12C-MR-H-He", "12C-MR-H-He.saver"), pdir)
    os.remove(base / "Wood95" / "co070.2.04dt1")
    with pytest.raises(FileNotFoundError):
        physpar.load_mr_tables(str(base))
    shutil.copy(os.path.join(ppd.WD_MODELS, "Wood95", "co070.2.04dt1"), base / "Wood95")
    os.remove(base / "Hamada" / "mr_hamada.dat")
    with pytest.raises(FileNotFoundError):
        physpar.load_mr_tables(str(base))


def test_cardinal_cubics_match_interp1d():
    from scipy.interpolate import interp1d
    from lfit_python_amd import physpar
    card = physpar.cardinal_cubics()
    rng = np.random.default_rng(5)
    grid = np.linspace(0.4, 1.0, 101)
    for _ in range(20):
        rk = rng.uniform(0.005, 0.02, 7)
        want = interp1d(physpar.WOOD_MASSES, rk, kind="cubic")(grid)
        assert np.max(np.abs(physpar.eval_cardinal(card, rk, grid) - want)) <= 1e-15


def test_numpy_de_boor_matches_the_spline(tables):
    from scipy.interpolate import SmoothBivariateSpline
    from lfit_python_amd import physpar
    teff, mass, radius = tables.panei_data
    spl = SmoothBivariateSpline(teff, mass, radius)
    T, m = np.meshgrid(np.linspace(5000.0, 45000.0, 20), np.linspace(0.4, 1.2, 20), indexing="ij")
    want = spl(T[:, 0], m[0])
    got = physpar.eval_bispline(tables.arrays["pan_tx"], tables.arrays["pan_ty"], tables.arrays["pan_c"], T, m)
    assert np.max(np.abs(got / want - 1.0)) <= 1e-13


# ------------------------------------------------------------------ the host twin
def test_twin_matches_the_tight_double(twin):
    _, ref = ppd.shared(True)
    compare(*twin, ref)


def test_twin_strided_zero_rows_and_argument_errors(tables):
    from cpu_baseline import cpu
    from lfit_python_amd import _native
    b, _ = ppd.shared(True)
    port = cpu.CpuPort()
    n, ndim = 97, 5
    chain = np.zeros((n, ndim))
    chain[:, 3], chain[:, 0], chain[:, 4] = b["q"][:n], b["dphi"][:n], b["rw"][:n]
    flat = chain.reshape(-1)
    want = port.physpar(b["q"][:n], b["dphi"][:n], b["rw"][:n], b["T"][:n], b["P"][:n], tables)
    got = port.physpar(flat[3:], flat[0:], flat[4:], b["T"][:n], b["P"][:n], tables, ld=ndim, n=n, nthreads=3)
    for a, w in zip(got, want):
        assert np.array_equal(a, w, equal_nan=True)
    f = port.lib.lfg_cpu_physpar
    T = tables.host_struct()
    one = np.ones(4)
    dp, ip = one.ctypes.data_as(cpu._dp), np.zeros(4, np.int32).ctypes.data_as(cpu._ip)
    out = np.zeros(40).ctypes.data_as(cpu._dp)
    assert f(None, None, None, 1, None, None, 0, ctypes.byref(T), None, None, None, 1) == 0     # n = 0: nothing to do
    assert f(dp, dp, dp, 1, dp, dp, -1, ctypes.byref(T), out, ip, ip, 1) == -1
    assert f(dp, dp, dp, 0, dp, dp, 4, ctypes.byref(T), out, ip, ip, 1) == -1
    assert f(dp, dp, dp, 1, dp, dp, 4, None, out, ip, ip, 1) == -1
    assert f(None, dp, dp, 1, dp, dp, 4, ctypes.byref(T), out, ip, ip, 1) == -1
    bad = tables.host_struct()
    bad.pan_nx = _native.MR_MAX_KNOTS + 1
    assert f(dp, dp, dp, 1, dp, dp, 4, ctypes.byref(bad), out, ip, ip, 1) == -1
    bad = tables.host_struct()
    bad.wood_off[3] = bad.wood_off[2] + 1
    assert f(dp, dp, dp, 1, dp, dp, 4, ctypes.byref(bad), out, ip, ip, 1) == -1


def test_library_refuses_bad_arguments_before_any_launch(tables):
    """lfg_physpar's argument errors need no GPU: LFG_E_ARGS before a launch, n = 0 a no-op"""
    from lfit_python_amd import _native
    L = _native.lib()
    for s in _native.EXPORTS_PHYSPAR:
        assert hasattr(L, s)
    assert not set(_native.EXPORTS_PHYSPAR) & set(_native.EXPORTS)
    T = tables.host_struct()      # host pointers: never dereferenced by these calls
    vp8 = ctypes.c_void_p(8)
    assert L.lfg_physpar(None, None, None, 1, None, None, 0, ctypes.byref(T), None, None, None, None) == 0
    assert L.lfg_physpar(vp8, vp8, vp8, 1, vp8, vp8, -1, ctypes.byref(T), vp8, vp8, vp8, None) == -1
    assert L.lfg_physpar(vp8, vp8, vp8, 0, vp8, vp8, 4, ctypes.byref(T), vp8, vp8, vp8, None) == -1
    assert L.lfg_physpar(vp8, vp8, vp8, 1, vp8, vp8, 4, None, vp8, vp8, vp8, None) == -1
    assert L.lfg_physpar(vp8, vp8, None, 1, vp8, vp8, 4, ctypes.byref(T), vp8, vp8, vp8, None) == -1
    bad = tables.host_struct()
    bad.n_ham = _native.MR_MAX_DOUBLES
    assert L.lfg_physpar(vp8, vp8, vp8, 1, vp8, vp8, 4, ctypes.byref(bad), vp8, vp8, vp8, None) == -1
    assert L.lfg_physpar_lanes() >= 256


def test_struct_layout_matches_ctypes(tmp_path):
    import subprocess
    from lfit_python_amd import _native
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include "lfg_physpar.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(lfg_mr_tables), offsetof(lfg_mr_tables, wood_off),
         offsetof(lfg_mr_tables, wood_card), offsetof(lfg_mr_tables, n_ham), offsetof(lfg_mr_tables, pan_tx),
         offsetof(lfg_mr_tables, pan_nx), offsetof(lfg_mr_tables, G));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    T = _native.LfgMrTables
    assert got == [ctypes.sizeof(T), T.wood_off.offset, T.wood_card.offset, T.n_ham.offset, T.pan_tx.offset,
                   T.pan_nx.offset, T.G.offset]


def test_twin_matches_the_reference_fixture(twin):
    """Against the reference's own solve() (brentq at scipy's defaults, which
    bound Mw's error by about 4e-12 absolute).  The rows that returned None
    match exactly.  The column tolerance is measured, not fixed in advance,
    because near the Hamada end Rw's sensitivity to Mw is large: the double
    run at both tolerances on the fixed batch differs by at most 3.3941e-12
    relative (in Mw and Mr; 1.13e-12 in Rw, Rr, a, Kw, Kr, 7.1e-14 in logg);
    the bound is ten times that, 3.3941e-11.  Measured against the fixture:
    3.3967e-12, and 5.8e-12 degrees in incl."""
    table, model, status = twin
    g = np.load(os.path.join(ROOT, "tests", "golden", "physpar_ref.npz"))
    b, tight = ppd.shared(True)
    for k in ("q", "dphi", "rw", "T", "P"):
        assert np.array_equal(g[k], b[k], equal_nan=True), k   # the fixture is of this batch
    valid = np.isin(status, (0, 6))                  # the rows whose inputs the reference's code is defined on
    assert np.array_equal(g["none"][valid], status[valid] == 6)
    assert not g["raised"][valid].any() and np.all(status[g["raised"]] == 2)   # it raises where findi does
    _, loose = ppd.shared(False)
    ok = status == 0
    spread = np.max(np.abs(loose["table"][ok] - tight["table"][ok]) / np.abs(tight["table"][ok]))
    print("double, default against tight: %.4e" % spread)
    assert 0.5 * GOLDEN_RTOL <= 10.0 * spread <= 2.0 * GOLDEN_RTOL      # the bound is still ten times the spread
    a, r = table[ok], g["table"][ok]
    rel = np.abs(a[:, :9] - r[:, :9]) / np.abs(r[:, :9])
    print("twin against the fixture: %.4e, incl %.2e degrees" % (rel.max(), np.abs(a[:, 9] - r[:, 9]).max()))
    assert rel.max() <= GOLDEN_RTOL
    assert np.abs(a[:, 9] - r[:, 9]).max() <= INCL_ATOL
