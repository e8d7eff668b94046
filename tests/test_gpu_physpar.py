"""GPU: lfg_physpar (include/lfg_physpar.h; MODEL_SPEC section 12) and
lfit_python_amd.physpar on the device.

  parity    the fixed batch of tests/physpar_double.py against the tight
            double (brentq at xtol = 1e-15, the oracle's xl1 / findi): status
            and model equal everywhere, columns to rtol 1e-11, incl to 1e-9
            degrees (tests/test_physpar_cpu.py's tolerances and their reasons)
  counts    n of 1, 63, 64, 65, 255, 256, 257 and one count beyond a launch's
            lanes (the grid-stride loop's second trip): row i of any batch is
            bit-identical to the same row solved alone, and a second run of a
            batch to the first
  strides   a [steps][W][ndim] chain read in place (ld = ndim) and a thinned
            view of it (ld = thin ndim) against the contiguous call, bit for bit
  guards    tests/abi_guard.py's arena: out is exactly [10][n], model and
            status exactly [n], every element written, inputs and tables
            unchanged, guard bytes intact; the same on a side stream with the
            default stream kept busy
  python    from_chain, its seeded draws, summary against pandas, the CLI
All shapes are small: 257 rows solved alone are the reference of the counts.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import abi_guard as ag
from tests import physpar_double as ppd
from tests.test_physpar_cpu import compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 63, 64, 65, 255, 256, 257)
NROWS = 257


@pytest.fixture(scope="module")
def tables():
    from lfit_python_amd import physpar
    return physpar.load_mr_tables(ppd.WD_MODELS)


@pytest.fixture(scope="module")
def rows():
    """257 rows of the fixed batch: its special rows and base rows, shuffled"""
    b, ref = ppd.shared(True)
    n_all = len(b["q"])
    k = np.concatenate([np.arange(b["n_base"], n_all), np.arange(NROWS - (n_all - b["n_base"]))])
    k = k[np.random.default_rng(3).permutation(NROWS)]
    assert set(np.unique(ref["model"][k])) == {-1, 0, 1, 2} and set(np.unique(ref["status"][k])) == {0, 1, 2, 5, 6}
    return {name: b[name][k].copy() for name in ("q", "dphi", "rw", "T", "P")}


def _solve(r, tables, sel=slice(None)):
    from lfit_python_amd import physpar
    return physpar.solve(r["q"][sel], r["dphi"][sel], r["rw"][sel], r["T"][sel], r["P"][sel], tables)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    import torch
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def alone(rows, tables):
    """every one of the 257 rows solved alone: (table [257, 10], model, status)"""
    import torch
    got = [_solve(rows, tables, slice(i, i + 1)) for i in range(NROWS)]
    return tuple(torch.cat([g[k] for g in got]) for k in range(3))


def test_parity_with_the_tight_double(tables):
    b, ref = ppd.shared(True)
    table, model, status = _solve({k: b[k] for k in ("q", "dphi", "rw", "T", "P")}, tables)
    assert table.shape == (len(b["q"]), 10) and model.shape == status.shape == (len(b["q"]),)
    compare(table.cpu().numpy(), model.cpu().numpy(), status.cpu().numpy(), ref)


@pytest.mark.parametrize("n", COUNTS)
def test_rows_do_not_depend_on_the_batch(rows, tables, alone, n):
    first = _solve(rows, tables, slice(0, n))
    assert _same(first, tuple(a[:n] for a in alone))
    assert _same(_solve(rows, tables, slice(0, n)), first)


def test_grid_stride_second_trip(rows, tables, alone):
    import torch
    from lfit_python_amd import _native
    lanes = _native.lib().lfg_physpar_lanes()
    n = lanes + 300
    reps = -(-n // NROWS)
    big = {k: np.tile(v, reps)[:n] for k, v in rows.items()}
    first = _solve(big, tables)
    want = tuple(torch.cat([a] * reps)[:n] for a in alone)
    assert _same(first, want)
    assert _same(_solve(big, tables), first)


def _raw_call(tables, q, dphi, rw, ld, T, P, n):
    """lfg_physpar through ctypes on device tensors: (out [10][n], model, status)"""
    import torch
    from lfit_python_amd import _native
    dev = q.device
    out = torch.empty((10, n), dtype=torch.float64, device=dev)
    model = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    S = tables.device_struct(dev)
    rc = _native.lib().lfg_physpar(ag.ptr(q), ag.ptr(dphi), ag.ptr(rw), ld, ag.ptr(T), ag.ptr(P), n, ctypes.byref(S),
                                   ag.ptr(out), ag.ptr(model), ag.ptr(status), _native.stream_ptr(dev))
    assert rc == 0
    return out, model, status


def test_strided_chain_is_read_in_place(rows, tables):
    import torch
    steps, W, ndim, thin = 6, 5, 9, 3
    n = steps * W
    dev = torch.device("cuda", torch.cuda.current_device())
    chain = np.random.default_rng(8).uniform(-5.0, 5.0, (steps, W, ndim))
    flat_rows = chain.reshape(n, ndim)
    flat_rows[:, 4], flat_rows[:, 5], flat_rows[:, 8] = rows["q"][:n], rows["dphi"][:n], rows["rw"][:n]
    c = torch.as_tensor(chain, device=dev)
    flat = c.reshape(-1)
    col = {k: torch.as_tensor(rows[k][:n], device=dev) for k in rows}
    want = _raw_call(tables, col["q"], col["dphi"], col["rw"], 1, col["T"], col["P"], n)
    got = _raw_call(tables, flat[4:], flat[5:], flat[8:], ndim, col["T"], col["P"], n)
    assert _same(got, want) and torch.equal(c.cpu(), torch.as_tensor(chain))
    # a thinned view: every third row
    k = -(-n // thin)
    tcol = {key: v[::thin].contiguous() for key, v in col.items()}
    want = _raw_call(tables, tcol["q"], tcol["dphi"], tcol["rw"], 1, tcol["T"], tcol["P"], k)
    got = _raw_call(tables, flat[4:], flat[5:], flat[8:], thin * ndim, tcol["T"], tcol["P"], k)
    assert _same(got, want)


# ------------------------------------------------------------------ guarded buffers
MODEL_FILL = 0x5A5A5A5A   # model -1 is all-ones bytes, the arena's poison: this buffer gets a fill of its own


def _guarded(A, rows, tables, n):
    import torch
    from lfit_python_amd import _native
    tab = {name: A.inp("tab_" + name, a) for name, a in tables.arrays.items()}
    S = tables.struct_over(lambda name: tab[name].data_ptr())
    col = {k: A.inp(k, rows[k][:n]) for k in ("q", "dphi", "rw", "T", "P")}
    out = A.out("out", (10, n), torch.float64)
    model = A.out("model", (n,), torch.int32)
    status = A.out("status", (n,), torch.int32)
    model.fill_(MODEL_FILL)
    rc = _native.lib().lfg_physpar(ag.ptr(col["q"]), ag.ptr(col["dphi"]), ag.ptr(col["rw"]), 1, ag.ptr(col["T"]),
                                   ag.ptr(col["P"]), n, ctypes.byref(S), ag.ptr(out), ag.ptr(model), ag.ptr(status),
                                   A.stream_ptr())
    assert rc == 0
    A.check()                                   # guards intact, inputs and tables unchanged
    assert not A.poisoned("out").any() and not A.poisoned("status").any()
    assert not bool((model == MODEL_FILL).any())
    return out.t().clone(), model.clone(), status.clone()


@pytest.fixture(scope="module")
def arena():
    return ag.Arena(nbytes=16 * 1024 * 1024)


@pytest.mark.parametrize("n", (1, 257))
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


# ------------------------------------------------------------------ the Python surface
NAMES = ["wdFlux", "dFlux", "sFlux", "rsFlux", "q_core", "dphi_core", "rdisc", "ulimb", "rwd_core"]


@pytest.fixture(scope="module")
def chain(oracle):
    """4 walkers x 8 steps around q = 0.1, i = 85 degrees, rwd = 0.02: [steps][W][ndim]"""
    rng = np.random.default_rng(12)
    c = rng.uniform(0.0, 1.0, (8, 4, len(NAMES)))
    c[:, :, 4] = 0.1 * (1.0 + 0.02 * rng.standard_normal((8, 4)))
    c[:, :, 5] = oracle.findphi(0.1, 85.0) * (1.0 + 0.01 * rng.standard_normal((8, 4)))
    c[:, :, 8] = 0.02 * (1.0 + 0.05 * rng.standard_normal((8, 4)))
    return c


def test_from_chain_without_errors_is_solve_on_constants(chain, tables):
    import torch
    from lfit_python_amd import physpar
    flat = chain.reshape(-1, len(NAMES))
    want = physpar.solve(flat[:, 4], flat[:, 5], flat[:, 8], 15000.0, 0.07, tables)
    assert int((want[2] == 0).sum()) == 32
    dev_chain = torch.as_tensor(chain, device="cuda")
    for c in (dev_chain, chain, flat):           # S.chain_dev's shape, a host chain, a flat chain
        assert _same(physpar.from_chain(c, NAMES, 15000.0, 0.0, 0.07, 0.0, tables), want)
    # thinned by steps, as the reference's flatchain thins
    t2 = chain[::2].reshape(-1, len(NAMES))
    want2 = physpar.solve(t2[:, 4], t2[:, 5], t2[:, 8], 15000.0, 0.07, tables)
    assert _same(physpar.from_chain(dev_chain, NAMES, 15000.0, 0.0, 0.07, 0.0, tables, thin=2), want2)
    # a flat chain is thinned by rows, in place
    t3 = flat[::3]
    want3 = physpar.solve(t3[:, 4], t3[:, 5], t3[:, 8], 15000.0, 0.07, tables)
    assert _same(physpar.from_chain(flat, NAMES, 15000.0, 0.0, 0.07, 0.0, tables, thin=3), want3)


def test_long_inputs_are_cut_into_chunks(rows, tables, alone, chain, monkeypatch):
    """the path of more than 2^31 - 1 rows, with the limit lowered to 100 rows"""
    from lfit_python_amd import physpar
    flat = chain.reshape(-1, len(NAMES))
    want = physpar.from_chain(flat, NAMES, 15000.0, 0.0, 0.07, 0.0, tables, thin=3)
    monkeypatch.setattr(physpar, "MAX_ROWS", 100)
    assert _same(_solve(rows, tables), alone)                       # 257 rows: chunks of 100, 100 and 57
    monkeypatch.setattr(physpar, "MAX_ROWS", 4)
    assert _same(physpar.from_chain(flat, NAMES, 15000.0, 0.0, 0.07, 0.0, tables, thin=3), want)   # 11 rows: 4, 4, 3


def test_from_chain_draws_are_seeded(chain, tables):
    import torch
    from lfit_python_amd import physpar
    a = physpar.from_chain(chain, NAMES, 15000.0, 500.0, 0.07, 1e-4, tables, seed=5)
    b = physpar.from_chain(chain, NAMES, 15000.0, 500.0, 0.07, 1e-4, tables, seed=5)
    c = physpar.from_chain(chain, NAMES, 15000.0, 500.0, 0.07, 1e-4, tables, seed=6)
    fixed = physpar.from_chain(chain, NAMES, 15000.0, 0.0, 0.07, 0.0, tables)
    assert _same(a, b) and not torch.equal(a[0][:, 1], c[0][:, 1]) and not torch.equal(a[0][:, 1], fixed[0][:, 1])
    # the draws move the mass by what 500 K and 1e-4 d can: a few per cent at most
    assert float((a[0][:, 1] / fixed[0][:, 1] - 1.0).abs().max()) < 0.1


def test_summary_is_pandas_mean_and_std(rows, tables):
    import pandas as pd
    from lfit_python_amd import physpar
    table, model, status = _solve(rows, tables)
    s = physpar.summary(table, status)
    ok = status.cpu().numpy() == 0
    df = pd.DataFrame(table.cpu().numpy()[ok], columns=list(physpar.COLUMNS))
    np.testing.assert_allclose(s["mean"], df.mean().to_numpy(), rtol=1e-12)
    np.testing.assert_allclose(s["std"], df.std().to_numpy(), rtol=1e-10)
    assert s["solved"] == int(ok.sum()) and s["n"] == NROWS and s["fraction"] == ok.sum() / NROWS


def test_cli_writes_both_files(chain, tables, tmp_path):
    from lfit_python_amd import physpar, sampler
    fname = str(tmp_path / "chain_prod.txt")
    sampler.write_chain(fname, NAMES, chain, np.zeros(chain.shape[:2]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "lfit_python_amd.calcPhysicalParams", fname, "15000", "500", "0.07",
                        "1e-4", "--dir", ppd.WD_MODELS], cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "The chain contains 32 samples" in r.stdout and "Found solutions for 100 percent" in r.stdout
    assert "  q: {:.3f}".format(chain[:, :, 4].mean()) in r.stdout
    log = open(tmp_path / "physicalparams.log").read().splitlines()
    assert log[0] == "q Mw Rw logg Mr Rr a Kw Kr incl" and len(log) == 33
    data = np.array([[float(v) for v in line.split(" ")] for line in log[1:]])
    assert data.shape == (32, 10) and np.all(np.isfinite(data))
    lines = open(tmp_path / "physicalparams_summary.log").read().splitlines()
    assert len(lines) == 10
    for name, line, col in zip(physpar.COLUMNS, lines, data.T):
        m = re.fullmatch(r" *(\w+): (-?\d+\.\d{5}) \+/- (\d+\.\d{5})", line)
        assert m and m.group(1) == name and len(line.split(":")[0]) == max(5, len(name)), line
        assert abs(float(m.group(2)) - col.mean()) <= 1e-5 and abs(float(m.group(3)) - col.std(ddof=1)) <= 1e-5
        assert line in r.stdout
