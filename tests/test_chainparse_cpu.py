"""CPU: chain_prod.txt's numbers read back (MODEL_SPEC.md section 18) without a GPU.

  * the host twin (lfg_chainparse.hpp compiled for the host) through
    chainparse.parse_text against Python's float() (tests/chainparse_cases.py),
    8 bytes for 8 bytes: every token list, the long tokens included, and every
    structure case; it refuses nothing;
  * sampler.read_chain, mcmc_utils.readchain and readflatchain against the
    np.loadtxt / pandas expressions they used to be, on files from write_chain;
  * the fallbacks: a comment line, walker numbers out of order, no twin;
  * the committed table of powers of five against its generator;
  * the C ABI's set of names.
"""
import os
import re

import numpy as np
import pytest

from lfit_python_amd import _native, chainparse, mcmc_utils, sampler
from tests import chainparse_cases as cc
from tests import chaintext_double as ct


@pytest.fixture(scope="module", autouse=True)
def twin_library(tmp_path_factory):
    """the tree's twin where build() left it, else one built for this module"""
    keep = chainparse._twin, chainparse.TWIN_PATH
    if chainparse.twin() is None:
        from cpu_baseline import cpu
        so = str(tmp_path_factory.mktemp("chainparse") / "liblfg_cpu.so")
        cpu.build(out=so)
        chainparse._twin, chainparse.TWIN_PATH = None, so
        assert chainparse.twin() is not None
    yield
    chainparse._twin, chainparse.TWIN_PATH = keep


@pytest.fixture(scope="module")
def tile():
    return chainparse.tile_bytes()


def old_read_chain(fname):
    """sampler.read_chain as it was: the double"""
    data = np.loadtxt(fname, skiprows=1)
    nw = int(data[:, 0].max()) + 1
    ns = data.shape[0] // nw
    chain = np.full((nw, ns, data.shape[1] - 1), np.nan)
    for i in range(nw):
        chain[i] = data[data[:, 0] == i, 1:]
    return chain


def old_readflatchain(file):
    import pandas as pd
    return np.array(pd.read_csv(file, header=None, sep=r"\s+", float_precision="round_trip"))


@pytest.mark.parametrize("name", sorted(cc.LISTS))
def test_twin_equals_float_on_the_token_lists(name):
    text, want, tokens = cc.list_case(name)
    assert len(tokens) >= {"roundtrip": 400000, "digits17_19": 10000, "ties": 3000, "long": 1400}.get(name, 50)
    out, info = chainparse.parse_host(text, 1)
    assert list(info) == [len(tokens), len(tokens), 0, 0, 0, -1, 0, 0]   # refused: 0, the long tokens included
    bad = cc.same(out, want)
    assert bad.size == 0, [(tokens[i], out[i, 0], want[i, 0]) for i in bad[:5]]


def test_the_lists_hold_what_they_are_meant_to():
    assert float("2.4703282292062327e-324") == 0.0 and float("2.4703282292062328e-324") == 5e-324
    assert float("1.797693134862315807e308") == 1.7976931348623157e308 and float("1.797693134862315808e308") == np.inf
    assert float("9007199254740993") == 2.0 ** 53
    assert all(t in cc.EDGES for t in ("1e99999999999999999999", "-0.000000", "0e999", ".5", "5.", "+1", "-nan"))
    assert cc.significant_digits("0000000000001234567890123456789") == 19
    assert cc.significant_digits("1.234567890123456789000000000000e-5") == 19 and cc.significant_digits("0.00120") == 2
    long = cc.long()
    may = [cc.may_refuse(t) for t in long]
    assert sum(may) > 1300 and not all(may)
    assert sum(len(t) == cc.MAX_TOKEN + 1 for t in long) >= 5 and max(map(len, long)) > 300
    want = cc.expected(cc.digits17_19())
    be = (np.abs(want).view(np.uint64) >> np.uint64(52)).astype(int)
    assert set(range(0, 2047)) <= set(be[np.isfinite(want)])        # every binade, the subnormals' too
    assert (want == 0).any() and np.isinf(want).any()               # underflow to zero, overflow
    for t in [t for t in cc.ties()[::4] if t.isdigit()][:200]:                              # (2m + 1) * 2^e: half-even decides
        m = int(t)
        lo = m - (m & -m)                                           # the double below: the lowest set bit cleared
        assert int(float(t)) in (lo, lo + 2 * (m & -m)) and (int(float(t)) // (2 * (m & -m))) % 2 == 0


def test_structure(tile):
    cases = cc.structure_cases(tile)
    assert len(cases) >= 35
    for name, text, ncol, want in cases:
        for data in (text, bytearray(text), memoryview(text), np.frombuffer(text, np.uint8)):
            out = chainparse.parse_text(data, ncol)
            assert out.shape == want.shape, (name, out.shape, want.shape)
            assert cc.same(out, want).size == 0, name
    import torch
    name, text, ncol, want = cases[0]
    out = chainparse.parse_text(torch.from_numpy(np.frombuffer(text, np.uint8).copy()), ncol)
    assert isinstance(out, np.ndarray) and cc.same(out, want).size == 0


def test_every_seam(tile):
    for shift in range(cc.MAX_TOKEN + 2):
        text, want = cc.shifted(tile, shift)
        assert cc.same(chainparse.parse_text(text, 2), want).size == 0, shift


def test_ragged_rows_and_bad_tokens_name_the_first_row():
    for name, text, ncol, row in cc.ragged_cases():
        with pytest.raises(ValueError, match="row %d has not" % row):
            chainparse.parse_text(text, ncol)
    for tok, text, row in cc.bad_files():
        with pytest.raises(ValueError, match="row %d holds" % row):
            chainparse.parse_text(text, 3)
    with pytest.raises(ValueError):
        chainparse.parse_text(b"1 2\n", cc.MAX_NCOL + 1)
    with pytest.raises(TypeError):
        chainparse.parse_text(np.zeros(4, np.int32))


def write(tmp_path, chain, lnp, name="chain_prod.txt"):
    path = str(tmp_path / name)
    names = ["p%d" % i for i in range(chain.shape[2])]
    sampler.write_chain(path, names, chain, lnp)
    return path, names


def test_readers_equal_the_loadtxt_route(tmp_path, monkeypatch):
    used = []
    real = chainparse.parse_host
    monkeypatch.setattr(chainparse, "parse_host", lambda *a, **k: (used.append(1), real(*a, **k))[1])
    for k, (steps, W, ndim) in enumerate(((7, 5, 18), (3, 4, 1), (2, 3, 87), (1, 2, 3), (40, 1, 2))):
        chain, lnp = ct.block_case(steps, W, ndim, seed=k)
        path, names = write(tmp_path, chain, lnp, "c%d.txt" % k)
        want = old_read_chain(path)
        n = len(used)
        for got in (sampler.read_chain(path), mcmc_utils.readchain(path), mcmc_utils.readchain_dask(path)):
            assert got.shape == want.shape == (W, steps, ndim + 1) and got.flags.c_contiguous
            assert cc.same(got, want).size == 0
        assert len(used) == n + 3                    # through the parser, not through the fallback
        assert cc.same(want[:, :, :-1].transpose(1, 0, 2), chain).size == 0
        grid, got_names = chainparse.read_chain(path)
        assert got_names == names + ["ln_prob"] and cc.same(grid, want.transpose(1, 0, 2)).size == 0
        assert cc.same(chainparse.read_table(path, skip_lines=1)[:, 1:], want.transpose(1, 0, 2)).size == 0
    # a tempered run's cold level, written from its strided view
    chain, lnp = ct.block_case(6, 4 * 5, 3, seed=1)          # [steps][T = 4][W = 5]
    c4, l4 = chain.reshape(6, 4, 5, 3), lnp.reshape(6, 4, 5)
    path, _ = write(tmp_path, c4[:, 0], l4[:, 0], "cold.txt")
    want = old_read_chain(path)
    assert cc.same(sampler.read_chain(path), want).size == 0 and want.shape == (5, 6, 4)


def test_readflatchain_equals_pandas(tmp_path, monkeypatch):
    used = []
    real = chainparse.parse_host
    monkeypatch.setattr(chainparse, "parse_host", lambda *a, **k: (used.append(1), real(*a, **k))[1])
    chain, lnp = ct.block_case(9, 4, 5, seed=4)
    flat = chain.reshape(-1, 5)
    flat = flat[np.isfinite(flat).all(axis=1)]
    path = str(tmp_path / "flat.txt")
    with open(path, "w") as fh:
        for r in flat:
            fh.write(" ".join(map(repr, map(float, r))) + "\n")
    got, want = mcmc_utils.readflatchain(path), old_readflatchain(path)
    assert got.dtype == want.dtype and got.shape == want.shape and cc.same(got, want).size == 0 and used
    # whole numbers only: pandas keeps integers, and so does readflatchain
    with open(path, "w") as fh:
        fh.write("1 2 3\n4 5 6\n")
    got, want = mcmc_utils.readflatchain(path), old_readflatchain(path)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    # a header of names: pandas' array of objects, as before
    with open(path, "w") as fh:
        fh.write("a b\n1.5 2\n")
    got, want = mcmc_utils.readflatchain(path), old_readflatchain(path)
    assert got.dtype == want.dtype == object and got.tolist() == want.tolist()


def test_fallbacks(tmp_path, monkeypatch):
    chain, lnp = ct.block_case(4, 3, 2, seed=9)
    chain, lnp = np.round(chain, 6) % 1000.0, -np.abs(lnp) % 1000.0
    chain[~np.isfinite(chain)] = 0.25
    lnp[~np.isfinite(lnp)] = -0.5
    path, names = write(tmp_path, chain, lnp)
    lines = open(path).read().split("\n")
    # a comment line inside the data: '#' is no number; np.loadtxt skips it
    commented = str(tmp_path / "commented.txt")
    with open(commented, "w") as fh:
        fh.write("\n".join(lines[:4] + ["# a remark"] + lines[4:]))
    with pytest.raises(ValueError, match="row 3 "):
        chainparse.read_chain(commented)
    assert cc.same(sampler.read_chain(commented), old_read_chain(path)).size == 0
    # walker numbers out of order: the gather per walker sorts them
    shuffled = str(tmp_path / "shuffled.txt")
    body = lines[1:-1]
    body[0], body[1] = body[1], body[0]
    with open(shuffled, "w") as fh:
        fh.write("\n".join(lines[:1] + body) + "\n")
    with pytest.raises(ValueError, match="walker numbers"):
        chainparse.read_chain(shuffled)
    assert cc.same(sampler.read_chain(shuffled), old_read_chain(path)).size == 0
    # rows that do not divide among the walkers
    with open(shuffled, "w") as fh:
        fh.write("\n".join(lines[:-2]) + "\n")
    with pytest.raises(ValueError, match="do not divide"):
        chainparse.read_chain(shuffled)
    for reader in (old_read_chain, sampler.read_chain):   # (raised before and raises now, the same way)
        with pytest.raises(ValueError, match="could not broadcast"):
            reader(shuffled)
    # a file of one row raised before and raises now
    with open(shuffled, "w") as fh:
        fh.write("\n".join(lines[:2]) + "\n")
    with pytest.raises(IndexError):
        old_read_chain(shuffled)
    with pytest.raises(IndexError):
        sampler.read_chain(shuffled)
    # no twin: TwinMissing from the parser, the earlier reader for the callers
    monkeypatch.setattr(chainparse, "_twin", False)
    with pytest.raises(chainparse.TwinMissing):
        chainparse.parse_text(b"1 2\n")
    assert cc.same(sampler.read_chain(path), old_read_chain(path)).size == 0
    assert chainparse.try_table(path, 1) is None


def test_the_table_equals_its_regenerated_self():
    from lfit_python_amd import gen_chainparse_table as gen
    with open(gen.PATH) as fh:
        text = fh.read()
    assert text == gen.text()
    got = [(int(a, 16), int(b, 16)) for a, b in re.findall(r"\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\}", text)]
    assert len(got) == gen.Q_MAX - gen.Q_MIN + 1 == 651
    # independently of the generator's own arithmetic: the row is 5^q scaled by a power of two into
    # [2^127, 2^128), from below by less than one unit for q >= 0, within one unit for q < 0
    for q, (hi, lo) in zip(range(gen.Q_MIN, gen.Q_MAX + 1), got):
        g = (hi << 64) | lo
        assert g >> 127 == 1
        if q >= 0:
            p = 5 ** q
            sh = p.bit_length() - 128
            assert (g << sh <= p < (g + 1) << sh) if sh >= 0 else (g == p << -sh)
        else:
            p = 5 ** -q
            b = p.bit_length() + 127          # 2^127 <= 2^b / p < 2^128
            assert abs(g * p - (1 << b)) < p
            if q >= -27:
                assert (g - 1) * p <= (1 << b) < g * p   # (never below the true value where a tie can be)
    hpp = open(os.path.join(_native._HERE, "csrc", "lfg_chainparse.hpp")).read()
    assert "CP_Q_MIN = %d, CP_Q_MAX = %d" % (gen.Q_MIN, gen.Q_MAX) in hpp


def test_abi_set_and_sources():
    assert set(_native.EXPORTS_CHAINPARSE) == {"lfg_chain_parse_tile_bytes", "lfg_chain_parse_workspace_size",
                                               "lfg_chain_parse_count", "lfg_chain_parse"}
    for other in (_native.EXPORTS, _native.EXPORTS_PHYSPAR, _native.EXPORTS_WD, _native.EXPORTS_CHAIN,
                  _native.EXPORTS_LIMBDARK, _native.EXPORTS_CORNER, _native.EXPORTS_CHAINTEXT):
        assert not set(_native.EXPORTS_CHAINPARSE) & set(other)
    path = os.path.join(_native.REPO, "include", "lfg_chainparse.h")
    code = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert set(re.findall(r"\b(lfg_\w+)\s*\(", code)) == set(_native.EXPORTS_CHAINPARSE)
    text = open(os.path.join(_native.REPO, "include", "lfg.h")).read()
    assert not any(f in text for f in _native.EXPORTS_CHAINPARSE)
    assert path in _native.HEADERS
    for f in ("lfg_chainparse.hpp", "lfg_chainparse_table.hpp"):
        assert os.path.join(_native._HERE, "csrc", f) in _native.HEADERS
    assert any(p.endswith("lfg_chainparse.hip") for p in _native.SOURCES)
    head = open(path).read()
    assert ("#define LFG_CHAIN_PARSE_MAX_TOKEN %d" % _native.CHAIN_PARSE_MAX_TOKEN) in head
    assert _native.CHAIN_PARSE_MAX_TOKEN >= 32 and cc.MAX_TOKEN == _native.CHAIN_PARSE_MAX_TOKEN
    assert _native.CHAIN_PARSE_MAX_NCOL == cc.MAX_NCOL >= _native.CHAIN_TEXT_MAX_NDIM + 2
    twin_h = open(os.path.join(_native.REPO, "cpu_baseline", "lfg_cpu.h")).read()
    assert "lfg_cpu_chain_parse_count" in twin_h and "lfg_cpu_chain_parse(" in twin_h
    assert chainparse.tile_bytes() % 16 == 0
