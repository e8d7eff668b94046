"""CPU: chain_prod.txt's rows (MODEL_SPEC.md section 17) without a GPU.

  * the host twin lfg_cpu_chain_text (lfg_chaintext.hpp compiled for the
    host) against Python's own repr / '{:f}' / '{:4d}' (tests/
    chaintext_double.py), byte for byte: the hard doubles, the '{:f}' ties and
    carries, 2^63 and beyond, and the random lists;
  * the committed table of powers of ten against its generator;
  * the C ABI's set of names, and sampler.write_chain's file bytes.
"""
import os
import re

import numpy as np
import pytest

from lfit_python_amd import _native, chaintext, sampler
from tests import chaintext_double as ct


@pytest.fixture(scope="module")
def port(tmp_path_factory):
    from cpu_baseline import cpu
    so = str(tmp_path_factory.mktemp("chaintext") / "liblfg_cpu.so")
    cpu.build(out=so)
    return cpu.CpuPort(so)


def flat(port, chain, lnp, walker0=0):
    steps, W, ndim = chain.shape
    return port.chain_text(chain, steps, W, ndim, max(1, W * ndim), ndim, lnp, max(1, W), 1, walker0=walker0)


def test_the_hex_literals_are_the_doubles_they_name():
    H = ct.H
    assert H("0x1.0f0cf064dd592p+73") == 1e22 and H("0x1.52d02c7e14af6p+76") == 1e23
    assert H("0x1.0000000000000p+53") == 9007199254740993.0 == 2.0 ** 53
    assert H("0x1.1c37937e07fffp+53") == 9999999999999998.0 and H("0x1.e000000000000p+6") == 120.0
    assert H("0x1.a36e2eb1c432dp-14") == 1e-4 and H("0x1.4f8b588e368f1p-17") == 1e-5
    assert H("0x1.421f5f40d8376p-23") == 1.5e-7 and H("0x1.c6bf52634p+49") == 1e15 and H("0x1.1c37937e08p+53") == 1e16
    assert H("0x0.0000000000001p-1022") == 5e-324 and H("0x1.fffffffffffffp+1023") == 1.7976931348623157e308
    # what the issue checked by hand, in the oracle itself
    for x, s in ((1e16, "1e+16"), (1e15, "1000000000000000.0"), (1e-4, "0.0001"), (1e-5, "1e-05"),
                 (1.5e-7, "1.5e-07"), (5e-324, "5e-324"), (1.7976931348623157e308, "1.7976931348623157e+308")):
        assert repr(x) == s
    for x, s in ((0.0000005, "0.000000"), (1.0000005, "1.000001"), (-1e-300, "-0.000000")):
        assert "{:f}".format(x) == s


@pytest.mark.parametrize("name", sorted(ct.LISTS))
def test_twin_equals_python_on_the_value_lists(port, name):
    chain, lnp, want = ct.column_case(name, False)
    assert chain.shape[0] >= {"random_bits": 200000, "log_uniform": 200000}.get(name, 1)
    got = flat(port, chain, lnp)
    assert got == want, ct.first_difference(got, want)


def test_twin_formats_two_to_the_63_and_beyond(port):
    v = np.array(ct.refused())
    chain = np.ones((v.size, 1, 1))
    got = flat(port, chain, v.reshape(-1, 1))
    want = ct.rows(chain, v.reshape(-1, 1))
    assert got == want, ct.first_difference(got, want)
    assert max(len(r) for r in want.split(b"\n")) > 300


@pytest.mark.parametrize("shape,walker0", [((3, 5, 1), 0), ((2, 7, 18), 9995), ((1, 3, 87), 99998), ((4, 1, 2), 0),
                                           ((0, 4, 3), 0), ((3, 0, 3), 7)])
def test_twin_rows_walker_field_and_shapes(port, shape, walker0):
    chain, lnp = ct.block_case(*shape)
    got = flat(port, chain, lnp, walker0)
    want = ct.rows(chain, lnp, walker0)
    assert got == want, ct.first_difference(got, want)


def test_twin_reads_strided_views(port):
    """the cold level of a tempered chain and a thinned chain, as views"""
    chain, lnp = ct.block_case(6, 4 * 5, 3, seed=1)          # [steps][T = 4][W = 5]
    buf, lbuf = chain.reshape(-1), lnp.reshape(-1)
    got = port.chain_text(buf, 6, 5, 3, 4 * 5 * 3, 3, lbuf, 4 * 5, 1, offset=5 * 3, lnp_offset=5)  # level 1
    c4, l4 = chain.reshape(6, 4, 5, 3), lnp.reshape(6, 4, 5)
    assert got == ct.rows(c4[:, 1], l4[:, 1])
    got = port.chain_text(buf, 2, 20, 3, 3 * 20 * 3, 3, lbuf, 3 * 20, 1, offset=2 * 20 * 3, lnp_offset=2 * 20)
    assert got == ct.rows(chain[2::3], lnp[2::3])   # steps 2 and 5: the last element read is the buffer's last


def test_twin_refuses_bad_arguments(port):
    chain, lnp = ct.block_case(2, 3, 2)
    for kw in (dict(ndim=0), dict(ndim=_native.CHAIN_TEXT_MAX_NDIM + 1), dict(walker0=-1)):
        a = dict(ndim=2, walker0=0)
        a.update(kw)
        with pytest.raises(ValueError):
            port.chain_text(np.zeros(2 * 3 * 1100), 2, 3, a["ndim"], 3 * a["ndim"], a["ndim"], lnp, 3, 1,
                            walker0=a["walker0"])
    with pytest.raises(ValueError):
        port.chain_text(chain, 2, 3, 2, 0, 2, lnp, 3, 1)


def test_the_table_equals_its_regenerated_self():
    from lfit_python_amd import gen_chaintext_table as gen
    with open(gen.PATH) as fh:
        text = fh.read()
    assert text == gen.text()
    got = [(int(a, 16), int(b, 16)) for a, b in re.findall(r"\{0x([0-9a-f]{16})ull, 0x([0-9a-f]{16})ull\}", text)]
    assert len(got) == gen.K_MAX - gen.K_MIN + 1 == 617
    # independently of the generator's own arithmetic: the row brackets 10^k from above by less than one unit
    for k, (hi, lo) in zip(range(gen.K_MIN, gen.K_MAX + 1), got):
        g = (hi << 64) | lo
        assert g >> 127 == 1
        num, den = (10 ** k, 1) if k >= 0 else (1, 10 ** -k)
        sh = ((k * 1741647) >> 19) - 127
        # (g - 1) * 2^sh < 10^k <= g * 2^sh
        if sh >= 0:
            assert (g - 1) * den << sh < num <= g * den << sh
        else:
            assert (g - 1) * den < num << -sh <= g * den


def test_abi_set_and_sources():
    assert set(_native.EXPORTS_CHAINTEXT) == {"lfg_chain_text_bound", "lfg_chain_text_workspace_size",
                                              "lfg_chain_text_tile_rows", "lfg_chain_text"}
    for other in (_native.EXPORTS, _native.EXPORTS_PHYSPAR, _native.EXPORTS_WD, _native.EXPORTS_CHAIN,
                  _native.EXPORTS_LIMBDARK, _native.EXPORTS_CORNER):
        assert not set(_native.EXPORTS_CHAINTEXT) & set(other)
    path = os.path.join(_native.REPO, "include", "lfg_chaintext.h")
    code = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert set(re.findall(r"\b(lfg_\w+)\s*\(", code)) == set(_native.EXPORTS_CHAINTEXT)
    text = open(os.path.join(_native.REPO, "include", "lfg.h")).read()
    assert not any(f in text for f in _native.EXPORTS_CHAINTEXT)
    assert path in _native.HEADERS
    for f in ("lfg_chaintext.hpp", "lfg_chaintext_table.hpp"):
        assert os.path.join(_native._HERE, "csrc", f) in _native.HEADERS
    assert any(p.endswith("lfg_chaintext.hip") for p in _native.SOURCES)
    assert ("#define LFG_CHAIN_TEXT_MAX_NDIM %d" % _native.CHAIN_TEXT_MAX_NDIM) in open(path).read()


def test_python_rows_is_the_documented_last_resort():
    chain, lnp = ct.block_case(2, 3, 4)
    assert chaintext.python_rows(chain, lnp, 5) == ct.rows(chain, lnp, 5)
    z = np.zeros((2, 3, 0))
    assert chaintext.format_rows(z, lnp[:, :3]) == ct.rows(z, lnp[:, :3])   # (a row length the ABI refuses)


def test_write_chain_file_bytes_on_a_host_chain(port, tmp_path, monkeypatch):
    """-inf and nan ln_probs; arrays, host tensors and a strided view; with
    the twin and with the last resort the file is the oracle's"""
    import torch
    chain, lnp = ct.block_case(5, 6, 18, seed=2)
    lnp = lnp.copy()
    lnp[0, 0], lnp[1, 2], lnp[4, 5], lnp[2, 1] = -np.inf, np.nan, np.inf, 2.0 ** 70
    names = ["p%d" % i for i in range(18)]
    want = ("walker_no " + " ".join(names) + " ln_prob\n").encode() + ct.rows(chain, lnp)
    monkeypatch.setattr(chaintext, "_twin", None)   # the library the fixture built
    monkeypatch.setattr(chaintext, "TWIN_PATH", port.lib._name)
    f = str(tmp_path / "chain.txt")
    for c, l in ((chain, lnp), (torch.as_tensor(chain.copy()), torch.as_tensor(lnp)), (chain.tolist(), lnp.tolist())):
        sampler.write_chain(f, names, c, l)
        assert chaintext.twin() is not None
        assert open(f, "rb").read() == want
    sampler.write_chain(f, names, chain[:2], lnp[:2])
    sampler.write_chain(f, None, chain[2:], lnp[2:], mode="a")
    assert open(f, "rb").read() == want
    wide = np.zeros((5, 3, 6, 18))
    wide[:, 1] = chain
    lw = np.zeros((5, 3, 6))
    lw[:, 1] = lnp
    sampler.write_chain(f, names, torch.as_tensor(wide)[:, 1], torch.as_tensor(lw)[:, 1])
    assert open(f, "rb").read() == want
    monkeypatch.setattr(chaintext, "_twin", False)   # no twin: the Python expression
    sampler.write_chain(f, names, chain, lnp)
    assert open(f, "rb").read() == want
