"""CPU: the chain-parse host twin (cpu_baseline/lfg_cpu_chainparse.cpp:
lfg_chainparse.hpp compiled for the host) as a stand-alone program under the
host's address and undefined-behaviour sanitizers.

tests/chainparse_host_main.cpp keeps the text in a heap block of exactly its
size, so that a read past its last byte is caught (the parser looks one byte
ahead for '\\r\\n' and walks tokens that end with the text), ws in a block of
exactly the size function's value, and the output between guard bands; doubles
beyond rows * ncol must stay untouched.  It is built -O1 -g
-fsanitize=address,undefined -fno-sanitize-recover=all and run as that
program: no sanitizer is applied to code loaded into Python.  Its doubles are
float()'s (tests/chainparse_cases.py).
"""
import os
import subprocess

import numpy as np

from tests import chainparse_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TILE = 8192   # (only sizes the texts here; the other tests ask the library)


def cases():
    """(header, text, rc of count, rc of parse, expected info or None, expected values or None)"""
    out = []

    def add(text, ncol, want=None, info=None, extra=1, ws_short=0, rc1=0, rc2=0):
        h = np.array([len(text), ncol, extra, ws_short], np.int64)
        if want is not None:
            info = [want.shape[0], want.size, 0, 0, 0, -1, 0, 0]
        out.append((h, text, rc1, rc2, info, want))

    for name in ("digits17_19", "ties", "edges", "long"):
        text, want, _ = cc.list_case(name)
        add(text, 1, want)
    text, want, _ = cc.list_case("roundtrip")
    cut = text.index(b"\n", 400000) + 1
    add(text[:cut], 1, want[:text[:cut].count(b"\n")])
    for name, text, ncol, want in cc.structure_cases(TILE):
        if ncol is not None:
            add(text, ncol, want)
    for shift in (0, 1, 15, 16, 17, cc.MAX_TOKEN, cc.MAX_TOKEN + 1):
        text, want = cc.shifted(TILE, shift)
        add(text, 2, want)
        add(text[:-1], 2, want)               # the text ends with its last token
    for name, text, ncol, row in cc.ragged_cases():
        add(text, ncol, info=[None, None, 0, 0, "nonzero", row, 0, 0])
    for tok, text, row in cc.bad_files():
        add(text, 3, info=[5, 15, 1, 0, 0, row, 0, 0])
        add(text[:-1], 3, info=[5, 15, 1, 0, 0, row, 0, 0])
    # refusals: nothing written
    text, want = cc.table(["1", "2", "3", "4"], 2)
    add(text, 0, rc1=-1)
    add(text, cc.MAX_NCOL + 1, rc1=-1)
    add(text, 2, ws_short=1, rc1=-1)
    add(text, 2, info=[2, 4, 0, 0, 0, -1, 1, 0], extra=-1)   # a capacity below the rows: found, nothing written
    return out


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    todo = cases()
    with open(src, "wb") as fh:
        fh.write(np.int32(len(todo)).tobytes())
        for h, text, _, _, _, _ in todo:
            fh.write(h.tobytes())
            fh.write(text)
    exe = str(tmp_path / "chainparse_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "chainparse_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_chainparse.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0
    for i, (h, text, rc1, rc2, info, want) in enumerate(todo):
        got1, got2 = (int(v) for v in np.frombuffer(data, np.int32, 2, pos))
        got = [int(v) for v in np.frombuffer(data, np.int64, 8, pos + 8)]
        pos += 72
        assert got1 == rc1, (i, h)
        if rc1 != 0:
            assert got2 == -99 and got == [-7] * 8   # nothing written
            continue
        assert got2 == rc2, (i, h)
        for g, w in zip(got, info):
            assert w is None or (g != 0 if w == "nonzero" else g == w), (i, h, got, info)
        if got[4] == 0 and got[6] == 0:
            n = got[0] * int(h[1])
            vals = np.frombuffer(data, np.float64, n, pos)
            pos += 8 * n
            if want is not None:
                bad = cc.same(vals, want)
                assert bad.size == 0, (i, h, bad[:5])
    assert pos == len(data)
