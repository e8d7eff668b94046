"""CPU: the chain-text host twin (cpu_baseline/lfg_cpu_chaintext.cpp:
lfg_chaintext.hpp compiled for the host) as a stand-alone program under the
host's address and undefined-behaviour sanitizers.

tests/chaintext_host_main.cpp keeps the chain and ln_prob in heap blocks of
exactly their size (strided views included: the last element read is the
block's last) and the output between guard bands; bytes beyond the total must
stay untouched.  It is built -O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=all and run as that program: no sanitizer is applied to
code loaded into Python.  Its bytes equal Python's (tests/chaintext_double.py).
"""
import os
import subprocess

import numpy as np

from tests import chaintext_double as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def row_bound(ndim, walker_max):
    return max(4, len(str(walker_max))) + 25 * ndim + 29


def cases():
    """(header, chain block, ln_prob block, expected rc, expected bytes)"""
    out = []

    def add(buf, lbuf, steps, W, ndim, sld, wld, off, lsld, lwld, loff, walker0, want, cap=None, rc=0):
        # the blocks end with the last element read
        if steps and W:
            buf = buf[: off + (steps - 1) * sld + (W - 1) * wld + ndim]
            lbuf = lbuf[: loff + (steps - 1) * lsld + (W - 1) * lwld + 1]
        if cap is None:
            cap = steps * W * row_bound(ndim, walker0 + max(W, 1) - 1)
        h = np.array([steps, W, ndim, sld, wld, off, buf.size, lsld, lwld, loff, lbuf.size, walker0, cap], np.int64)
        out.append((h, np.ascontiguousarray(buf), np.ascontiguousarray(lbuf), rc, want))

    for name in ("hard", "fixed"):   # every hard value as a chain value and as a ln_prob
        chain, lnp, want = ct.column_case(name, False)
        n = chain.shape[0]
        big = int(np.count_nonzero(np.isfinite(lnp) & (np.abs(lnp) >= ct.TWO63)))
        add(chain.reshape(-1), lnp.reshape(-1), n, 1, 1, 1, 1, 0, 1, 1, 0, 0, want, cap=n * row_bound(1, 0) + 320 * big)
    v = ct.random_bits()[:4000]
    add(v, v, 4000, 1, 1, 1, 1, 0, 1, 1, 0, 0, ct.rows(v.reshape(-1, 1, 1), v.reshape(-1, 1)),
        cap=4000 * row_bound(1, 0) + 320 * 4000)
    for (steps, W, ndim), w0 in (((3, 5, 1), 0), ((2, 7, 18), 9995), ((1, 3, 87), 99998), ((0, 4, 3), 0), ((3, 0, 3), 7)):
        chain, lnp = ct.block_case(steps, W, ndim)
        add(chain.reshape(-1), lnp.reshape(-1), steps, W, ndim, max(1, W * ndim), ndim, 0, max(1, W), 1, 0, w0,
            ct.rows(chain, lnp, w0))
    # the cold level of a tempered chain [6][T = 4][W = 5], level 3: the last element is the buffer's last
    chain, lnp = ct.block_case(6, 20, 3, seed=1)
    c4, l4 = chain.reshape(6, 4, 5, 3), lnp.reshape(6, 4, 5)
    add(chain.reshape(-1), lnp.reshape(-1), 6, 5, 3, 60, 3, 45, 20, 1, 15, 0, ct.rows(c4[:, 3], l4[:, 3]))
    # thinned by 3 from step 2: steps 2 and 5
    add(chain.reshape(-1), lnp.reshape(-1), 2, 20, 3, 180, 3, 120, 60, 1, 40, 0, ct.rows(chain[2::3], lnp[2::3]))
    # refusals: nothing written
    add(chain.reshape(-1), lnp.reshape(-1), 6, 20, 3, 60, 3, 0, 20, 1, 0, 0, b"", cap=100, rc=-1)
    add(chain.reshape(-1), lnp.reshape(-1), 6, 20, 3, 0, 3, 0, 20, 1, 0, 0, b"", rc=-1)
    return out


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    todo = cases()
    with open(src, "wb") as fh:
        fh.write(np.int32(len(todo)).tobytes())
        for h, buf, lbuf, _, _ in todo:
            fh.write(h.tobytes())
            fh.write(buf.astype(np.float64).tobytes())
            fh.write(lbuf.astype(np.float64).tobytes())
    exe = str(tmp_path / "chaintext_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "chaintext_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_chaintext.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0
    for i, (h, _, _, rc, want) in enumerate(todo):
        got_rc = int(np.frombuffer(data, np.int32, 1, pos)[0])
        nb = np.frombuffer(data, np.int64, 2, pos + 4)
        pos += 20
        assert got_rc == rc, (i, h)
        if rc != 0:
            assert list(nb) == [-7, -7]   # nothing written
            continue
        assert list(nb) == [len(want), 0], (i, h)
        got = data[pos:pos + len(want)]
        pos += len(want)
        assert got == want, (i, ct.first_difference(got, want))
    assert pos == len(data)
