"""CPU: lfg_cpu_wd_lnprob (cpu_baseline/lfg_cpu_wd.cpp: lfg_wd.hpp and
lfg_device.hpp compiled for the host) as a stand-alone program under the
host's address and undefined-behaviour sanitizers.

tests/wd_host_main.cpp reads the packed model (g and r colour-corrected) and
257 rows of the fixed batch from a file, keeps every table and buffer in a
heap block of exactly its size, the outputs between guard bands, and calls
the twin for n of 0, 1, 65 and 257 on a strided chain (ld = 6).  It is built
-O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all and run as that
program: no sanitizer is applied to code loaded into Python.  A finding in the
shared headers is a finding about the device code.  Its results meet the
double within tests/wd_double.py's bounds.
"""
import os
import subprocess

import numpy as np

from tests import wd_double as wdd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COUNTS = (0, 1, 65, 257)
LD = 6


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    b, _ = wdd.shared("A", True)
    M = wdd.build_model("A", True)
    n_all = len(b["theta"])
    rows = np.arange(257) % n_all
    rows = rows[np.random.default_rng(5).permutation(257)]
    assert set(rows) == set(range(n_all))    # every row of the batch, the special ones included
    theta = b["theta"][rows]
    D = wdd.Double("A", True)
    chain = np.full((257, LD), 7.0)
    chain[:, :4] = theta
    A, S = M.arrays, M.host_struct()
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([M.B, A["tx"].size, A["ty"].size, 257, LD], dtype=np.int32).tobytes())
        fh.write(np.array(list(S.cnx), dtype=np.int32).tobytes())
        fh.write(np.array(list(S.cny), dtype=np.int32).tobytes())
        fh.write(np.array(list(S.prior_type), dtype=np.int32).tobytes())
        for name in ("tx", "ty", "c"):
            fh.write(A[name].astype(np.float64).tobytes())
        for k in range(M.B):
            if S.cnx[k]:
                for name in ("ctx%d", "cty%d", "cc%d"):
                    fh.write(A[name % k].astype(np.float64).tobytes())
        fh.write(np.array(list(S.k) + list(S.mag) + list(S.err) + [S.lnnorm] + list(S.prior_p1) + list(S.prior_p2) +
                          list(S.prior_c0) + list(S.prior_c1)).tobytes())
        fh.write(chain.tobytes())
    assert sum(1 for k in range(M.B) if S.cnx[k]) == 2
    exe = str(tmp_path / "wd_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "wd_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_wd.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0
    for n in COUNTS:
        rc = int(np.frombuffer(data, np.int32, 1, pos)[0])
        pos += 4
        lnp = np.frombuffer(data, np.float64, n, pos)
        pos += 8 * n
        ll = np.frombuffer(data, np.float64, n, pos)
        pos += 8 * n
        mags = np.frombuffer(data, np.float64, M.B * n, pos).reshape(M.B, n).T
        pos += 8 * M.B * n
        status = np.frombuffer(data, np.int32, n, pos)
        pos += 4 * n
        assert rc == 0
        if n:
            wdd.check_against(lnp, mags, ll, status, D.run(theta[:n]), "n = %d" % n)
    assert pos == len(data)
