"""CPU: lfg_cpu_limbdark (cpu_baseline/lfg_cpu_limbdark.cpp: lfg_limbdark.hpp
and lfg_physpar.hpp's spline evaluation compiled for the host) as a
stand-alone program under the host's address and undefined-behaviour
sanitizers.

tests/ld_host_main.cpp reads the packed tables and 257 rows from a file, keeps
every table and buffer in a heap block of exactly its size, the outputs
between guard bands, and calls the twin for n of 0, 1, 65 and 257 on a strided
chain (ld = 5) whose rows include all three statuses.  It is built -O1 -g
-fsanitize=address,undefined -fno-sanitize-recover=all and run as that
program: no sanitizer is applied to code loaded into Python.  A finding in the
shared headers is a finding about the device code.  Its results meet the
reference's values (tests/golden/limbdark_ref.npz) within 64 eps c_max.
"""
import os
import subprocess

import numpy as np

from tests import ld_double as ldd

ROOT = ldd.ROOT
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COUNTS = (0, 1, 65, 257)
LD = 5


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    tables = ldd.tables()
    logg, teff, idx = ldd.mixed_rows(257)
    assert set(ldd.expected_status(logg, teff)) == {ldd.ST_OK, ldd.ST_BAD_ARGS, ldd.ST_CLAMPED}
    assert set(ldd.expected_status(logg[:65], teff[:65])) == {ldd.ST_OK, ldd.ST_BAD_ARGS, ldd.ST_CLAMPED}
    chain = np.full((257, LD), 7.0)
    chain[:, 0], chain[:, 1] = teff, logg
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([tables.tx.size, tables.ty.size, 257, LD], dtype=np.int32).tobytes())
        for a in (tables.tx, tables.ty, tables.c, chain):
            fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    exe = str(tmp_path / "ld_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "ld_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_limbdark.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0
    for n in COUNTS:
        rc = int(np.frombuffer(data, np.int32, 1, pos)[0])
        pos += 4
        out = np.frombuffer(data, np.float64, 25 * n, pos).reshape(n, 25)
        pos += 200 * n
        status = np.frombuffer(data, np.int32, n, pos)
        pos += 4 * n
        assert rc == 0
        ldd.check_rows(out, status, logg[:n], teff[:n], idx[:n], "sanitized twin, n = %d" % n)
    assert pos == len(data)
