"""CPU: lfg_cpu_physpar (cpu_baseline/lfg_cpu_physpar.cpp: lfg_physpar.hpp and
lfg_device.hpp compiled for the host) as a stand-alone program under the
host's address and undefined-behaviour sanitizers.

tests/physpar_host_main.cpp reads the packed tables and 257 rows of the fixed
batch from a file, keeps every table and buffer in a heap block of exactly its
size, the outputs between guard bands, and calls the twin for n of 0, 1, 65
and 257 on a strided chain (ld = 5).  It is built -O1 -g -fsanitize=address,
undefined -fno-sanitize-recover=all and run as that program: no sanitizer is
applied to code loaded into Python.  A finding in the shared headers is a
finding about the device code.  Its results meet the tight double within
tests/test_physpar_cpu.py's tolerances.
"""
import os
import subprocess

import numpy as np

from tests import physpar_double as ppd
from tests.test_physpar_cpu import INCL_ATOL, RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COUNTS = (0, 1, 65, 257)
LD = 5


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    from lfit_python_amd import physpar
    tables = physpar.load_mr_tables(ppd.WD_MODELS)
    b, ref = ppd.shared(True)
    # the batch's special rows (status, gate, clamp, bracket ends) and base rows up to 257
    n_all = len(b["q"])
    rows = np.concatenate([np.arange(b["n_base"], n_all), np.arange(257 - (n_all - b["n_base"]))])
    rows = rows[np.random.default_rng(3).permutation(257)]
    assert len(rows) == 257 and set(np.unique(ref["status"][rows])) == {0, 1, 2, 5, 6}
    assert set(np.unique(ref["model"][rows])) == {-1, 0, 1, 2}
    chain = np.full((257, LD), 7.0)
    chain[:, 0], chain[:, 1], chain[:, 2] = b["q"][rows], b["dphi"][rows], b["rw"][rows]
    A = tables.arrays
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([A["wood_t"].size, A["ham_m"].size, A["pan_tx"].size, A["pan_ty"].size, 257, LD],
                          dtype=np.int32).tobytes())
        fh.write(tables.wood_off.astype(np.int32).tobytes())
        for name in ("wood_t", "wood_r", "wood_card", "ham_m", "ham_r", "pan_tx", "pan_ty", "pan_c"):
            fh.write(A[name].astype(np.float64).tobytes())
        fh.write(np.array([tables.constants[k] for k in ("G", "GMsun", "Rsun", "day")]).tobytes())
        fh.write(chain.tobytes())
        fh.write(b["T"][rows].tobytes())
        fh.write(b["P"][rows].tobytes())
    exe = str(tmp_path / "physpar_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "physpar_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_physpar.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0
    for n in COUNTS:
        rc = int(np.frombuffer(data, np.int32, 1, pos)[0])
        pos += 4
        out = np.frombuffer(data, np.float64, 10 * n, pos).reshape(10, n).T
        pos += 80 * n
        model = np.frombuffer(data, np.int32, n, pos)
        pos += 4 * n
        status = np.frombuffer(data, np.int32, n, pos)
        pos += 4 * n
        assert rc == 0
        k = rows[:n]
        assert np.array_equal(status, ref["status"][k]) and np.array_equal(model, ref["model"][k]), n
        ok = status == 0
        assert np.all(np.isnan(out[~ok]))
        if ok.any():
            a, w = out[ok], ref["table"][k][ok]
            assert np.max(np.abs(a[:, :9] - w[:, :9]) / np.abs(w[:, :9])) <= RTOL, n
            assert np.max(np.abs(a[:, 9] - w[:, 9])) <= INCL_ATOL, n
    assert pos == len(data)
