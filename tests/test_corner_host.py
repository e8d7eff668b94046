"""CPU: the corner-plot data's host twin (cpu_baseline/lfg_cpu_corner.cpp:
lfg_corner.hpp compiled for the host) as a stand-alone program under the
host's address and undefined-behaviour sanitizers.

tests/corner_host_main.cpp keeps every input in a heap block of exactly its
size (the strided views of tests/chain_double.py's layouts: the last element
read is the block's last, or lies before a NaN pad that must not be read) and
every output between guard bands.  It is built -O1 -g -fsanitize=address,
undefined -fno-sanitize-recover=all and run as that program: no sanitizer is
applied to code loaded into Python.  Its counts equal the numpy double's
(tests/corner_double.py).
"""
import os
import subprocess

import numpy as np

from tests import chain_double as cd
from tests import corner_double as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def cases():
    """every size and every layout of the sizes-by-layouts block once, and
    every K / nb / range case of the list"""
    block = [c for c in co.CASES if c[2:] == (10, 3, 50, "default")]
    rest = [c for c in co.CASES if c not in block]
    return [c for c in block if (co.SIZES.index(c[0]) + co.LAYOUTS.index(c[1])) % 4 == 0] + rest


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    todo = cases()
    assert len(todo) >= 20 and {c[1] for c in todo} == set(co.LAYOUTS) and {c[0] for c in todo} == set(co.SIZES)
    nl = len(co.FRACS)
    with open(src, "wb") as fh:
        fh.write(np.int32(len(todo) + 1).tobytes())
        for c in todo:
            size, kind, C, K, nb, mode = c
            x, cols, rng, _ = co.case(*c)
            buf, off, sld, wld = cd.layout(x, kind)
            steps, W = size
            # the block ends with the last element read: the largest chosen column of the last row
            buf = buf[: off + (steps - 1) * sld + (W - 1) * wld + max(cols) + 1]
            fh.write(np.array([steps, W, C, sld, wld, off, buf.size, K, nb, nl], dtype=np.int64).tobytes())
            fh.write(np.ascontiguousarray(buf, dtype=np.float64).tobytes())
            fh.write(np.array(cols, dtype=np.int32).tobytes())
            fh.write(np.ascontiguousarray(rng, dtype=np.float64).tobytes())
            fh.write(np.array(co.FRACS, dtype=np.float64).tobytes())
        # no rows at all: zeros and the flags
        fh.write(np.array([0, 3, 4, 12, 4, 0, 0, 2, 5, nl], dtype=np.int64).tobytes())
        fh.write(np.array([3, 1], dtype=np.int32).tobytes())
        fh.write(np.array([0.0, 1.0, 2.0, 2.0], dtype=np.float64).tobytes())
        fh.write(np.array(co.FRACS, dtype=np.float64).tobytes())
    exe = str(tmp_path / "corner_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "corner_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_corner.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0

    def take(dtype, *shape):
        nonlocal pos
        a = np.frombuffer(data, dtype, int(np.prod(shape, dtype=np.int64)), pos).reshape(shape)
        pos += a.nbytes
        return a
    for c in todo:
        K, nb = c[3], c[4]
        P = K * (K - 1) // 2
        assert tuple(take(np.int32, 2)) == (0, 0)
        got = {"h1": take(np.int64, K, nb), "h2": take(np.int64, P, nb, nb), "levels": take(np.int64, P, nl),
               "flag": take(np.int32, K)}
        co.check(got, co.case(*c)[3], c)
    assert tuple(take(np.int32, 2)) == (0, 0)
    assert not take(np.int64, 2, 5).any() and not take(np.int64, 1, 5, 5).any() and not take(np.int64, 1, nl).any()
    assert list(take(np.int32, 2)) == [0, 1]
    assert pos == len(data)
