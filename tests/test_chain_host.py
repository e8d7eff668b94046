"""CPU: the chain summary's host twin (cpu_baseline/lfg_cpu_chain.cpp:
lfg_chain.hpp compiled for the host) as a stand-alone program under the host's
address and undefined-behaviour sanitizers.

tests/chain_host_main.cpp keeps every input in a heap block of exactly its
size (the strided views of tests/chain_double.py's layouts: the last element
read is the block's last, or lies before a NaN pad that must not be read) and
every output between guard bands.  It is built -O1 -g -fsanitize=address,
undefined -fno-sanitize-recover=all and run as that program: no sanitizer is
applied to code loaded into Python.  Its results meet the numpy double as in
tests/test_chainstats_cpu.py.
"""
import os
import subprocess

import numpy as np

from tests import chain_double as cd
from tests.test_chainstats_cpu import rhat_chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def cases():
    """(x, layout kind, window, fracs, rhat, clip)"""
    out = []
    for size, kind in zip(cd.SIZES, ("chain_dev", "walker_major", "padded", "skipthin", "skipthin", "walker_major")):
        out.append((cd.shared(size[0], size[1], 7)[0], kind, None, cd.FRACS, False, False))
    x = cd.shared(37, 6, 7)[0]
    out.append((x, "padded", np.tile([-0.5, 1.5], (7, 1)), (0.5, 0.0, 1.0), False, True))
    out.append((x, "chain_dev", np.tile([1e301, 1e302], (7, 1)), cd.FRACS, False, True))
    out.append((cd.skewed().reshape(-1, 1, 1), "chain_dev", None, (0.5,), False, True))
    out.append((cd.shared(37, 6, 18)[0], "skipthin", None, (), False, False))
    mixed, offset = rhat_chains()
    out.append((mixed, "chain_dev", None, (), True, False))
    out.append((offset, "walker_major", None, cd.FRACS, True, False))
    out.append((np.empty((0, 3, 2)), "chain_dev", None, cd.FRACS, True, False))
    return out


def test_twin_under_sanitizers_on_guarded_buffers(tmp_path):
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    todo = cases()
    with open(src, "wb") as fh:
        fh.write(np.int32(len(todo)).tobytes())
        for x, kind, window, fracs, rhat, clip in todo:
            buf, off, sld, wld = cd.layout(x, kind)
            steps, W, C = x.shape
            if kind != "padded" and steps and W:   # the block ends with the last element read
                buf = buf[: off + (steps - 1) * sld + (W - 1) * wld + C]
            fh.write(np.array([steps, W, C, sld, wld, off, buf.size, window is not None, len(fracs), rhat, clip],
                              dtype=np.int64).tobytes())
            fh.write(np.ascontiguousarray(buf, dtype=np.float64).tobytes())
            if window is not None:
                fh.write(np.ascontiguousarray(window, dtype=np.float64).tobytes())
            fh.write(np.array(fracs, dtype=np.float64).tobytes())
    exe = str(tmp_path / "chain_host")
    subprocess.run(["g++", "-std=c++17", "-fopenmp", "-march=x86-64-v3", "-Wno-unknown-pragmas"] + SAN +
                   ["-I", os.path.join(ROOT, "cpu_baseline"), "-I", os.path.join(ROOT, "cpu_baseline", "shim"),
                    "-I", os.path.join(ROOT, "lfit_python_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "chain_host_main.cpp"),
                    os.path.join(ROOT, "cpu_baseline", "lfg_cpu_chain.cpp")], check=True)
    r = subprocess.run([exe, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    data = open(dst, "rb").read()
    pos = 0

    def take(dtype, *shape):
        nonlocal pos
        a = np.frombuffer(data, dtype, int(np.prod(shape, dtype=np.int64)), pos).reshape(shape)
        pos += a.nbytes
        return a
    for x, kind, window, fracs, rhat, clip in todo:
        C, nq = x.shape[2], len(fracs)
        assert int(take(np.int32, 1)[0]) == 0
        got = {"n": take(np.int64, C), "n_bad": take(np.int64, C)}
        for k in ("mean", "m2", "min", "max"):
            got[k] = take(np.float64, C)
        got["ostat"], got["quant"] = take(np.float64, C, nq, 2), take(np.float64, C, nq)
        if rhat:
            got["rhat"] = take(np.float64, C)
        want = cd.expected(x, window, fracs, rhat) if x.size else None
        if want is None:
            assert np.all(got["n"] == 0) and np.all(np.isnan(got["quant"])) and np.all(np.isnan(got["rhat"]))
        else:
            cd.check(got, want, (kind, x.shape), rhat)
        if clip:
            nxt = take(np.float64, C, 2)
            win = np.tile([-np.inf, np.inf], (C, 1)) if window is None else np.asarray(window, dtype=np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                sd = np.sqrt(got["m2"] / got["n"])
            ok = (got["n"] > 0) & np.isfinite(sd)
            lo = np.where(ok, np.maximum(win[:, 0], got["quant"][:, 0] - 3.0 * sd), win[:, 0])
            hi = np.where(ok, np.minimum(win[:, 1], got["quant"][:, 0] + 3.0 * sd), win[:, 1])
            assert np.array_equal(nxt[:, 0], lo) and np.array_equal(nxt[:, 1], hi)
    assert pos == len(data)
