"""The test double of chain_prod.txt's rows (MODEL_SPEC.md section 17): Python
itself.  rows() is the expression sampler.write_chain used to loop over, and
every comparison against it is byte equality; the value lists below are what
the host twin (tests/test_chaintext_cpu.py, tests/test_chaintext_host.py) and
the device (tests/test_gpu_chaintext.py) are held to.
"""
import functools
import struct

import numpy as np

H = float.fromhex
INF, NAN = float("inf"), float("nan")
NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xfff8000000000000))[0]
TWO63 = 2.0 ** 63


def rows(chain, lnprob, walker0=0):
    """the oracle: bytes of the rows of chain [steps, W, ndim], lnprob [steps, W]"""
    chain, lnprob = np.asarray(chain, dtype=np.float64), np.asarray(lnprob, dtype=np.float64)
    out = []
    for s in range(chain.shape[0]):
        for k in range(chain.shape[1]):
            out.append("{0:4d} {1:s} {2:f}\n".format(walker0 + k, " ".join(map(repr, map(float, chain[s, k]))),
                                                     float(lnprob[s, k])))
    return "".join(out).encode()


def around(x):
    """x and both neighbours"""
    return [float(np.nextafter(x, -INF)), float(x), float(np.nextafter(x, INF))]


def both(v):
    return list(v) + [-x for x in v]


@functools.lru_cache(None)
def hard():
    """the hard doubles of repr"""
    v = [0.0, H("0x0.0000000000001p-1022"), H("0x0.fffffffffffffp-1022"), H("0x1p-1022"),
         H("0x1.fffffffffffffp+1023"),
         H("0x1.0f0cf064dd592p+73"),   # 1e22
         H("0x1.52d02c7e14af6p+76"),   # 1e23 (whose shortest digits are 1e+23)
         H("0x1.0000000000000p+53"),   # 9007199254740993.0 reads as 2^53
         H("0x1.1c37937e07fffp+53"),   # 9999999999999998.0
         H("0x1.e000000000000p+6"),    # 120.0
         H("0x1.a36e2eb1c432dp-14"),   # 0.0001
         H("0x1.4f8b588e368f1p-17"),   # 1e-05
         H("0x1.421f5f40d8376p-23"),   # 1.5e-07
         H("0x1.c6bf52634p+49"),       # 1000000000000000.0
         H("0x1.1c37937e08p+53"),      # 1e+16
         9007199254740993.0, 9999999999999998.0, 120.0, 1e16, 1e15, 1e-4, 1e-5, 1.5e-7, 5e-324,
         1.7976931348623157e308]
    for k in list(range(-1074, 1024, 41)) + [-1022, -1021, -1, 0, 1, 52, 53, 54, 62, 63, 64, 1023]:
        x = 2.0 ** k if k > -1075 else 0.0
        v += [y for y in around(x) if np.isfinite(y)]
    for k in range(-5, 24):
        v += around(float("1e%d" % k))
    digits = "12345678901234567"
    for n in range(1, 18):
        v += [float(digits[0] + "." + digits[1:n] + "e%d" % e if n > 1 else digits[0] + "e%d" % e)
              for e in (-7, -5, -4, 0, 3, 15, 16, 17, 21, 100, -100)]
    return tuple(both(v) + [INF, -INF, NAN, NEG_NAN])


@functools.lru_cache(None)
def fixed():
    """the hard doubles of '{:f}' below 2^63, and the non-finite ones"""
    v = [0.0, 0.0000005, 1.0000005, 1e-300, 5e-324, 4.9999e-7, 5.000001e-7, 0.9999995, 9.9999995, 99.9999995,
         999999.9999995, 0.9999994999999999, 0.99999949, 0.99999951, 0.5, 1.5, 2.5, 1e-6, 1e-7, 123456.789,
         H("0x1.fffffffffffffp+62"), H("0x1.ffffffffffffep+62"), H("0x1p+62"), 2.0 ** 53, 2.0 ** 53 - 1.0,
         2.0 ** 52 - 0.5, 2.0 ** 52 + 0.5, 2.0 ** 51 + 0.25, 2.0 ** 51 - 0.25, 2.0 ** 33 + 2.0 ** -19, 2.0 ** -10,
         2.0 ** -11, 2.0 ** -20, 2.0 ** -21, 2.0 ** -22, 3 * 2.0 ** -21, 2.0 ** -74, 2.0 ** -75, 2.0 ** -64,
         2.0 ** -63, 2.0 ** -65]
    # exact ties at the sixth decimal: j / 2^7 has seven decimals, the last a 5
    # for odd j; both parities of the sixth digit occur, and offsets keep the tie
    for j in range(1, 512, 2):
        v += [j / 128.0, 1000.0 + j / 128.0, 2.0 ** 40 + j / 128.0]
    v += [j / 128.0 for j in range(0, 256, 2)]   # (and their neighbours that are no ties)
    # ties of fewer binary digits, carries into the integer part
    v += [0.5 ** 7, 3 * 0.5 ** 7, 1 - 0.5 ** 7, 7.0 - 0.5 ** 7, 9.0 + 127.0 / 128.0]
    for x in (0.9999995, 9.9999995, 1.0000005, 0.0000005, 0.0078125, 0.0234375):
        v += around(x)
    return tuple(both(v) + [INF, -INF, NAN, NEG_NAN])


def refused():
    """finite doubles of 2^63 and beyond: '{:f}' the device leaves to the host"""
    return tuple(both([TWO63, float(np.nextafter(TWO63, INF)), 1e19, 1e22, 1e300, H("0x1.fffffffffffffp+1023")]))


@functools.lru_cache(None)
def random_bits(n=200704):
    return np.random.default_rng(20261).integers(0, 2 ** 64, size=n, dtype=np.uint64).view(np.float64)


@functools.lru_cache(None)
def log_uniform(n=200704):
    rng = np.random.default_rng(20262)
    return 10.0 ** rng.uniform(-6.0, 6.0, size=n) * rng.choice([-1.0, 1.0], size=n)


@functools.lru_cache(None)
def short_decimals(n=20480):
    rng = np.random.default_rng(20263)
    x = np.concatenate([np.round(rng.uniform(-1000.0, 1000.0, size=n // 4), d) for d in (1, 2, 3, 6)])
    i = rng.integers(-10 ** 9, 10 ** 9, size=n // 2).astype(np.float64)
    big = rng.integers(0, 2 ** 62, size=n // 4).astype(np.float64)
    return np.concatenate([x, i, big, big * 1e4])


def device_ok(v):
    """v with the values the device refuses as ln_prob replaced by 0.5"""
    v = np.array(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        v[np.isfinite(v) & (np.abs(v) >= TWO63)] = 0.5
    return v


LISTS = {"hard": lambda: np.array(hard()), "fixed": lambda: np.array(fixed()), "random_bits": random_bits,
         "log_uniform": log_uniform, "short_decimals": short_decimals}


@functools.lru_cache(None)
def column_case(name, device):
    """(chain [n, 1, 1], lnprob [n, 1], the oracle's bytes) of a value list:
    every value as a chain value and as a ln_prob (device: as device_ok)"""
    v = np.ascontiguousarray(LISTS[name]())
    lnp = device_ok(v) if device else v.copy()
    chain = v.reshape(-1, 1, 1)
    lnp = lnp.reshape(-1, 1)
    want = rows(chain, lnp)
    return chain, lnp, want


@functools.lru_cache(None)
def block_case(steps, W, ndim, seed=0):
    """a chain of mixed values (chain [steps, W, ndim], lnprob [steps, W]):
    random patterns, walks around one, short decimals and the hard lists"""
    rng = np.random.default_rng(1000 + seed)
    n = steps * W * ndim
    pool = np.concatenate([random_bits()[:4096], 1.0 + 1e-3 * rng.standard_normal(4096), short_decimals()[:4096],
                           np.array(hard())])
    chain = pool[rng.integers(0, pool.size, size=n)].reshape(steps, W, ndim)
    lpool = np.concatenate([-1e4 * rng.random(4096), np.array(fixed()), device_ok(random_bits()[:1024])])
    lnp = lpool[rng.integers(0, lpool.size, size=steps * W)].reshape(steps, W)
    return chain, lnp


def first_difference(got, want):
    """a readable account of where two byte strings part"""
    if got == want:
        return None
    n = min(len(got), len(want))
    i = next((j for j in range(n) if got[j] != want[j]), n)
    a = want.rfind(b"\n", 0, i) + 1
    return "lengths %d / %d, first difference at byte %d: got %r, want %r" % (
        len(got), len(want), i, got[a:i + 40], want[a:i + 40])
