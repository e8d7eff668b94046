"""The token lists and text builders of the chain parser's tests (MODEL_SPEC.md
section 18).  Python's float() is the oracle: it is correctly rounded and
shares no code with lfg_chainparse.hpp.  Every comparison is equality of the 8
bytes of float(token), NaN against NaN (same()).

The host twin (tests/test_chainparse_cpu.py, tests/test_chainparse_host.py)
must get every token right; the device (tests/test_gpu_chainparse.py) may
refuse exactly what may_refuse() says, from the rule of include/lfg_chainparse.h
alone: a token of more than MAX_TOKEN bytes, or a mantissa of more than 19
significant digits.
"""
import functools
import random
import re
import struct

import numpy as np

from tests import chaintext_double as ct

MAX_TOKEN = 64      # LFG_CHAIN_PARSE_MAX_TOKEN
MAX_NCOL = 1025     # LFG_CHAIN_PARSE_MAX_NCOL


def expected(tokens):
    """float64 array of float(token)"""
    return np.array([float(t) for t in tokens], dtype=np.float64)


def same(got, want):
    """indices at which two float64 arrays differ: other bits, NaN against NaN allowed"""
    got, want = np.ascontiguousarray(got, np.float64).reshape(-1), np.ascontiguousarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    eq = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    return np.flatnonzero(~eq)


def significant_digits(token):
    """digits from the first non-zero to the last non-zero one of the mantissa, across the point"""
    m = re.split("[eE]", token.lstrip("+-"))[0].replace(".", "")
    return len(m.strip("0"))


def may_refuse(token):
    """the rule of include/lfg_chainparse.h: what the device is allowed to refuse"""
    if token.lstrip("+-").lower() in ("inf", "infinity", "nan"):
        return len(token) > MAX_TOKEN
    return len(token) > MAX_TOKEN or significant_digits(token) > 19


def table(tokens, ncol=1, sep=" ", eol="\n", lead="", trail="", final=True):
    """(text, expected [rows][ncol]) of the tokens laid out ncol to a row;
    the last row is filled up with '1'"""
    tokens = list(tokens)
    tokens += ["1"] * (-len(tokens) % ncol)
    rows = [lead + sep.join(tokens[i:i + ncol]) + trail for i in range(0, len(tokens), ncol)]
    text = eol.join(rows) + (eol if final else "")
    return text.encode("latin-1"), expected(tokens).reshape(-1, ncol)


# ---- the token lists ---------------------------------------------------------------------------
@functools.lru_cache(None)
def roundtrip():
    v = ct.random_bits(400000)
    out = [repr(float(x)) for x in v]
    for name in ("hard", "fixed"):
        vals = [float(x) for x in getattr(ct, name)()]
        out += [repr(x) for x in vals]
        out += ["%f" % x for x in vals if not abs(x) >= 1e13]   # (NaN passes: 'nan')
    return tuple(out)


def _in_binade(rng, b):
    """a random double of binade b (-1074 .. 1023; below -1022 a subnormal)"""
    if b >= -1022:
        return struct.unpack("<d", struct.pack("<Q", ((b + 1023) << 52) | rng.getrandbits(52)))[0]
    top = 1 << (b + 1074)
    return struct.unpack("<d", struct.pack("<Q", top | rng.getrandbits(b + 1074) if b > -1074 else 1))[0]


@functools.lru_cache(None)
def digits17_19():
    rng = random.Random(20264)
    out = []
    for x in ct.random_bits()[:3000]:
        if np.isfinite(x):
            out += ["%.16e" % x, "%.17g" % x]
    for b in range(-1074, 1024):   # every binade, 18 and 19 digits
        x = _in_binade(rng, b)
        out += ["%.17e" % x, "-%.18e" % x]
    for _ in range(3000):          # underflow to subnormal and to zero, overflow
        nd = rng.choice((18, 19))
        m = rng.randrange(10 ** (nd - 1), 10 ** nd)
        e = rng.randrange(-345, 311)
        out.append(rng.choice(("%de%d", "%dE%+d")) % (m, e - rng.choice((0, nd - 1))))
    assert all(significant_digits(t) <= 19 and len(t) <= 32 for t in out)
    return tuple(out)


def _render(M, X):
    """the decimal M * 10^X, plain where that is short"""
    if X == 0:
        return str(M)
    s = str(M)
    if X < 0 and -X < len(s):
        return s[:X] + "." + s[X:]
    if X < 0 and -X < len(s) + 4:
        return "0." + "0" * (-X - len(s)) + s
    return "%se%d" % (s, X)


@functools.lru_cache(None)
def ties():
    """exact halfway decimals of at most 19 digits, and their two neighbours in the last digit"""
    rng = random.Random(20265)
    mx = []   # (M, X): the value M * 10^X
    for e in range(10):
        for _ in range(40):
            m = rng.randrange(1 << 52, 1 << 53)
            odd = 2 * m + 1                      # 54 bits: halfway between two doubles
            mx.append((odd << e, 0))
            if e == 0:
                mx += [(odd * 5, -1), (odd * 25, -2), (odd * 125, -3)]   # halved, quartered, eighthed
    for q in range(1, 23):
        lo, hi = -(-(1 << 53) // 5 ** q), ((1 << 54) - 1) // 5 ** q
        ws = [w for w in range(lo, min(hi, lo + 400) + 1) if w % 2 == 1]
        if hi - lo > 400:
            ws += [w | 1 for w in (rng.randrange(lo, hi) for _ in range(40)) if (w | 1) <= hi]
        assert ws, q
        mx += [(w, q) for w in ws[:60]]
    out = []
    for M, X in mx:
        if len(str(M).strip("0")) > 19 or len(str(M + 1)) > 19:
            continue
        out += [_render(M, X), _render(M + 1, X), _render(M - 1, X), "-" + _render(M, X)]
    assert len(out) > 3000 and all(significant_digits(t) <= 19 for t in out)
    return tuple(out)


EDGES = ("2.4703282292062327e-324", "2.4703282292062328e-324", "4.9406564584124654e-324", "2.2250738585072011e-308",
         "2.2250738585072014e-308", "1.797693134862315807e308", "1.797693134862315808e308", "9007199254740993",
         "1e400", "1e-400", "1e99999999999999999999", "-1e-99999999999999999999", "0e999", ".5", "5.", "+1",
         "-0.000000", "INF", "-Infinity", "NaN", "-nan", "inf", "+inf", "iNfInItY", "+NAN", "0", "-0", "0.0", "-.0",
         "0e0", "1e0", "1E+0", "1e-0", "1e308", "1e309", "-1e309", "1e-323", "1e-324", "5e-324", "3e-324", "2e-324",
         "0000000000001234567890123456789", "0.0000000000001234567890123456789", "1234567890123456789000000000000",
         "1.234567890123456789000000000000e-5", "000000000000.1234567890123456789e300",
         "-1234567890123456789000000000000e-340", "1234567890123456789000000000000e278",
         "0.0000000000001234567890123456789e-305", "9999999999999999999",
         "9999999999999999999e-19", "0.000000000000000000000000000000000000000000000000000000000001",
         "1" + "0" * 63, "0." + "0" * 61 + "1")
assert all(not may_refuse(t) for t in EDGES)


@functools.lru_cache(None)
def long():
    """what the device may refuse and the twin must get right (and a few of the
    same shapes it may not refuse)"""
    rng = random.Random(20266)
    out = []
    for nd in range(20, 41):
        for _ in range(60):
            m = rng.randrange(10 ** (nd - 1), 10 ** nd)
            k = rng.randrange(0, nd)
            s = str(m)
            out.append((s[:k] + "." + s[k:] if rng.random() < 0.7 else s) + "e%d" % rng.randrange(-330, 300))
    # the halfway cases of 17 digits made longer: a cut after 19 digits cannot decide them
    for t in ties()[:400:4]:
        if "e" not in t:
            out += [t + ("" if "." in t else ".") + "0" * 12 + "1", t + ("" if "." in t else ".") + "0" * 25]
    out += ["%f" % float("1e%d" % k) for k in range(15, 301, 5)]
    out += ["%f" % -1.2345678901234567e13, "%f" % 9.87654321e18, "123456789012345678901234567890",
            "18446744073709551615"]
    out += ["1." + "0" * (MAX_TOKEN - 2) + "1", "0." + "0" * (MAX_TOKEN - 14) + "1234567890123",
            "1" + "0" * MAX_TOKEN, "1e" + "0" * (MAX_TOKEN - 2) + "5", "-" + "0" * MAX_TOKEN, "0" * 300 + "1.5"]
    assert all(len(t) == MAX_TOKEN + 1 for t in out[-6:-1])
    return tuple(out)


BAD = ("1_0", "0x10", "1e", "--1", "1.2.3", "#", "\x80", "1\xff", "e5", ".", "+", "-", "inf1", "nane", "1e+", "1.5e5.5",
       "infinit", "in", "na", "1,2", "1d5", "++1", "1e--1", "1\r2", "(1)", "1f", "0b1", "2\x00")

LISTS = {"roundtrip": roundtrip, "digits17_19": digits17_19, "ties": ties, "edges": lambda: EDGES, "long": long}


@functools.lru_cache(None)
def list_case(name, ncol=1):
    """(text, expected [rows][ncol], tokens) of a list, shared among the tests"""
    tokens = LISTS[name]()
    text, want = table(tokens, ncol)
    want.setflags(write=False)
    return text, want, tokens


def bad_files():
    """(token, where, text, the row it stands in) for every BAD token alone in
    a good 5 x 3 file, in the first, a middle and the last row"""
    good = [["%d.5" % (3 * r + c) for c in range(3)] for r in range(5)]
    out = []
    for tok in BAD:
        for row, col in ((0, 0), (2, 1), (4, 2)):
            cells = [list(r) for r in good]
            cells[row][col] = tok
            text = "".join(" ".join(r) + "\n" for r in cells).encode("latin-1")
            out.append((tok, text, row))
    return out


# ---- structure ---------------------------------------------------------------------------------
def _block(nbytes, ncol=3, seed=0):
    """tokens whose table is close to nbytes long"""
    rng = random.Random(1000 + seed)
    toks, n = [], 0
    while n < nbytes:
        t = rng.choice((repr(rng.uniform(-1e3, 1e3)), "%f" % rng.uniform(-1e4, 0), str(rng.randrange(10 ** 6)),
                        "%.17e" % rng.uniform(-1, 1), "-inf", "nan", "1e-320", "%d" % rng.randrange(10 ** 18, 10 ** 19)))
        toks.append(t)
        n += len(t) + 1
    return toks


def exact_size(nbytes, ncol=3, seed=0):
    """(text of exactly nbytes bytes, expected): the table of _block with blanks
    put in front of the last newline (or cut short by whole rows and padded)"""
    toks = _block(nbytes, ncol, seed)
    while True:
        text, want = table(toks, ncol)
        if len(text) <= nbytes:
            break
        toks = toks[:-ncol]
    pad = nbytes - len(text)
    return text[:-1] + b" " * pad + b"\n", want


def structure_cases(tile):
    """[(name, text, ncol or None, expected array)]: texts the parser must read"""
    out = []
    toks = _block(600, 3, 1)
    base, want = table(toks, 3)
    out.append(("plain", base, 3, want))
    out.append(("ncol found", base, None, want))
    out.append(("crlf", table(toks, 3, eol="\r\n")[0], 3, want))
    out.append(("tabs and runs", table(toks, 3, sep=" \t  ")[0], 3, want))
    out.append(("leading and trailing blanks", table(toks, 3, lead="  \t", trail=" \t ")[0], 3, want))
    out.append(("crlf with trailing blanks", table(toks, 3, eol=" \r\n", lead=" ")[0], 3, want))
    out.append(("no final newline", table(toks, 3, final=False)[0], 3, want))
    out.append(("no final newline, cr", table(toks, 3, final=False)[0] + b"\r", 3, want))
    out.append(("three trailing blank lines", base + b"\n  \n\t\r\n", 3, want))
    out.append(("trailing blanks without newline", base + b"   ", 3, want))
    out.append(("empty", b"", 3, np.empty((0, 3))))
    out.append(("blanks only", b"  \n\t \r\n \n", 3, np.empty((0, 3))))
    out.append(("blanks only, ncol found", b"  \n\t \r\n \n", None, np.empty((0, 0))))
    out.append(("one row", b"1.5 -2 3e5\n", 3, expected(["1.5", "-2", "3e5"]).reshape(1, 3)))
    out.append(("one row, no newline", b"1.5 -2 3e5", None, expected(["1.5", "-2", "3e5"]).reshape(1, 3)))
    out.append(("one token", b"7", 1, expected(["7"]).reshape(1, 1)))
    for ncol in (1, 19, 89, MAX_NCOL):
        t = _block(3 * tile if ncol > 100 else 2000, ncol, ncol)
        text, w = table(t, ncol)
        out.append(("ncol %d" % ncol, text, ncol, w))
    for k in (1, 2, 3):
        for d in (-3, -1, 0, 1, 2):
            text, w = exact_size(k * tile + d, 3, 10 * k + d)
            assert len(text) == k * tile + d
            out.append(("%d tiles %+d bytes" % (k, d), text, 3, w))
    return out


def ragged_cases():
    """[(name, text, ncol, the first ragged row)]"""
    rows = ["%d %d.25 %de-3" % (r, r, r) for r in range(9)]
    def join(rs):
        return ("\n".join(rs) + "\n").encode()
    short = list(rows); short[4] = "4 4.25"
    long_ = list(rows); long_[6] = "6 6.25 6e-3 7"
    blank = rows[:3] + ["  "] + rows[3:]
    empty = rows[:5] + [""] + rows[5:]
    return [("short row", join(short), 3, 4), ("long row", join(long_), 3, 6), ("blank line", join(blank), 3, 3),
            ("empty line", join(empty), 3, 5), ("short last row", join(rows[:-1] + ["8 8.25"]), 3, 8),
            ("short first row", join(["0"] + rows[1:]), 3, 0), ("wrong ncol", join(rows), 4, 0),
            ("short last row, no newline", join(rows[:-1] + ["8 8.25"])[:-1], 3, 8),
            ("leading blank line", b"\n" + join(rows), 3, 0)]


@functools.lru_cache(None)
def seam_text(tile):
    """a 3-tile text (tokens of every length up to MAX_TOKEN among them) and its values"""
    rng = random.Random(77)
    toks = []
    n = 0
    while n < 3 * tile - 200:
        k = rng.randrange(1, MAX_TOKEN + 1)
        if k < 4:
            t = str(rng.randrange(10 ** (k - 1), 10 ** k))
        else:
            d = "".join(rng.choice("0123456789") for _ in range(min(k - 2, 17)))
            t = "1." + d + "0" * (k - 2 - len(d))
        assert len(t) == k
        toks.append(t)
        n += k + 1
    return table(toks, 2)


def shifted(tile, shift):
    """seam_text behind `shift` leading blanks: over shift = 0 .. MAX_TOKEN + 1 a
    token straddles every position of a tile seam and a newline sits on the
    last and on the first byte of a tile"""
    text, want = seam_text(tile)
    return b" " * shift + text, want
