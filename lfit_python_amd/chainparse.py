"""chain_prod.txt's numbers in bulk (include/lfg_chainparse.h, MODEL_SPEC.md
section 18): every field the double Python's float(token) gives, bit for bit,
without a Python or numpy loop over the rows.  The inverse of chaintext.

    parse_text(data, ncol=None, device=None) -> [rows][ncol] float64
    read_table(path, skip_lines=0, device=None) -> [rows][ncol]
    read_chain(path, device=None) -> (chain [steps][W][ncol - 1], names)

Bytes on the device, or device= given, go to the gfx950 kernels
(lfg_chain_parse_count, one device read of info, lfg_chain_parse) and the
result stays there.  A field the device refuses (a token beyond
LFG_CHAIN_PARSE_MAX_TOKEN bytes, a mantissa of more than 19 digits whose cut
does not decide the rounding) sends the text to the kernels' host twin
(cpu_baseline/lfg_cpu_chainparse.cpp), which decides every token; host data
goes there at once.  A bad token or a ragged row raises ValueError naming the
first offending row: the callers in sampler, mcmc_utils, calcPhysicalParams
and wdparams then read the file the way they always did.

A device request without the HIP library is an error, as everywhere in this
package; host data without the twin's library raises TwinMissing (a
ValueError, so that those callers fall back as well).
"""
import ctypes
import os

import numpy as np

from . import _native

TWIN_PATH = os.path.join(_native.REPO, "cpu_baseline", "liblfg_cpu.so")
_twin = None
BLANK = b" \t\r\n"
# fit_summary and limbdark --chain read on the device when there is one
# (tests switch it off to compare with the host route)
DEVICE_ROUTE = True


class TwinMissing(ValueError):
    """the host twin's library cannot be loaded"""


def twin():
    """the host twin's library, or None when it cannot be loaded"""
    global _twin
    if _twin is None:
        try:
            L = ctypes.CDLL(TWIN_PATH)
            vp, i64, ci, sz = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_size_t
            L.lfg_cpu_chain_parse_tile_bytes.restype = ci
            L.lfg_cpu_chain_parse_tile_bytes.argtypes = []
            L.lfg_cpu_chain_parse_workspace_size.restype = sz
            L.lfg_cpu_chain_parse_workspace_size.argtypes = [i64]
            L.lfg_cpu_chain_parse_count.restype = ci
            L.lfg_cpu_chain_parse_count.argtypes = [vp, i64, ci, vp, vp, sz]
            L.lfg_cpu_chain_parse.restype = ci
            L.lfg_cpu_chain_parse.argtypes = [vp, i64, ci, vp, i64, vp, vp, sz]
            _twin = L
        except (OSError, AttributeError):
            _twin = False
    return _twin or None


def device_available():
    """a GPU and the HIP library are there (what the command-line tools ask
    before they read a chain on the device)"""
    if not DEVICE_ROUTE or not os.path.exists(_native.LOAD_PATH):
        return False
    try:
        import torch
        return bool(torch.cuda.is_available())
    except ImportError:
        return False


def tile_bytes():
    """bytes of one tile: the device's, or the twin's equal constant"""
    L = twin()
    if L is not None:
        return int(L.lfg_cpu_chain_parse_tile_bytes())
    return int(_native.lib().lfg_chain_parse_tile_bytes())


def first_line_fields(head):
    """the number of fields of the first non-blank line of `head` (bytes)"""
    for line in bytes(head).split(b"\n"):
        n = len(line.split())
        if n:
            return n
    return 0


def _raise_for(info, where):
    rows, fields, bad, refused, ragged, first = (int(v) for v in info[:6])
    if ragged:
        raise ValueError("%s: row %d has not the %s fields of the others (%d fields in %d rows)"
                         % (where, first, "same number of" if rows else "", fields, rows))
    if bad:
        raise ValueError("%s: row %d holds a field that is not a number (%d such fields)" % (where, first, bad))


def _host_bytes(data):
    """a contiguous uint8 numpy view (a copy only where there is no such view)"""
    if hasattr(data, "data_ptr"):
        data = data.detach().cpu().numpy()
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise TypeError("text is uint8, not %s" % data.dtype)
        return np.ascontiguousarray(data).reshape(-1)
    return np.frombuffer(data, dtype=np.uint8)


def parse_host(data, ncol=None):
    """the twin on host bytes: ([rows][ncol] float64 array, info [8])"""
    L = twin()
    if L is None:
        raise TwinMissing("the host twin %s is missing: build it with cpu_baseline.cpu.build()" % TWIN_PATH)
    a = _host_bytes(data)
    n = int(a.size)
    if ncol is None:
        ncol = first_line_fields(_first_lines(a))
    ncol = int(ncol)
    if ncol == 0:                      # blanks only
        return np.empty((0, 0)), np.zeros(8, np.int64)
    if not 1 <= ncol <= _native.CHAIN_PARSE_MAX_NCOL:
        raise ValueError("rows of %d fields: at most %d" % (ncol, _native.CHAIN_PARSE_MAX_NCOL))
    need = L.lfg_cpu_chain_parse_workspace_size(n)
    if need == 0:
        raise ValueError("a text of %d bytes is refused" % n)
    ws = np.empty(need, dtype=np.uint8)
    info = np.zeros(8, dtype=np.int64)
    keep = np.zeros(1, np.uint8)
    p = a.ctypes.data if n else keep.ctypes.data
    _native.check(L.lfg_cpu_chain_parse_count(p, n, ncol, info.ctypes.data, ws.ctypes.data, need),
                  "lfg_cpu_chain_parse_count")
    _raise_for(info, "chain text")
    rows = int(info[0])
    out = np.empty((rows, ncol))
    _native.check(L.lfg_cpu_chain_parse(p, n, ncol, out.ctypes.data if rows else keep.ctypes.data, rows,
                                        info.ctypes.data, ws.ctypes.data, need), "lfg_cpu_chain_parse")
    _raise_for(info, "chain text")
    return out, info


def _first_lines(a, limit=1 << 16):
    """the bytes up to the end of the first non-blank line (host numpy or a
    device tensor): what ncol is found from"""
    n = int(a.shape[0])
    size = limit
    while True:
        head = a[:size]
        head = bytes(head.cpu().numpy().tobytes() if hasattr(head, "data_ptr") else head.tobytes())
        s = head.lstrip(BLANK)
        if b"\n" in s or size >= n:
            return head
        size *= 16


def parse_device(text, ncol=None):
    """the kernels on a device uint8 tensor: (out [rows][ncol] device tensor,
    info as a list of 8 ints).  Two device reads of info: between the calls
    and behind them."""
    import torch
    L = _native.lib()
    dev = text.device
    text = text.reshape(-1)
    if not text.is_contiguous():
        text = text.contiguous()
    n = int(text.numel())
    if ncol is None:
        ncol = first_line_fields(_first_lines(text))
    ncol = int(ncol)
    if ncol == 0:
        return torch.empty((0, 0), dtype=torch.float64, device=dev), [0] * 4 + [0, -1, 0, 0]
    if not 1 <= ncol <= _native.CHAIN_PARSE_MAX_NCOL:
        raise ValueError("rows of %d fields: at most %d" % (ncol, _native.CHAIN_PARSE_MAX_NCOL))
    need = L.lfg_chain_parse_workspace_size(n)
    if need == 0:
        raise ValueError("a text of %d bytes is refused" % n)
    with torch.cuda.device(dev):
        info = torch.empty(8, dtype=torch.int64, device=dev)
        ws = _native.Workspace.get(need, dev)
        st = _native.stream_ptr(dev)
        keep = torch.empty(16, dtype=torch.uint8, device=dev)
        p = text.data_ptr() if n else keep.data_ptr()
        _native.check(L.lfg_chain_parse_count(p, n, ncol, info.data_ptr(), ws.data_ptr(), ws.numel(), st),
                      "lfg_chain_parse_count")
        got = info.tolist()            # the one device read between the two calls
        _raise_for(got, "chain text")
        rows = got[0]
        out = torch.empty((rows, ncol), dtype=torch.float64, device=dev)
        _native.check(L.lfg_chain_parse(p, n, ncol, out.data_ptr() if rows else keep.data_ptr(), rows,
                                        info.data_ptr(), ws.data_ptr(), ws.numel(), st), "lfg_chain_parse")
        got = info.tolist()
    _raise_for(got, "chain text")
    return out, got


def parse_text(data, ncol=None, device=None):
    """[rows][ncol] float64 of the text `data`: bytes, bytearray, memoryview,
    a numpy uint8 array or a torch uint8 tensor.  A device tensor, or device=
    given, goes to the kernels and a device tensor comes back; everything else
    goes to the host twin and a numpy array comes back.  ncol=None: the fields
    of the first non-blank line.  ValueError for a bad token or a ragged row,
    naming the first such row."""
    on_device = hasattr(data, "data_ptr") and data.device.type == "cuda"
    if not on_device and device is None:
        return parse_host(data, ncol)[0]
    import torch
    _native.require_gpu()
    if on_device:
        if data.dtype != torch.uint8:
            raise TypeError("text is uint8, not %s" % data.dtype)
        text = data
    else:
        a = _host_bytes(data)
        if ncol is None:               # (found before the copy: no device read for it)
            ncol = first_line_fields(_first_lines(a))
        text = torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device(device))
    out, info = parse_device(text, ncol)
    if info[3]:                        # refused fields: the twin decides them
        host, _ = parse_host(text, ncol if ncol is not None else out.shape[1])
        out = torch.from_numpy(host).to(text.device)
    return out


def _skip_lines(a, skip_lines):
    """the offset behind `skip_lines` lines of the uint8 array a"""
    off = 0
    for _ in range(int(skip_lines)):
        size = 4096
        while True:
            hit = np.flatnonzero(a[off:off + size] == 10)
            if hit.size:
                off += int(hit[0]) + 1
                break
            if off + size >= a.size:
                return int(a.size)
            size *= 16
    return off


def read_table(path, skip_lines=0, device=None):
    """The numbers of a whitespace-separated file without its first
    `skip_lines` lines: parse_text of the file's bytes (one np.fromfile)."""
    a = np.fromfile(path, dtype=np.uint8)
    return parse_text(a[_skip_lines(a, skip_lines):], device=device)


def try_table(path, skip_lines=0):
    """read_table on the host for the callers that keep their earlier reader
    as the fallback: the array, or None for anything but a file name, for a
    text the parser reports as bad or ragged, for no rows at all, and when
    the twin's library is absent"""
    if not isinstance(path, (str, os.PathLike)):
        return None
    try:
        t = read_table(path, skip_lines)
    except ValueError:
        return None
    return t if t.shape[0] else None


def read_chain(path, device=None):
    """A chain file as sampler.write_chain writes it -> (chain, names).

    names: the header's names without walker_no (ln_prob included: a row of
    the chain is the file's row without its walker number).  chain
    [steps][W][ncol - 1]: a view of the parsed [rows][ncol] buffer with the
    walker column sliced away, a device tensor with device=, else a numpy
    array.  The walker column must count 0 .. W - 1 over and over, with
    W = its maximum + 1 and rows a multiple of W: ValueError otherwise."""
    a = np.fromfile(path, dtype=np.uint8)
    off = _skip_lines(a, 1)
    names = a[:off].tobytes().decode().split()[1:]
    flat = parse_text(a[off:], device=device)
    rows, ncol = (int(v) for v in flat.shape)
    if rows == 0 or ncol < 2:
        raise ValueError("%s: no rows of a walker number and values" % path)
    wcol = flat[:, 0]
    W = int(wcol.max()) + 1 if bool((wcol == wcol).all()) else 0
    if W < 1 or rows % W != 0:
        raise ValueError("%s: %d rows do not divide among walkers 0 .. %d" % (path, rows, W - 1))
    grid = flat.reshape(rows // W, W, ncol)
    if hasattr(grid, "data_ptr"):
        import torch
        want = torch.arange(W, dtype=torch.float64, device=grid.device)
        regular = bool((grid[:, :, 0] == want).all())
    else:
        regular = bool((grid[:, :, 0] == np.arange(W, dtype=np.float64)).all())
    if not regular:
        raise ValueError("%s: the walker numbers do not count 0 .. %d in every step" % (path, W - 1))
    return grid[:, :, 1:], names
