"""chain_prod.txt's rows in bulk (include/lfg_chaintext.h, MODEL_SPEC.md
section 17): the bytes Python's own formatting gives,

    '{0:4d} {1:s} {2:f}\\n'.format(walker0 + k, ' '.join(map(repr, map(float, chain[s, k]))), float(lnprob[s, k]))

for every step s and walker k, without a Python loop over the rows.

    format_rows(chain, lnprob, walker0=0) -> bytes

chain [steps, W, ndim] and lnprob [steps, W].  Tensors on the device go to
the gfx950 kernels (lfg_chain_text): one device read of the total, then one
copy of exactly that many bytes; strided views (a tempered chain's cold level,
a thinned chain) are passed as views.  A chunk in which the device refused a
row (a finite |ln_prob| >= 2^63) is formatted on the host instead.  Host
tensors and numpy arrays go to the kernels' host twin
(cpu_baseline/lfg_cpu_chaintext.cpp), which is exact for every double.

The last resort is the Python expression above (python_rows): it is used for
host data only when the twin's library cannot be loaded, and for a row length
the C ABI refuses (ndim = 0 or beyond LFG_CHAIN_TEXT_MAX_NDIM).  A device
tensor without the HIP library is an error, as everywhere in this package.
"""
import ctypes
import os

import numpy as np

from . import _native

TWIN_PATH = os.path.join(_native.REPO, "cpu_baseline", "liblfg_cpu.so")
_twin = None


def python_rows(chain, lnprob, walker0=0):
    """the reference expression, row by row (host arrays)"""
    chain = np.asarray(chain, dtype=np.float64)
    lnprob = np.asarray(lnprob, dtype=np.float64)
    out = []
    for s in range(chain.shape[0]):
        out.extend("{0:4d} {1:s} {2:f}\n".format(walker0 + k, " ".join(map(repr, map(float, chain[s, k]))),
                                                 float(lnprob[s, k]))
                   for k in range(chain.shape[1]))
    return "".join(out).encode()


def twin():
    """the host twin's library, or None when it cannot be loaded"""
    global _twin
    if _twin is None:
        try:
            L = ctypes.CDLL(TWIN_PATH)
            vp, i64, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
            L.lfg_cpu_chain_text.restype = ci
            L.lfg_cpu_chain_text.argtypes = [vp, i64, i64, ci, i64, i64, vp, i64, i64, i64, vp, ctypes.c_size_t, vp, ci]
            L.lfg_cpu_chain_text_bound.restype = i64
            L.lfg_cpu_chain_text_bound.argtypes = [i64, i64, ci, i64]
            _twin = L
        except (OSError, AttributeError):
            _twin = False
    return _twin or None


def _host_view(a, nd):
    """a float64 array whose strides are whole positive elements, the last
    one contiguous (a copy only when the array is not such a view)"""
    a = np.asarray(a)
    if a.dtype != np.float64:
        a = np.ascontiguousarray(a, dtype=np.float64)
    ok = all(s > 0 and s % 8 == 0 for s, n in zip(a.strides, a.shape) if n > 1)
    if nd == 3 and a.shape[2] > 1 and a.strides[2] != 8:
        ok = False
    return a if ok else np.ascontiguousarray(a)


def _format_host(chain, lnprob, walker0):
    L = twin()
    steps, W, ndim = chain.shape
    if L is None or not 1 <= ndim <= _native.CHAIN_TEXT_MAX_NDIM:
        return python_rows(chain, lnprob, walker0)
    if steps == 0 or W == 0:
        return b""
    chain, lnprob = _host_view(chain, 3), _host_view(lnprob, 2)
    bound = L.lfg_cpu_chain_text_bound(steps, W, ndim, walker0)
    if bound < 0:
        return python_rows(chain, lnprob, walker0)
    # the bound leaves out '%f' of 2^63 and beyond (at most 317 characters)
    with np.errstate(invalid="ignore"):
        bound += 320 * int(np.count_nonzero(np.isfinite(lnprob) & (np.abs(lnprob) >= 2.0 ** 63)))
    out = np.empty(bound, dtype=np.uint8)
    nb = np.zeros(2, dtype=np.int64)

    def ld(a, i):
        return max(1, a.strides[i] // 8)
    rc = L.lfg_cpu_chain_text(chain.ctypes.data, steps, W, ndim, ld(chain, 0), ld(chain, 1), lnprob.ctypes.data,
                              ld(lnprob, 0), ld(lnprob, 1), walker0, out.ctypes.data, bound, nb.ctypes.data, 0)
    _native.check(rc, "lfg_cpu_chain_text")
    return out[:int(nb[0])].tobytes()


def device_rows(chain, lnprob, walker0=0):
    """lfg_chain_text on device tensors: (out [bound] uint8, nbytes [2] int64),
    both on the device and still in flight on the current stream"""
    import torch
    steps, W, ndim = chain.shape

    def view(t, nd):
        if t.dtype != torch.float64:
            t = t.double()
        st = t.stride()
        ok = all(s > 0 for s, n in zip(st, t.shape) if n > 1) and (nd == 2 or t.shape[2] <= 1 or st[2] == 1)
        return t if ok else t.contiguous()
    chain, lnprob = view(chain, 3), view(lnprob, 2)
    L = _native.lib()
    dev = chain.device
    bound = L.lfg_chain_text_bound(steps, W, ndim, walker0)
    if bound < 0:
        raise ValueError("lfg_chain_text refuses steps = %d, W = %d, ndim = %d, walker0 = %d" % (steps, W, ndim, walker0))
    with torch.cuda.device(dev):
        out = torch.empty(max(bound, 1), dtype=torch.uint8, device=dev)
        nbytes = torch.empty(2, dtype=torch.int64, device=dev)
        need = L.lfg_chain_text_workspace_size(steps, W, ndim)
        ws = _native.Workspace.get(need, dev)
        cs, ls = chain.stride(), lnprob.stride()
        rc = L.lfg_chain_text(chain.data_ptr(), steps, W, ndim, max(1, cs[0]), max(1, cs[1]), lnprob.data_ptr(),
                              max(1, ls[0]), max(1, ls[1]), walker0, out.data_ptr(), bound, nbytes.data_ptr(),
                              ws.data_ptr(), ws.numel(), _native.stream_ptr(dev))
    _native.check(rc, "lfg_chain_text")
    return out, nbytes


def format_rows(chain, lnprob, walker0=0):
    """The rows' bytes (module docstring).  chain [steps, W, ndim], lnprob
    [steps, W]: torch tensors on the device or the host, or array-likes."""
    walker0 = int(walker0)
    if walker0 < 0:
        raise ValueError("walker0 must not be negative")
    on_device = hasattr(chain, "device") and hasattr(chain, "data_ptr") and chain.device.type == "cuda"
    if hasattr(chain, "device") and hasattr(chain, "data_ptr") and not on_device:
        chain = chain.detach().numpy()
    if hasattr(lnprob, "device") and hasattr(lnprob, "data_ptr") and not (on_device and lnprob.device == chain.device):
        lnprob = lnprob.detach().cpu().numpy()
    if not on_device:
        chain, lnprob = np.asarray(chain), np.asarray(lnprob)
    elif not hasattr(lnprob, "data_ptr"):
        import torch
        lnprob = torch.as_tensor(np.asarray(lnprob, dtype=np.float64), device=chain.device)
    if chain.ndim != 3 or lnprob.ndim != 2 or tuple(lnprob.shape) != tuple(chain.shape[:2]):
        raise ValueError("chain [steps, W, ndim] and lnprob [steps, W] expected, got %s and %s"
                         % (tuple(chain.shape), tuple(lnprob.shape)))
    steps, W, ndim = (int(n) for n in chain.shape)
    if not on_device:
        return _format_host(chain, lnprob, walker0)
    if not 1 <= ndim <= _native.CHAIN_TEXT_MAX_NDIM:
        return python_rows(chain.cpu().numpy(), lnprob.cpu().numpy(), walker0)
    if steps == 0 or W == 0:
        return b""
    out, nbytes = device_rows(chain, lnprob, walker0)
    total, refused = nbytes.tolist()   # the one device read
    if refused:
        return _format_host(chain.cpu().numpy(), lnprob.cpu().numpy(), walker0)
    return out[:total].cpu().numpy().tobytes()
