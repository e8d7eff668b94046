"""Test helper: guarded device buffers for the C ABI's memory contract.

include/lfg.h promises that an entry point works in the caller's scratch of
exactly the size function's value, writes outputs of the stated shapes and
leaves const inputs alone.  A case is written once as a function of an
allocator (Plain or Arena below) and runs unchanged on either:

    def case(A):
        x = A.inp("x", numpy_array)            # const input
        pos = A.io("pos", numpy_array)         # updated in place by the call
        out = A.out("out", (W, N), torch.float64)
        ws = A.ws("ws", nbytes)                # scratch of exactly nbytes
        rc = L.lfg_...(ptr(x), ..., ptr(out), ptr(ws), nbytes, A.stream_ptr())

Plain hands out separate torch.empty tensors.  Arena places every buffer in
ONE uint8 device allocation:

    [ pad | guard | payload | guard | payload | guard | ... | pad ]

  * every guard is GUARD bytes (>= 64 KiB and larger than any row a case
    writes) of the byte GUARD_BYTE; the arena begins and ends with PAD bytes
    of it (several MiB), so that an overrun of any plausible size stays inside
    memory the test owns: nothing here can fault, a stray write only becomes
    visible;
  * payloads start at an odd multiple of 256 bytes, the alignment lfg.h asks
    of scratch and no more;
  * `out` and `ws` payloads are pre-filled with POISON (all-ones bytes: a NaN
    no kernel produces as a double, -1 as an int), `ws` optionally with zeros
    or not at all (left over from whatever ran in the arena before);
  * `in` payloads are copied in and kept for comparison.

check() (synchronises) raises on a damaged guard, naming the buffer and the
first damaged byte, and on a changed `in` payload; poisoned(name) gives the
elements of an `out` buffer that still hold poison; result() the bytes of
every out / io buffer for bit comparison between runs.
"""
import ctypes

import numpy as np

GUARD = 64 * 1024
PAD = 4 * 1024 * 1024
GUARD_BYTE = 0xA5
POISON = 0xFF
ALIGN = 256


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nbytes(shape, dtype):
    import torch
    return int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()


class _Base:
    def __init__(self, device="cuda"):
        import torch
        self.device = torch.device(device)
        self.bufs = {}     # name -> (role, tensor view with dtype and shape)
        self.order = []
        self._kept = {}    # name -> host copy of an `in` payload

    def stream_ptr(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _add(self, name, role, t):
        assert name not in self.bufs, name
        self.bufs[name] = (role, t)
        self.order.append(name)
        return t

    def inp(self, name, array):
        import torch
        a = torch.as_tensor(np.ascontiguousarray(array))
        t = self._take(name, a.numel() * a.element_size(), "in").view(a.dtype).view(a.shape)
        t.copy_(a)
        self._add(name, "in", t)
        self._kept[name] = a.clone()
        return t

    def io(self, name, array):
        import torch
        a = torch.as_tensor(np.ascontiguousarray(array))
        t = self._take(name, a.numel() * a.element_size(), "io").view(a.dtype).view(a.shape)
        t.copy_(a)
        return self._add(name, "io", t)

    def out(self, name, shape, dtype):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        raw = self._take(name, _nbytes(shape, dtype), "out")
        raw.fill_(POISON)
        return self._add(name, "out", raw.view(dtype).view(shape))

    def ws(self, name, nbytes):
        raw = self._take(name, int(nbytes), "ws")
        return self._add(name, "ws", raw)

    def tensor(self, name):
        return self.bufs[name][1]

    def raw(self, name):
        import torch
        t = self.bufs[name][1]
        if t.numel() == 0:
            return torch.empty(0, dtype=torch.uint8, device=t.device)
        return t.reshape(-1).view(torch.uint8)

    def poisoned(self, name):
        """bool numpy array, shaped as the buffer: the elements whose every byte is POISON"""
        t = self.bufs[name][1]
        if t.numel() == 0:
            return np.zeros(tuple(t.shape), dtype=bool)
        return (self.raw(name).view(-1, t.element_size()) == POISON).all(dim=1).view(t.shape).cpu().numpy()

    def result(self):
        """name -> bytes (numpy uint8) of every out and io buffer"""
        return {n: self.raw(n).cpu().numpy() for n in self.order if self.bufs[n][0] in ("out", "io")}

    def check_inputs(self):
        import torch
        for n in self.order:
            if self.bufs[n][0] == "in":
                if self._kept[n].numel() == 0:
                    continue
                got, want = self.raw(n).cpu(), self._kept[n].reshape(-1).view(torch.uint8)
                if not torch.equal(got, want):
                    k = int(torch.nonzero(got != want)[0])
                    raise AssertionError("const input %r was changed (first at byte %d of %d)" % (n, k, got.numel()))


class Plain(_Base):
    """separate torch.empty tensors; ws_fill as Arena's"""

    def __init__(self, device="cuda", ws_fill=None):
        super().__init__(device)
        self.ws_fill = ws_fill

    def _take(self, name, nbytes, role):
        import torch
        t = torch.empty(max(nbytes, 0), dtype=torch.uint8, device=self.device)
        if role == "ws" and self.ws_fill is not None:
            t.fill_(self.ws_fill)
        return t

    def check(self):
        import torch
        torch.cuda.synchronize(self.device)
        self.check_inputs()


class Arena(_Base):
    """One guarded allocation (module docstring).  ws_fill: POISON, 0, or None
    (scratch keeps what the arena's previous use left there).  The scratch
    buffers live in a zone of their own, the second half of the arena, so that
    what a reused arena leaves in a case's scratch is mostly the scratch of
    the case before."""

    def __init__(self, nbytes=48 * 1024 * 1024, device="cuda", ws_fill=POISON):
        import torch
        super().__init__(device)
        assert nbytes % (2 * ALIGN) == 0 and nbytes >= 4 * PAD
        self.mem = torch.empty(nbytes + 2 * ALIGN, dtype=torch.uint8, device=self.device)
        # base: the first 512-aligned address, so that offsets decide the odd multiples
        self.base = (-self.mem.data_ptr()) % (2 * ALIGN)
        self.size = nbytes
        self.mem.fill_(GUARD_BYTE)
        self.reset(ws_fill)

    def reset(self, ws_fill=POISON):
        """Forget the buffers (a new case) and restore the guard pattern
        everywhere; with ws_fill None the scratch zone keeps its contents (the
        guards of the new scratch buffers are laid over it as they are taken,
        and what lies behind the last of them is then not checked)."""
        self.bufs, self.order, self._kept = {}, [], {}
        self.ws_fill = ws_fill
        keep_from = self.size // 2 if ws_fill is None else self.size
        self.mem[self.base: self.base + keep_from].fill_(GUARD_BYTE)
        self.spans = []            # (name, role, payload offset, nbytes)
        self.next = {"data": PAD, "ws": self.size // 2}
        self.limit = {"data": self.size // 2 - GUARD, "ws": self.size - PAD}

    def _take(self, name, nbytes, role):
        zone = "ws" if role == "ws" else "data"
        off = self.next[zone] + GUARD
        off += (-off) % ALIGN
        if (off // ALIGN) % 2 == 0:   # an odd multiple of 256: aligned to 256 and to no more
            off += ALIGN
        end = off + nbytes
        assert end + GUARD <= self.limit[zone], "arena too small for %s (%d bytes)" % (name, nbytes)
        # the guards: everything between the previous payload and this one, and GUARD bytes behind it
        self.mem[self.base + self.next[zone]: self.base + off].fill_(GUARD_BYTE)
        self.mem[self.base + end: self.base + end + GUARD + 2 * ALIGN].fill_(GUARD_BYTE)
        self.spans.append((name, zone, off, nbytes))
        self.next[zone] = end
        t = self.mem[self.base + off: self.base + end]
        assert nbytes == 0 or (t.data_ptr() % ALIGN == 0 and t.data_ptr() % (2 * ALIGN) != 0)
        if role == "ws" and self.ws_fill is not None:
            t.fill_(self.ws_fill)
        return t

    def guard_report(self):
        """[] or [(buffer name, side, first damaged byte relative to the payload)]: every byte of
        the arena outside the payloads must hold GUARD_BYTE"""
        import torch
        keep = torch.ones(self.size, dtype=torch.bool, device=self.device)
        for _, _, off, n in self.spans:
            keep[off: off + n] = False
        if self.ws_fill is None:
            keep[self.next["ws"] + GUARD:] = False
        body = self.mem[self.base: self.base + self.size]
        bad = torch.nonzero((body != GUARD_BYTE) & keep).reshape(-1).cpu().numpy()
        out = []
        if bad.size:
            first = int(bad[0])
            best = min(self.spans, key=lambda s: min(abs(first - s[2]), abs(first - (s[2] + s[3]))))
            name, _, off, n = best
            side = "before" if first < off else "after"
            out.append((name, side, first - off, int(bad.size)))
        return out

    def check(self):
        import torch
        torch.cuda.synchronize(self.device)
        rep = self.guard_report()
        if rep:
            name, side, rel, count = rep[0]
            raise AssertionError("guard damaged %s buffer %r: first at byte %d relative to its payload "
                                 "(%d guard bytes changed in all)" % (side, name, rel, count))
        self.check_inputs()
