"""Guarded buffers for the workspace-hygiene tests (tests/test_gpu_workspace_hygiene.py).

The C ABI promises that the contents of a workspace, a tape or an output buffer do not matter on entry and that nothing
beyond the declared size is touched.  An `Arena` hands out buffers that make both visible: every buffer lives in a
uint8 tensor of its own, with a 64 KiB guard in front of it and another behind it, the interior pre-filled with one of
three patterns and the guards with a byte that differs from it.  After the call, `check_guards()` names the buffer and
the first guard offset that changed.

The fills:
    0x00  what a fresh allocation usually holds (the arrangement the rest of the suite exercises by accident)
    0xFF  NaN as float32 and float64, -1 as any signed integer (lbdrn_randperm's own sentinel)
    0xA5  a denormal-sized negative float (-2.87e-16), a large integer
A region whose initialisation is missing differs under at least one of them.

A buffer may also be placed OFF its alignment on purpose (tests/test_gpu_call_shapes.py): `skew` bytes past a multiple of
`align`, so that a caller's pointer is aligned to what include/lbdrn_hip.h asks of that argument and to nothing more.  A
test that reuses code which builds its own Arena states the skews once, by buffer name, with `placement(fn)`.

Works on any device (tests/test_guarded_host.py runs it on CPU tensors).  A plain module: no fixture, no marker."""
import contextlib
import ctypes

import torch

GUARD = 1 << 16              # bytes in front of and behind every buffer (a condition of the tests, not a measurement)
FILLS = (0x00, 0xFF, 0xA5)   # in this order: the arrangement the suite already exercises runs first
GUARD_BYTE, GUARD_BYTE_ALT = 0x5A, 0xC3


def fill_id(fill):
    return f"fill{fill:02X}"


def guard_byte(fill):
    """the byte the guards of a buffer filled with `fill` hold: never the fill itself"""
    return GUARD_BYTE if (fill & 0xFF) != GUARD_BYTE else GUARD_BYTE_ALT


class GuardError(AssertionError):
    pass


class Buf:
    """`nbytes` of device memory at an address `skew` bytes past a multiple of `align` (256-byte aligned as the Arena hands
    them out by default), between two guards in the same tensor."""

    def __init__(self, name, nbytes, fill, align, dev, skew=0):
        assert nbytes >= 0 and align >= 1 and 0 <= fill <= 0xFF and 0 <= skew < align
        self.name, self.nbytes, self.fill, self.align, self.skew = name, int(nbytes), fill, align, int(skew)
        self.whole = torch.empty(GUARD + align + self.nbytes + GUARD, dtype=torch.uint8, device=dev)
        base = self.whole.data_ptr()
        self.start = GUARD + (skew - (base + GUARD)) % align    # first offset at that residue with a whole guard in front of it
        self.end = self.start + self.nbytes
        self.whole.fill_(guard_byte(fill))
        self.t = self.whole[self.start:self.end]                # the interior, a view
        self.t.fill_(fill)

    # ---- the interior
    def data_ptr(self):
        return self.whole.data_ptr() + self.start

    @property
    def ptr(self):
        return ctypes.c_void_p(self.data_ptr())

    def view(self, dtype, count=None):
        """the interior (or its first `count` elements) as a 1-D tensor of `dtype`"""
        size = torch.empty(0, dtype=dtype).element_size()
        n = self.nbytes // size if count is None else count
        assert n * size <= self.nbytes, (self.name, n, size, self.nbytes)
        return self.t[:n * size].view(dtype)

    def as_u8(self, count=None):
        return self.view(torch.uint8, count)

    def as_i16(self, count=None):
        return self.view(torch.int16, count)

    def as_u16(self, count=None):
        return self.view(torch.uint16, count)

    def as_i32(self, count=None):
        return self.view(torch.int32, count)

    def as_i64(self, count=None):
        return self.view(torch.int64, count)

    def as_f32(self, count=None):
        return self.view(torch.float32, count)

    def as_f64(self, count=None):
        return self.view(torch.float64, count)

    def write(self, array):
        """copy a numpy array's bytes to the start of the interior"""
        import numpy as np
        raw = torch.from_numpy(np.ascontiguousarray(array).reshape(-1).view(np.uint8).copy())
        assert raw.numel() <= self.nbytes, (self.name, raw.numel(), self.nbytes)
        self.t[:raw.numel()].copy_(raw)
        return self

    def numpy(self, dtype, count=None):
        """the interior (or its first `count` elements of `dtype`) on the host"""
        import numpy as np
        size = np.dtype(dtype).itemsize
        n = self.nbytes // size if count is None else count
        return self.t[:n * size].cpu().numpy().view(dtype).copy()

    # ---- the guards
    def guard_damage(self):
        """None, or (side, offset): the first touched guard byte, as an offset from the interior's start (negative in the
        front guard, >= nbytes in the back guard)"""
        g = guard_byte(self.fill)
        for side, lo, hi in (("front", 0, self.start), ("back", self.end, self.whole.numel())):
            bad = self.whole[lo:hi] != g
            if bool(bad.any()):
                first = int(torch.nonzero(bad)[0].item())
                return side, lo + first - self.start
        return None


_PLACEMENT = None     # name -> skew, for the buffers of every Arena built inside `with placement(fn)`


@contextlib.contextmanager
def placement(fn):
    """Inside the block every Arena places a buffer whose `skew` is not given at fn(name) bytes past a multiple of its
    alignment: one statement of where each argument of a call lies, for code that builds its Arena itself."""
    global _PLACEMENT
    before, _PLACEMENT = _PLACEMENT, fn
    try:
        yield
    finally:
        _PLACEMENT = before


class Arena:
    """Every buffer a test hands to the library: guarded, filled, and checked together."""

    def __init__(self, dev):
        self.dev = torch.device(dev)
        self.bufs = []
        self.consts = []
        self.placement = _PLACEMENT

    def buf(self, nbytes, fill, align=256, name=None, skew=None):
        name = name or f"buf{len(self.bufs)}"
        if skew is None:
            skew = self.placement(name) if self.placement else 0
        b = Buf(name, nbytes, fill, align, self.dev, skew)
        self.bufs.append(b)
        return b

    def const(self, array, name=None, skew=None):
        """an input the call must not change: a guarded buffer holding `array`, remembered for check_consts()"""
        import numpy as np
        a = np.ascontiguousarray(array)
        b = self.buf(a.nbytes, 0x00, name=name or f"const{len(self.consts)}", skew=skew).write(a)
        self.consts.append((b, a.reshape(-1).view(np.uint8).copy()))
        return b

    def check_guards(self):
        for b in self.bufs:
            hit = b.guard_damage()
            if hit is not None:
                side, off = hit
                raise GuardError(f"buffer '{b.name}' ({b.nbytes} bytes, {fill_id(b.fill)}): its {side} guard was written, "
                                 f"first at offset {off} from the buffer's start")

    def check_consts(self):
        import numpy as np
        for b, want in self.consts:
            got = b.numpy(np.uint8)
            if not np.array_equal(got, want):
                first = int(np.flatnonzero(got != want)[0])
                raise GuardError(f"const input '{b.name}' was changed by the call, first at byte {first}")

    def check(self):
        self.check_guards()
        self.check_consts()
