"""Buffers placed inside larger ones, for tests that call the C entry points themselves: a payload at a chosen element offset of
a byte buffer filled with one byte value, a guard band on either side, and a snapshot for inputs.  A kernel that stores before or
behind its output, writes into an input, or takes a staging or store-width path its pointer does not allow shows up in
guards_ok() / unchanged() or in the result.  Works on any torch device; tests/test_embed_cpu.py checks on the CPU that every one
of these checks can fail.

Pointers: the first guard starts on a 256-byte boundary and guard_bytes is a multiple of 256, so the payload pointer of an
Embedded is offset_elems * itemsize modulo 256, and that of a Workspace is `align` modulo 256 (aligned to `align`, never to 256)."""
import numpy as np
import torch

BASE_ALIGN = 256
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}


def _np_dtype(dtype):
    if isinstance(dtype, torch.dtype):
        return next(k for k, v in TORCH_DT.items() if v == dtype)
    dt = np.dtype(dtype)
    assert dt in TORCH_DT, "unsupported dtype %s" % dt
    return dt


class _Guarded(object):
    """`nbytes` payload bytes `shift` bytes behind a guard of `guard_bytes`, another guard behind them (rounded up so that the
    whole region is a multiple of 256); everything but the payload holds `fill_byte`."""

    def __init__(self, nbytes, shift, fill_byte, guard_bytes, device):
        assert guard_bytes > 0 and guard_bytes % BASE_ALIGN == 0 and 0 <= fill_byte <= 255 and shift >= 0 and nbytes >= 0
        self.fill, self.nbytes = int(fill_byte), int(nbytes)
        self.lo = guard_bytes + shift
        self.hi = self.lo + self.nbytes
        total = -(-(self.hi + guard_bytes) // BASE_ALIGN) * BASE_ALIGN
        self._alloc = torch.empty(total + BASE_ALIGN, dtype=torch.uint8, device=device)
        skip = -self._alloc.data_ptr() % BASE_ALIGN
        self.raw = self._alloc[skip:skip + total]
        self.raw.fill_(self.fill)
        self._snap = None

    def bytes_view(self):
        return self.raw[self.lo:self.hi]

    def ptr(self):
        return self.raw.data_ptr() + self.lo

    def guards_flag(self):
        """guards_ok() as a 0-dim bool tensor on the buffer's device (no synchronisation: see all_true)."""
        return (self.raw[:self.lo] == self.fill).all() & (self.raw[self.hi:] == self.fill).all()

    def guards_ok(self):
        """Both guards still hold the fill byte, bit for bit."""
        return bool(self.guards_flag().item())

    def refill(self):
        self.bytes_view().fill_(self.fill)

    def snapshot(self):
        self._snap = self.bytes_view().clone()

    def unchanged_flag(self):
        assert self._snap is not None, "no snapshot taken"
        return (self.bytes_view() == self._snap).all()

    def unchanged(self):
        """The payload holds the bits it held at the last put() / snapshot()."""
        return bool(self.unchanged_flag().item())


class Embedded(_Guarded):
    """A contiguous tensor of `shape` and `dtype` that starts guard_bytes + offset_elems * itemsize bytes into a byte buffer
    filled with `fill_byte` and has guard_bytes (or a little more) of it behind."""

    def __init__(self, shape, dtype, offset_elems=0, fill_byte=0xA5, guard_bytes=4096, device="cuda"):
        self.np_dtype = _np_dtype(dtype)
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(self.shape, dtype=np.int64))
        _Guarded.__init__(self, n * self.np_dtype.itemsize, offset_elems * self.np_dtype.itemsize, fill_byte, guard_bytes, device)

    def payload(self):
        return self.bytes_view().view(TORCH_DT[self.np_dtype]).view(self.shape)

    def put(self, array):
        """Copy `array` (same number of elements; converted to the dtype) into the payload and take the snapshot."""
        a = np.ascontiguousarray(np.asarray(array), dtype=self.np_dtype).reshape(self.shape)
        self.payload().copy_(torch.from_numpy(a))
        self.snapshot()
        return self

    def host(self):
        return self.payload().cpu().numpy()


class Workspace(_Guarded):
    """Exactly `nbytes` usable bytes between two guards, aligned to `align` (8, or 128 where the entry asks for it) and
    deliberately not to 256."""

    def __init__(self, nbytes, align=8, fill_byte=0xA5, guard_bytes=4096, device="cuda"):
        assert align in (8, 16, 32, 64, 128)
        _Guarded.__init__(self, nbytes, align, fill_byte, guard_bytes, device)

    def zero(self):
        self.bytes_view().zero_()
        return self


def embedded(array, offset_elems=0, dtype=None, device="cuda", **kw):
    """An Embedded input holding `array` (None stays None)."""
    if array is None:
        return None
    a = np.asarray(array)
    return Embedded(a.shape, a.dtype if dtype is None else dtype, offset_elems, device=device, **kw).put(a)


def ptr(b):
    return None if b is None else b.ptr()


def failed(inputs=(), outputs=(), workspaces=()):
    """The names of the buffers whose check fails, with one read-back for all of them: inputs (name -> buffer; None values are
    skipped) must be unchanged with both guards intact, outputs and workspaces must have both guards intact."""
    names, flags = [], []
    for name, b in dict(inputs).items():
        if b is not None:
            names += ["input %s changed" % name, "guard of input %s" % name]
            flags += [b.unchanged_flag(), b.guards_flag()]
    for kind, group in (("output", outputs), ("workspace", workspaces)):
        for name, b in dict(group).items():
            if b is not None:
                names.append("guard of %s %s" % (kind, name))
                flags.append(b.guards_flag())
    if not flags:
        return []
    ok = torch.stack(flags).cpu().tolist()
    return [n for n, f in zip(names, ok) if not f]
