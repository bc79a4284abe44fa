"""Parents too big to build on the host, for tests that call the C entry points themselves: the counterpart of tests/embed.py
for rows that lie gigabytes from the pointer the entry is given.  A FarParent is ONE device allocation filled with one byte
value: a low guard, the (B, Tmax, ld) parent, an ordinary guard band.  Small host arrays are placed into a few rows of it;
everything else stays the fill byte, so only the ADDRESSES are far apart.  After the call, untouched() takes the regions the
call may write out again and checks that the whole allocation is the fill byte once more: a row offset that wrapped in 32 bits
lands inside the caller's own buffer and shows up there as a stray write (or, on the read side, as a wrong value), not as a
fault.  With a low guard of 2^31 bytes that also holds for a 32-bit byte offset that was sign-extended.

Nothing here builds a host array larger than the placed pieces, and the whole-buffer fill and check run on the buffer's
device in pieces of at most 256 MiB.  Works on any torch device; tests/test_far_cpu.py shows on the CPU, with the boundaries
scaled down, that every kind of wrap is caught."""
import numpy as np
import torch

from embed import BASE_ALIGN, TORCH_DT, _np_dtype

PIECE_BYTES = 256 << 20
BOUNDARIES = (("2^31 bytes", "bytes", 1 << 31), ("2^32 bytes", "bytes", 1 << 32), ("2^31 elements", "elements", 1 << 31))
MEM_CAP = 12 << 30              # peak device memory a far test may use
BIG_GUARD = 1 << 31


def low_guard_for(payload_bytes, other_bytes=0, cap=MEM_CAP):
    """2^31 bytes where the parent, the check's temporaries (two pieces) and the call's other arrays stay under `cap` with
    it, 4096 bytes otherwise."""
    need = payload_bytes + other_bytes + 2 * PIECE_BYTES + (64 << 20)
    return BIG_GUARD if need + BIG_GUARD <= cap else 4096


class _Region(object):
    def __init__(self, kind, b, t0, t1, c0, c1, data=None):
        self.kind, self.b, self.t0, self.t1, self.c0, self.c1, self.data = kind, b, t0, t1, c0, c1, data

    def covers(self, o):
        return self.b == o.b and self.t0 <= o.t0 and o.t1 <= self.t1 and self.c0 <= o.c0 and o.c1 <= self.c1

    def overlaps(self, o):
        return self.b == o.b and self.t0 < o.t1 and o.t0 < self.t1 and self.c0 < o.c1 and o.c0 < self.c1

    def __repr__(self):
        return "%s b=%d rows [%d, %d) cols [%d, %d)" % (self.kind, self.b, self.t0, self.t1, self.c0, self.c1)


class FarParent(object):
    """A (B, Tmax, ld) array of `dtype` low_guard_bytes into one allocation of fill_byte, guard_bytes (or a little more) of
    it behind.  Rows are addressed as (b, rows, col0): rows is a count (the first rows of the utterance) or (t0, t1)."""

    def __init__(self, shape, dtype, low_guard_bytes=4096, fill_byte=0xA5, device="cuda", boundaries=BOUNDARIES, guard_bytes=4096,
                 piece_bytes=PIECE_BYTES):
        self.np_dtype = _np_dtype(dtype)
        self.isz = self.np_dtype.itemsize
        self.B, self.Tmax, self.ld = (int(s) for s in shape)
        assert self.B >= 0 and self.Tmax >= 0 and self.ld >= 0 and 0 <= fill_byte <= 255 and 0 < piece_bytes <= PIECE_BYTES
        assert low_guard_bytes > 0 and low_guard_bytes % BASE_ALIGN == 0 and guard_bytes > 0 and guard_bytes % BASE_ALIGN == 0
        self.fill, self.piece = int(fill_byte), int(piece_bytes)
        self.nbytes = self.B * self.Tmax * self.ld * self.isz
        self.lo = int(low_guard_bytes)
        self.hi = self.lo + self.nbytes
        total = -(-(self.hi + guard_bytes) // BASE_ALIGN) * BASE_ALIGN
        self._alloc = torch.empty(total + BASE_ALIGN, dtype=torch.uint8, device=device)
        skip = -self._alloc.data_ptr() % BASE_ALIGN
        self.raw = self._alloc[skip:skip + total]
        for p in self._pieces():
            p.fill_(self.fill)
        self.view = self.raw[self.lo:self.hi].view(TORCH_DT[self.np_dtype]).view(self.B, self.Tmax, self.ld)
        self.boundaries = tuple(boundaries)
        self.regions = []

    def free(self):
        """Drops the allocation (the caller still empties the cache)."""
        self.view = self.raw = self._alloc = None

    def _pieces(self):
        n = self.raw.numel()
        for s in range(0, n, self.piece):
            yield self.raw[s:min(s + self.piece, n)]

    def _rows(self, rows):
        t0, t1 = (0, rows) if isinstance(rows, (int, np.integer)) else rows
        assert 0 <= t0 <= t1 <= self.Tmax, rows
        return int(t0), int(t1)

    def _slice(self, r):
        return self.view[r.b, r.t0:r.t1, r.c0:r.c1]

    def _add(self, kind, b, rows, col0, width, data=None):
        t0, t1 = self._rows(rows)
        assert 0 <= b < self.B and 0 <= col0 and width >= 0 and col0 + width <= self.ld, (b, col0, width)
        r = _Region(kind, int(b), t0, t1, int(col0), int(col0 + width), data)
        self.regions.append(r)
        return r

    # ---- the caller's side

    def ptr(self, col0=0):
        """The pointer to hand to the C entry: element (0, 0, col0)."""
        return self.raw.data_ptr() + self.lo + col0 * self.isz

    def cols(self, col0, width):
        """The (B, Tmax, width) view of columns [col0, col0 + width): the column slice the tensor wrappers take."""
        assert 0 <= col0 and col0 + width <= self.ld
        return self.view[:, :, col0:col0 + width]

    def place(self, b, rows, col0, array):
        """Writes a host array (rows x width; converted to the dtype) into the rows of utterance b from column col0 on."""
        a = np.ascontiguousarray(np.asarray(array), dtype=self.np_dtype)
        t0, t1 = self._rows(rows)
        assert a.ndim == 2 and a.shape[0] == t1 - t0, (a.shape, rows)
        r = self._add("placed", b, rows, col0, a.shape[1], a.copy())
        self._slice(r).copy_(torch.from_numpy(a))
        return self

    def expect_written(self, b, rows, col0, width):
        """Declares a region the call may write."""
        self._add("expected", b, rows, col0, width)
        return self

    def read(self, b, rows, col0, width):
        t0, t1 = self._rows(rows)
        return self.view[b, t0:t1, col0:col0 + width].cpu().numpy()

    def span(self, r, col0=0):
        """(first byte, byte behind the last) of a region, relative to ptr(col0)."""
        first = ((r.b * self.Tmax + r.t0) * self.ld + r.c0 - col0) * self.isz
        last = ((r.b * self.Tmax + r.t1 - 1) * self.ld + r.c1 - col0) * self.isz
        return first, last

    def crossed(self, col0=0):
        """The names of the boundaries that some placed or expected region straddles (it begins before the boundary and ends
        after it) or lies beyond, in bytes or elements from ptr(col0)."""
        got = set()
        for r in self.regions:
            if r.t1 == r.t0 or r.c1 == r.c0:
                continue
            first, last = self.span(r, col0)
            for name, unit, at in self.boundaries:
                at_bytes = at * (self.isz if unit == "elements" else 1)
                if last > at_bytes:                                 # straddles (first < at_bytes) or lies beyond
                    got.add(name)
        return got

    def straddled(self, col0=0):
        """The names of the boundaries that ONE ROW of some region straddles: live data on both sides, mid-row."""
        got = set()
        for r in self.regions:
            for t in range(r.t0, r.t1):
                first = ((r.b * self.Tmax + t) * self.ld + r.c0 - col0) * self.isz
                last = first + (r.c1 - r.c0) * self.isz
                for name, unit, at in self.boundaries:
                    at_bytes = at * (self.isz if unit == "elements" else 1)
                    if first < at_bytes < last:
                        got.add(name)
        return got

    def untouched(self, rest=None):
        """The checks that fail, as a list of texts (empty: all hold).  Every placed region that no expected region covers
        must hold the bits that were placed; then the placed and expected regions are refilled and the whole allocation must
        be one byte value again: the fill byte in the guards, and in the parent `rest` (default: the fill byte too; 0 for an
        output whose every row the call writes, as zeros outside the expected regions).  Read the results out first: they
        are gone after."""
        rest = self.fill if rest is None else int(rest)
        fails = []
        expected = [r for r in self.regions if r.kind == "expected"]
        for r in self.regions:
            if r.kind != "placed" or r.data is None:
                continue
            if any(e.covers(r) for e in expected):
                continue                                            # in place: the call writes where its input was
            assert not any(e.overlaps(r) for e in expected), ("an expected region covers part of a placed one", r)
            got = self._slice(r).cpu().numpy()
            if got.tobytes() != r.data.tobytes():
                fails.append("input changed: %r" % r)
        for r in self.regions:
            self._refill(r, rest)
            r.data = None                                           # (a second call checks the bytes alone)
        spans = []                                                  # (first byte in raw, piece, the byte it must hold)
        for s, e, byte in ((0, self.lo, self.fill), (self.lo, self.hi, rest), (self.hi, self.raw.numel(), self.fill)):
            spans += [(k, self.raw[k:min(k + self.piece, e)], byte) for k in range(s, e, self.piece)]
        flags = [(p == byte).all() for _, p, byte in spans]
        ok = torch.stack(flags).cpu().tolist() if flags else []
        for f, (k, p, byte) in zip(ok, spans):
            if not f:
                bad = p != byte
                n = int(bad.sum().item())
                first = int(bad.to(torch.uint8).argmax().item()) + k - self.lo
                fails.append("stray write: %d bytes changed from payload byte offset %d on (payload is [0, %d))" % (n, first, self.nbytes))
        return fails

    def forget(self):
        """Drops the regions (after untouched(), before the parent serves another call in another role)."""
        self.regions = []

    def _refill(self, r, byte):
        bytes3 = self.raw[self.lo:self.hi].view(self.B, self.Tmax, self.ld * self.isz)
        bytes3[r.b, r.t0:r.t1, r.c0 * self.isz:r.c1 * self.isz].fill_(byte)
