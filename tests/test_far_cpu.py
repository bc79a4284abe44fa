"""tests/far.py on CPU tensors (-m "not gpu"), with the boundaries scaled down to 2^12 bytes, 2^13 bytes and 2^11 elements: the
entry shapes of the far tests are emulated with a few lines of numpy that gather and scatter rows by byte offset from the
parent's pointer, and every kind of 32-bit wrap is planted into that offset in turn.  Each planted wrap must fail
untouched() or the value comparison, the unplanted emulation must pass: every check of the helper is shown to be able to fail
(the contract tests/test_embed_cpu.py gives embed.py)."""
import numpy as np
import pytest
import torch

import far
from far import FarParent

SCALED = (("2^31 bytes", "bytes", 1 << 12), ("2^32 bytes", "bytes", 1 << 13), ("2^31 elements", "elements", 1 << 11))
ALL = {"2^31 bytes", "2^32 bytes", "2^31 elements"}
# 13 rows of 102 elements: row 5 (float64) / row 10 (float32) of utterance 0 starts 16 bytes below 2^12, rows from 6 / 11 on lie
# more than 2^12 bytes from their utterance's first, three utterances reach past 2^11 elements in either type
B, T, LD, W = 3, 13, 102, 9


def _parent(dtype, shape=(B, T, LD), low=1 << 12):
    return FarParent(shape, dtype, low_guard_bytes=low, device="cpu", boundaries=SCALED, piece_bytes=1000)


# ---------------------------------------------------------------------------------------------------- the helper itself

@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_layout_pointer_and_round_trip(dtype):
    p = _parent(dtype)
    isz = np.dtype(dtype).itemsize
    assert p.nbytes == B * T * LD * isz and p.lo == 4096 and p.raw.numel() - p.hi >= 4096
    assert p.ptr() == p.raw.data_ptr() + 4096 and p.ptr(7) == p.ptr() + 7 * isz and p.ptr() % 256 == 0
    assert bool((p.raw == 0xA5).all())
    a = (np.arange(4 * 5).reshape(4, 5) % 11).astype(dtype)
    p.place(2, (3, 7), 90, a)
    assert np.array_equal(p.read(2, (3, 7), 90, 5), a) and p.read(2, (3, 7), 90, 5).dtype == np.dtype(dtype)
    # the bytes sit where the C entry will look for them: element ((b * Tmax + t) * ld + col) from ptr()
    raw = p.raw.numpy()
    off = p.lo + ((2 * T + 4) * LD + 91) * isz
    assert raw[off:off + isz].tobytes() == a[1, 1:2].tobytes()
    assert p.untouched() == []
    assert bool((p.raw == 0xA5).all())                              # untouched() took the placed rows out again
    with pytest.raises(AssertionError):
        p.place(0, 2, LD - 4, np.zeros((2, 5)))                     # behind the row's end
    with pytest.raises(AssertionError):
        p.place(0, (0, T + 1), 0, np.zeros((T + 1, 1)))


@pytest.mark.parametrize("where", ["first byte of the low guard", "just before the parent", "between two placed rows",
                                   "an unplaced row", "just behind the parent", "last byte of the rear guard"])
def test_one_byte_anywhere_outside_the_regions_is_seen(where):
    p = _parent(np.float64)
    p.place(1, 2, 3, np.ones((2, 4)))
    pos = {"first byte of the low guard": 0, "just before the parent": p.lo - 1,
           "between two placed rows": p.lo + ((T + 0) * LD + 7) * 8, "an unplaced row": p.lo + ((2 * T + 5) * LD) * 8 + 3,
           "just behind the parent": p.hi, "last byte of the rear guard": p.raw.numel() - 1}[where]
    p.raw[pos] = 0x5A
    fails = p.untouched()
    assert len(fails) == 1 and "stray write: 1 bytes changed from payload byte offset %d on" % (pos - p.lo) in fails[0], fails
    p.raw[pos] = 0xA5
    assert p.untouched() == []


def test_inputs_must_keep_their_bits_and_expected_regions_may_change():
    p = _parent(np.float64)
    p.place(0, 3, 0, np.zeros((3, 2))).place(1, 1, 5, np.ones((1, 3)))
    p.expect_written(2, (4, 6), 10, 4)
    p.view[2, 4:6, 10:14] = 7.0                                     # what outputs are for
    assert p.untouched() == []
    p = _parent(np.float64)
    p.place(0, 3, 0, np.zeros((3, 2)))
    p.view[0, 1, 1] = -0.0                                          # equal as a number, still a change
    assert p.untouched() == ["input changed: placed b=0 rows [0, 3) cols [0, 2)"]
    # in place: an expected region that covers a placed one lifts the input check; one that covers part of it is a mistake
    p = _parent(np.float64)
    p.place(0, 3, 0, np.zeros((3, 2))).expect_written(0, 3, 0, 2)
    p.view[0, :3, :2] = 1.0
    assert p.untouched() == []
    p = _parent(np.float64)
    p.place(0, 3, 0, np.zeros((3, 2))).expect_written(0, 2, 0, 2)
    with pytest.raises(AssertionError):
        p.untouched()
    # forget(): the parent in another role, its earlier expected regions gone
    p = _parent(np.float64)
    p.expect_written(0, 3, 0, 2)
    assert p.untouched() == []
    p.forget()
    p.place(0, 3, 0, np.zeros((3, 2)))
    p.view[0, 2, 1] = 1.0
    assert p.untouched() == ["input changed: placed b=0 rows [0, 3) cols [0, 2)"] and p.crossed() == set()
    # a write one column beside an expected region
    p = _parent(np.float32)
    p.expect_written(1, 2, 4, 3)
    p.view[1, 1, 7] = 0.0
    assert len(p.untouched()) == 1


def test_an_output_written_everywhere_is_zero_outside_its_expected_regions():
    """untouched(rest=0): the call writes every row of the parent, zeros where nothing is live; the guards keep the fill."""
    p = _parent(np.float64)
    p.expect_written(1, T, 0, LD)
    assert len(p.untouched(rest=0)) >= 1                            # nothing was written: the parent still holds the fill byte
    p.view.zero_()
    p.view[1] = 3.0
    assert p.untouched(rest=0) == []
    p.view[2, 4, 7] = 5e-324                                        # one bit in a dead utterance
    fails = p.untouched(rest=0)
    assert len(fails) == 1 and "payload byte offset %d " % (((2 * T + 4) * LD + 7) * 8) in fails[0], fails
    p.view[2, 4, 7] = 0.0
    p.raw[p.lo - 1] = 0                                             # a zero just before the parent is a stray write
    assert len(p.untouched(rest=0)) == 1


def test_crossed_reports_a_boundary_a_region_straddles_or_lies_beyond():
    p = _parent(np.float64)
    assert p.crossed() == set()
    p.place(0, 5, 0, np.zeros((5, 102)))                            # ends at byte 4080
    assert p.crossed() == set() and p.straddled() == set()
    p.place(0, (5, 6), 0, np.zeros((1, 2)))                         # [4080, 4096): ends AT the boundary
    assert p.crossed() == set()
    p.expect_written(0, (5, 6), 0, 3)                               # [4080, 4104)
    assert p.crossed() == {"2^31 bytes"} and p.straddled() == {"2^31 bytes"}
    p.place(1, 1, 0, np.zeros((1, 1)))                              # utterance 1 starts at byte 10608: beyond 2^13, mid-row of none
    assert p.crossed() == {"2^31 bytes", "2^32 bytes"} and p.straddled() == {"2^31 bytes"}
    p.place(1, (7, 8), 0, np.zeros((1, 11)))                        # element 2040 .. 2051
    assert p.crossed() == ALL and p.straddled() == {"2^31 bytes", "2^31 elements"}
    # from a shifted pointer the offsets are smaller
    q = _parent(np.float64)
    q.place(0, (5, 6), 0, np.zeros((1, 3)))
    assert q.crossed() == {"2^31 bytes"} and q.crossed(col0=1) == set()
    # an empty region crosses nothing
    e = _parent(np.float32)
    e.place(2, (12, 12), 0, np.zeros((0, 4)))
    assert e.crossed() == set() and e.untouched() == []


def test_low_guard_is_two_gib_where_the_cap_allows():
    assert far.low_guard_for(6 << 30) == 1 << 31
    assert far.low_guard_for(9 << 30) == 1 << 31                    # the float32 wide parent: 9 utterances of 2^30 - 64 bytes
    assert far.low_guard_for(10 << 30) == 4096
    assert far.low_guard_for(6 << 30, other_bytes=4 << 30) == 4096
    assert far.PIECE_BYTES == 256 << 20 and far.MEM_CAP == 12 << 30
    assert [name for name, _, _ in far.BOUNDARIES] == [name for name, _, _ in SCALED]
    assert [at for _, _, at in far.BOUNDARIES] == [1 << 31, 1 << 32, 1 << 31]


# ---------------------------------------------------------------------------------------------------- planted wraps

def _wrap(fault, b, t, c, isz, ld=LD):
    """The byte offset of element (b, t, c) from the pointer as a kernel with the planted fault computes it."""
    elem = (b * T + t) * ld + c
    byte = elem * isz
    if fault is None:
        return byte
    if fault == "byte offset modulo 2^12":
        return byte % (1 << 12)
    if fault == "byte offset modulo 2^13":
        return byte % (1 << 13)
    if fault == "byte offset sign-extended from 13 bits":
        low = byte % (1 << 13)
        return np.where(low >= (1 << 12), low - (1 << 13), low)
    if fault == "element index modulo 2^11":
        return (elem % (1 << 11)) * isz
    if fault == "utterance base right, t * ld wrapped":
        return b * T * ld * isz + ((t * ld * isz) % (1 << 12)) + c * isz
    raise ValueError(fault)


FAULTS = ["byte offset modulo 2^12", "byte offset modulo 2^13", "byte offset sign-extended from 13 bits",
          "element index modulo 2^11", "utterance base right, t * ld wrapped"]


def _addresses(p, col, width, fault):
    """Byte positions in p.raw of columns [col, col + width) of every row, (B * T * width,) x itemsize."""
    b, t, c = np.meshgrid(np.arange(B), np.arange(T), np.arange(col, col + width), indexing="ij")
    pos = p.lo + _wrap(fault, b.ravel(), t.ravel(), c.ravel(), p.isz, p.ld)
    assert (pos >= 0).all() and (pos + p.isz <= p.raw.numel()).all()
    return pos[:, None] + np.arange(p.isz)[None, :]


def _entry(src, in_col, dst, out_col, fault_src=None, fault_dst=None):
    """out[b, t, out_col + j] = 2 * in[b, t, in_col + j] + 1 on every row, by offset from the two pointers."""
    x = src.raw.numpy()[_addresses(src, in_col, W, fault_src)].copy().view(src.np_dtype)[:, 0]
    y = (2 * x + 1).astype(dst.np_dtype)
    dst.raw.numpy()[_addresses(dst, out_col, W, fault_dst)] = y[:, None].view(np.uint8)


def _run(shape, dtype, fault):
    """One emulated call on a fresh far parent; returns (values right, untouched() of every parent)."""
    rng = np.random.RandomState(3)
    x = rng.randn(B, T, W).astype(dtype)
    wide = _parent(dtype)
    small = _parent(dtype, shape=(B, T, W), low=4096)
    # every shape puts its rows at column 0 (rows that straddle the boundaries mid-row) or at the row's end (t * ld + col large)
    if shape == "wide rows in, dense rows out":
        src, in_col, dst, out_col, f_src, f_dst = wide, LD - W, small, 0, fault, None
    elif shape == "dense rows in, wide rows out":
        src, in_col, dst, out_col, f_src, f_dst = small, 0, wide, 0, None, fault
    elif shape == "a column slice of the parent into another":
        src, in_col, dst, out_col, f_src, f_dst = wide, 0, wide, LD - W, fault, fault
    elif shape == "in place":
        src, in_col, dst, out_col, f_src, f_dst = wide, 0, wide, 0, fault, fault
    for b in range(B):
        src.place(b, T, in_col, x[b])
        dst.expect_written(b, T, out_col, W)
    assert wide.crossed() == ALL, wide.crossed()
    if shape != "wide rows in, dense rows out":
        assert wide.straddled() == ALL, wide.straddled()            # live data on both sides of every boundary, mid-row
    _entry(src, in_col, dst, out_col, f_src, f_dst)
    got = np.stack([dst.read(b, T, out_col, W) for b in range(B)])
    right = np.array_equal(got, (2 * x + 1).astype(dtype))
    return right, wide.untouched() + (small.untouched() if small in (src, dst) else [])


SHAPES = ["wide rows in, dense rows out", "dense rows in, wide rows out", "a column slice of the parent into another", "in place"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_unplanted_emulation_passes(shape, dtype):
    right, fails = _run(shape, dtype, None)
    assert right and fails == [], fails


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_planted_wrap_is_caught(shape, fault, dtype):
    right, fails = _run(shape, dtype, fault)
    assert not right, "the values did not notice"                   # rows were read from, or never written to, their place
    if shape != "wide rows in, dense rows out":
        assert fails, "untouched() did not notice the writes that landed elsewhere"
    else:
        assert fails == []                                          # a wrapped READ leaves no trace but the values


def test_the_wraps_differ_from_the_right_offset_only_beyond_their_boundary():
    """The planted faults are the pictures the far tests tell apart: each one is the identity below its boundary."""
    b, t, c = np.meshgrid(np.arange(B), np.arange(T), np.arange(LD), indexing="ij")
    for isz in (4, 8):
        good = _wrap(None, b, t, c, isz)
        first_bad = {}
        for f in FAULTS:
            bad = _wrap(f, b, t, c, isz) != good
            assert bad.any(), f
            first_bad[f] = int(good[bad].min())
        assert first_bad["byte offset modulo 2^12"] == first_bad["byte offset sign-extended from 13 bits"] == 1 << 12
        assert first_bad["byte offset modulo 2^13"] == 1 << 13
        assert first_bad["element index modulo 2^11"] == (1 << 11) * isz
        assert first_bad["utterance base right, t * ld wrapped"] == -(-(1 << 12) // (LD * isz)) * LD * isz
