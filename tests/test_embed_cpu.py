"""tests/embed.py on CPU tensors (-m "not gpu"): a guard that cannot fail is worth nothing, so every check of the harness is made
to fail here by the smallest write that must trip it -- one byte just before the payload, one just behind it, one at the far end
of either guard, one into an input -- and the payload pointer is checked for the residue the caller asked for."""
import numpy as np
import pytest
import torch

from embed import Embedded, Workspace, embedded, failed

DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint8]


def _flip(b, pos):
    b.raw[pos] = (b.fill ^ 0xFF)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [0, 1, 2, 3, 4])
def test_payload_pointer_shape_and_residue(dtype, off):
    isz = np.dtype(dtype).itemsize
    b = Embedded((3, 5), dtype, off, 0x5A, device="cpu")
    p = b.payload()
    assert p.shape == (3, 5) and p.is_contiguous() and p.data_ptr() == b.ptr()
    assert b.ptr() % 256 == (off * isz) % 256 and b.ptr() % 16 == (off * isz) % 16
    assert b.lo == 4096 + off * isz and b.raw.numel() - b.hi >= 4096
    assert b.guards_ok()
    assert bool((b.raw == 0x5A).all())                              # the payload starts out as the fill byte too
    a = (np.arange(15).reshape(3, 5) % 7).astype(dtype)
    b.put(a)
    assert np.array_equal(b.host(), a) and b.host().dtype == np.dtype(dtype)
    assert b.guards_ok() and b.unchanged()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["just before", "just behind", "first byte of the front guard", "last byte of the rear guard"])
def test_one_byte_in_a_guard_is_seen(dtype, where):
    b = Embedded((7,), dtype, 1, 0xA5, device="cpu").put(np.arange(7))
    assert b.guards_ok()
    pos = {"just before": b.lo - 1, "just behind": b.hi, "first byte of the front guard": 0,
           "last byte of the rear guard": b.raw.numel() - 1}[where]
    _flip(b, pos)
    assert not b.guards_ok()
    assert b.unchanged()                                            # the payload itself was not touched
    b.raw[pos] = b.fill
    assert b.guards_ok()


def test_a_write_of_the_fill_byte_into_the_payload_does_not_trip_the_guards_but_a_changed_input_is_seen():
    b = Embedded((4, 2), np.float64, 1, 0xA5, device="cpu").put(np.arange(8.0))
    assert b.unchanged()
    b.payload()[3, 1] = np.nextafter(7.0, 8.0)                      # one bit of the last element
    assert not b.unchanged() and b.guards_ok()
    b.payload()[3, 1] = 7.0
    assert b.unchanged()
    b.bytes_view()[0] ^= 1                                          # one bit of the first byte
    assert not b.unchanged()
    # -0.0 for 0.0 compares equal as a number and is still a change
    z = embedded(np.zeros(3), device="cpu")
    z.payload()[1] = -0.0
    assert not z.unchanged()
    with pytest.raises(AssertionError):
        Embedded((2,), np.int32, device="cpu").unchanged()          # no snapshot taken


def test_outputs_start_as_the_fill_and_refill_restores_it():
    b = Embedded((5,), np.int32, 1, 0xFF, device="cpu")
    assert np.array_equal(b.host(), np.full(5, -1, dtype=np.int32))
    b.payload().zero_()
    b.refill()
    assert np.array_equal(b.host(), np.full(5, -1, dtype=np.int32)) and b.guards_ok()
    assert embedded(None) is None
    e = Embedded((0, 3), np.float32, 1, device="cpu")               # an empty payload: the two guards touch
    assert e.payload().shape == (0, 3) and e.guards_ok()


@pytest.mark.parametrize("align", [8, 128])
@pytest.mark.parametrize("nbytes", [0, 8, 256, 1000, 4096])
def test_workspace_is_exact_aligned_and_never_256_aligned(align, nbytes):
    w = Workspace(nbytes, align, 0xA5, device="cpu")
    assert w.nbytes == nbytes and w.bytes_view().numel() == nbytes
    assert w.ptr() % align == 0 and w.ptr() % 256 == align
    assert w.guards_ok()
    w.zero()
    assert w.guards_ok() and (nbytes == 0 or not w.bytes_view().any())
    for pos in (w.lo - 1, w.hi, 0, w.raw.numel() - 1):
        _flip(w, pos)
        assert not w.guards_ok()
        w.raw[pos] = w.fill
    assert w.guards_ok()
    if nbytes:
        w.snapshot()
        w.bytes_view()[nbytes - 1] = 1
        assert not w.unchanged() and w.guards_ok()


def test_torch_dtypes_are_accepted_and_others_refused():
    assert Embedded((2,), torch.float64, device="cpu").payload().dtype == torch.float64
    with pytest.raises(AssertionError):
        Embedded((2,), np.float16, device="cpu")


def test_failed_names_exactly_the_buffers_that_were_hit():
    ins = dict(x=embedded(np.arange(4.0), 1, device="cpu"), lengths=None, y=embedded(np.arange(3), 0, device="cpu"))
    outs = dict(out=Embedded((2, 2), np.float32, device="cpu"), status=Embedded((2,), np.int32, 1, device="cpu"))
    works = dict(ws=Workspace(40, 8, device="cpu"))
    assert failed(ins, outs, works) == [] and failed() == []
    ins["x"].payload()[0] = 9.0
    _flip(ins["y"], ins["y"].hi)
    _flip(outs["status"], outs["status"].lo - 1)
    _flip(works["ws"], works["ws"].hi)
    outs["out"].payload().zero_()                                   # writing an output is what outputs are for
    assert failed(ins, outs, works) == ["input x changed", "guard of input y", "guard of output status", "guard of workspace ws"]
