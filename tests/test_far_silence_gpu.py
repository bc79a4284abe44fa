"""GPU tests (-m gpu) of nnmk_sil_expand / nnmk_sil_gather far from their pointers (tests/far.py).

Far sources: the phone matrix and the gather's source are column slices of ONE parent of few rows and a huge row stride --
130 rows and ld = 2064888, so that in float64 utterance b starts b * (2^31 - 128) bytes from the pointer and three utterances cross
2^31 and 2^32 bytes, and in float32 nine utterances reach 2^31 elements.  The columns sit at the start of the row and at its end.
Phone rows at or past num_phones and source rows at or past len_src hold the parent's fill byte and are never read; the rows equal
tools/silence_model.py bit for bit.

Far output: five kept rows go to a column slice of a parent of five rows whose stride (2^27 + 24 elements of float64, 2^29 + 24
of float32) puts row 4 past 2^32 bytes, and in float32 past 2^31 elements, from the pointer.

After each call FarParent.untouched() checks that every byte of the parent outside the columns the call may write is what it
was: a row offset that wrapped in 32 bits shows up as a stray write or a wrong value, not as a fault.

Grid limit: a batch of exactly as many output blocks as one grid takes runs and is correct; one block more is refused with its
text (include/nnmnkwii_silence.h: the entries refuse, they do not slice) and nothing is launched."""
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

import far
import silence_cases as SC
from far import FarParent
from silence_cases import FM, SM

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TORCH_DT = {F32: torch.float32, F64: torch.float64}
T, LD = 130, 2064888
BATCH = {F64: 3, F32: 9}
PHONES = {3: [130, 67, 3], 9: [130, 67, 1, 130, 0, 65, 64, 129, 130]}
LENS = {3: [130, 70, 0], 9: [130, 70, 0, 128, 2, 65, 64, 130, 130]}
WANT = {F64: {"2^31 bytes", "2^32 bytes"}, F32: {"2^31 bytes", "2^32 bytes", "2^31 elements"}}
LD_OUT = {F64: (1 << 27) + 24, F32: (1 << 29) + 24}
DL, D = 3, 2


def far_test(fn):
    """Peak device memory of the test stays under far.MEM_CAP; whatever it allocated is handed back at its end."""
    @functools.wraps(fn)
    def run(*a, **kw):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        try:
            fn(*a, **kw)
            peak = torch.cuda.max_memory_allocated()
        finally:
            gc.collect()
            torch.cuda.empty_cache()
        assert peak <= far.MEM_CAP, "peak device memory %.2f GiB" % (peak / 2.0 ** 30)
    return run


@pytest.mark.parametrize("dt", [F64, F32], ids=["float64", "float32"])
@far_test
def test_rows_from_far_sources(dt):
    from nnmnkwii_amd import _silence_hip as SH
    B = BATCH[dt]
    n, lens = np.array(PHONES[B], dtype=np.int32), np.array(LENS[B], dtype=np.int32)
    rng = np.random.RandomState(61)
    r = rng.choice([0, 1, 1, 1, 2], size=(B, T, 1)).astype(np.int64)          # about one frame per phone: T_b near num_phones
    sil = (rng.rand(B, T) < 0.3).astype(np.uint8)
    sil[0, 0], sil[0, T - 1], r[0, T - 1, 0] = 1, 0, 2                         # the first phone flagged, the last row of all read
    P = (np.round(rng.randn(B, T, DL) * 4) / 4).astype(dt)
    Y = SC.source(61, B, T, D, lens, dt)
    want, want_len, _ = SM.kept_frame_features_batch(P, r, sil, n, "full", 0, dtype=F64)
    gwant, gwant_len, _ = SM.remove_silence_frames_batch(Y, r, sil, lens, n, 0, T, F64)
    assert want_len[0] > 64 and gwant_len[0] > 64 and (gwant_len < lens).any()
    d, nt, st, lt = (torch.from_numpy(a).cuda() for a in (r, n, sil, lens))
    wide = FarParent((B, T, LD), dt, low_guard_bytes=far.low_guard_for(B * T * LD * np.dtype(dt).itemsize))
    n0 = SC.launches()
    for cp, cy in ((0, 512), (LD - DL - D, LD - D)):
        for b in range(B):
            if n[b]:
                wide.place(b, int(n[b]), cp, P[b, :n[b]])
            if lens[b]:
                wide.place(b, int(lens[b]), cy, Y[b, :lens[b]])
        out = torch.full((B, want.shape[1] + 2, DL + 9), -7.0, dtype=torch.float64, device="cuda")
        gout = torch.full((B, T, D), -7.0, dtype=torch.float64, device="cuda")
        lengths = SH.expand(wide.cols(cp, DL), d, nt, st, FM.FULL, 0, None, None, None, out)
        glengths = SH.gather(wide.cols(cy, D), lt, d, nt, st, 0, gout)
        torch.cuda.synchronize()
        assert np.array_equal(lengths.cpu().numpy(), want_len) and np.array_equal(glengths.cpu().numpy(), gwant_len), (cp, cy)
        got = out.cpu().numpy()
        assert SC.same_bits(got[:, :want.shape[1]], want) and not got[:, want.shape[1]:].any(), (cp, cy)
        assert SC.same_bits(gout.cpu().numpy(), gwant), (cp, cy)
        assert WANT[dt] <= wide.crossed(), wide.crossed()
        fails = wide.untouched()
        assert fails == [], (cp, cy, fails)
        wide.forget()
    assert SC.launches() == n0 + 4
    wide.free()


@pytest.mark.parametrize("dt", [F64, F32], ids=["float64", "float32"])
@far_test
def test_five_rows_into_a_far_output(dt):
    from nnmnkwii_amd import _silence_hip as SH
    rng = np.random.RandomState(62)
    r = np.array([[[1, 0, 1], [0, 2, 0], [1, 1, 1]]], dtype=np.int64)          # 7 frames, the middle phone's 2 flagged
    sil = np.array([[0, 1, 0]], dtype=np.uint8)
    P = np.round(rng.randn(1, 3, DL) * 4) / 4
    W = DL + 9
    Y = rng.randn(1, 7, W)
    want, want_len, _ = SM.kept_frame_features_batch(P, r, sil, None, "full", 0, dtype=dt)
    gwant, gwant_len, _ = SM.remove_silence_frames_batch(Y, r, sil, None, None, 0, 5, dt)
    assert want.shape == (1, 5, W) and list(want_len) == [5] == list(gwant_len)
    ld = LD_OUT[dt]
    wide = FarParent((1, 5, ld), dt, low_guard_bytes=far.low_guard_for(5 * ld * np.dtype(dt).itemsize))
    Pt, Yt, d, st = (torch.from_numpy(a).cuda() for a in (P, Y, r, sil))
    for c0 in (0, ld - W):
        for entry, expect in ((lambda o: SH.expand(Pt, d, None, st, FM.FULL, 0, None, None, None, o), want),
                              (lambda o: SH.gather(Yt, None, d, None, st, 0, o), gwant)):
            wide.expect_written(0, 5, c0, W)
            lengths = entry(wide.cols(c0, W))
            torch.cuda.synchronize()
            assert list(lengths.cpu().numpy()) == [5]
            assert SC.same_bits(wide.read(0, 5, c0, W), expect[0]), c0
            assert WANT[dt] <= wide.crossed(), wide.crossed()
            fails = wide.untouched()
            assert fails == [], (c0, fails)
            wide.forget()
    wide.free()


def test_as_many_blocks_as_one_grid_takes_and_one_more():
    """2^24 - 1 utterances of one output block each run in one launch and are correct; one utterance more is refused with its
    text, nothing is launched and no output byte is written."""
    from nnmnkwii_amd import _silence_hip as SH
    L = SH.lib()
    limit = (1 << 24) - 1
    B = limit + 1
    idx = torch.arange(B, device="cuda")
    P = (idx % 1000).to(torch.float32).view(B, 1, 1)
    d = (1 + idx % 2).to(torch.int32).view(B, 1, 1)                            # 1 or 2 frames
    sil = (idx % 3 == 0).view(B, 1)
    out = torch.full((B, 2, 1), -7.0, dtype=torch.float32, device="cuda")
    lengths = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n0 = SC.launches()
    args = lambda Bn: (0, None, 0, vp(P), 1, 2, vp(d), None, vp(sil), Bn, 1, 1, 1, 0, 0, None, None, None, 0, vp(out), 1, 2, vp(lengths))  # noqa: E731
    assert L.nnmk_sil_expand(*args(B)) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    gargs = lambda Bn: (0, None, 2, vp(d), None, vp(sil), Bn, 1, 1, 0, 0, vp(P), 1, None, 1, 1, 0, vp(out), 1, 2, vp(lengths))  # noqa: E731
    assert L.nnmk_sil_gather(*gargs(B)) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert SC.launches() == n0 and bool((out == -7.0).all().item()) and bool((lengths == -7).all().item())
    assert L.nnmk_sil_expand(*args(limit)) == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    keep = ~sil[:limit, 0]
    frames = torch.where(keep, d[:limit, 0, 0], torch.zeros_like(d[:limit, 0, 0]))
    assert SC.launches() == n0 + 1 and bool((lengths[:limit] == frames).all().item()) and int(lengths[limit].item()) == -7
    rows = torch.arange(2, device="cuda").view(1, 2)
    want = torch.where(rows < frames.view(-1, 1), P[:limit, 0], torch.zeros_like(P[:limit, 0]))
    assert bool((out[:limit, :, 0] == want).all().item()) and bool((out[limit] == -7.0).all().item())
    # the gather at the limit: one source row each, dropped where the phone is flagged
    out.fill_(-7.0)
    assert L.nnmk_sil_gather(*gargs(limit)) == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert bool((lengths[:limit] == keep.to(torch.int32)).all().item())
    gwant = torch.stack([torch.where(keep, P[:limit, 0, 0], torch.zeros_like(P[:limit, 0, 0])), torch.zeros(limit, device="cuda")], 1)
    assert bool((out[:limit, :, 0] == gwant).all().item()) and bool((out[limit] == -7.0).all().item())
