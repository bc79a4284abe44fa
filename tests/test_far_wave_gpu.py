"""GPU tests (-m gpu) of nnmk_wave_encode and nnmk_wave_decode far from their pointers and past the grid's limit.

Far utterances (tests/far.py): x and y are sample ranges of ONE parent of few utterances and a huge utterance stride --
ld = 2^28 - 16 samples, so that in float64 utterance b starts b * (2^31 - 128) bytes from the pointer and three utterances cross
2^31 and 2^32 bytes, and in float32 nine utterances reach 2^31 elements.  The samples sit at the start of the utterance's stride
and at its end.  After each call FarParent.untouched() checks that every byte of the parent outside what the call may write is
what it was: an offset that wrapped in 32 bits shows up as a stray write or a wrong value, not as a fault.

Grid limit: one batch of 2^24 + 3 utterances of two samples -- more workgroups than the 2^24 - 1 of 256 threads one launch takes
-- of which all but five have length 0: both launchers walk it in two slices, the live utterances on either side of the seam
come out as the model's, and every other sample is the padding value."""
import functools
import gc

import numpy as np
import pytest
import torch

import far
import wave_cases as WC
from far import FarParent
from wave_cases import WM

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
LD, LMAX = (1 << 28) - 16, 2500
BATCH = {F64: 3, F32: 9}
LENS = {3: [2500, 1025, 1], 9: [2500, 1025, 1, 2500, 0, 1024, 2049, 3, 2500]}
WANT = {F64: {"2^31 bytes", "2^32 bytes"}, F32: {"2^31 bytes", "2^32 bytes", "2^31 elements"}}


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
def test_encode_and_decode_on_far_utterances(dt):
    from nnmnkwii_amd import _wave_hip as WH
    B = BATCH[dt]
    lens = np.array(LENS[B], dtype=np.int32)
    rng = np.random.RandomState(51)
    X = np.full((B, LMAX), np.nan)
    for b, n in enumerate(lens):
        X[b, :n] = WC.wave(rng, n)
    X = X.astype(dt)
    want_enc = WM.encode_batch(X, lens, 0.97, WM.PLAIN, 256, dt)
    want_dec = WM.decode_batch(X, lens, WM.PLAIN, 256, 0.5, 1024, dt)
    Ld = torch.from_numpy(lens).cuda()
    wide = FarParent((B, 1, LD), dt, low_guard_bytes=far.low_guard_for(B * LD * np.dtype(dt).itemsize))
    n0 = WH.lib().nnmk_wave_launch_count()
    for cx, cy in ((0, 4096), (LD - 2 * LMAX - 8, LD - LMAX)):
        for op, want in (("encode", want_enc), ("decode", want_dec)):
            for b, n in enumerate(lens):
                if n:
                    wide.place(b, 1, cx, X[b:b + 1, :n])
            for b in range(B):
                wide.expect_written(b, 1, cy, LMAX)
            xs, ys = wide.cols(cx, LMAX)[:, 0, :], wide.cols(cy, LMAX)[:, 0, :]
            if op == "encode":
                WH.encode(xs, Ld, 0.97, WH.PLAIN, 256, ys)
            else:
                WH.decode(xs, Ld, WH.PLAIN, 256, None, 0.5, 1024, ys)
            torch.cuda.synchronize()
            got = np.concatenate([wide.read(b, 1, cy, LMAX) for b in range(B)])
            assert WC.same_bits(got, want), (op, cx, cy)
            assert WANT[dt] <= wide.crossed(), wide.crossed()
            fails = wide.untouched()
            assert fails == [], (op, cx, cy, fails)
            wide.forget()
    assert WH.lib().nnmk_wave_launch_count() == n0 + 4
    wide.free()


def test_a_batch_past_the_grid_limit_goes_in_slices():
    from nnmnkwii_amd import _wave_hip as WH
    limit = (1 << 24) - 1                       # max_workgroups(256)
    B, Lmax = limit + 4, 2
    live = {0: [0.25, -0.5], limit - 1: [0.5, 0.125], limit: [-0.75, 0.5], limit + 1: [0.0625, 0.25], B - 1: [-0.5, 1.0]}
    lengths = torch.zeros(B, dtype=torch.int32, device="cuda")
    x = torch.full((B, Lmax), float("nan"), dtype=torch.float32, device="cuda")
    for b, track in live.items():
        lengths[b] = 2
        x[b] = torch.tensor(track)
    c = torch.full((B, Lmax), 7, dtype=torch.uint8, device="cuda")
    y = torch.full((B, Lmax), -7.0, dtype=torch.float32, device="cuda")
    n0 = WH.lib().nnmk_wave_launch_count()
    WH.encode(x, lengths, 0.97, WH.QUANTIZE, 255, c)
    WH.decode(x, lengths, WH.PLAIN, 256, None, 0.97, 0, y)
    torch.cuda.synchronize()
    assert WH.lib().nnmk_wave_launch_count() == n0 + 2
    for b, track in live.items():
        t = np.array(track, dtype=np.float32)
        assert np.array_equal(c[b].cpu().numpy(), WM.encode(t, 0.97, WM.QUANTIZE, 255, np.uint8)), b
        assert WC.same_bits(y[b].cpu().numpy(), WM.decode(t, WM.PLAIN, coef=0.97, segment=0, dtype=np.float32, Lmax=2)), b
        c[b] = 127
        y[b].zero_()
    assert bool((c == 127).all().item()) and bool((y.view(torch.int32) == 0).all().item())
