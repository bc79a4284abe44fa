"""GPU tests (-m gpu) of nnmk_f0_interp far from its pointers and past the grid's limit.

Far rows (tests/far.py): x, y and vuv are column slices of ONE parent of few rows and a huge row stride -- Tmax = 130 and
ld = 2064888, so that in float64 utterance b starts b * (2^31 - 128) bytes from the pointer and three utterances cross 2^31 and
2^32 bytes, and in float32 nine utterances reach 2^31 elements.  The columns sit at the start of the row and at its end.  After
each call FarParent.untouched() checks that every byte of the parent outside the columns the call may write is what it was: a
row offset that wrapped in 32 bits shows up as a stray write or a wrong value, not as a fault.

Grid limit: one batch of 2^24 + 3 utterances of one column -- more (utterance, column) pairs than the 2^24 - 1 workgroups of 256
threads one launch takes -- of which all but five have length 0: the launcher walks it in two slices, the live utterances on
either side of the seam come out as the model's, and every other frame of y and vuv is zero."""
import functools
import gc

import numpy as np
import pytest
import torch

import f0_cases as FC
import far
from f0_cases import F0
from far import FarParent

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
T, LD = 130, 2064888
BATCH = {F64: 3, F32: 9}
LENS = {3: [130, 67, 1], 9: [130, 67, 1, 130, 0, 65, 64, 129, 130]}
WANT = {F64: {"2^31 bytes", "2^32 bytes"}, F32: {"2^31 bytes", "2^32 bytes", "2^31 elements"}}
C = 2


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
def test_f0_interp_on_far_rows(dt):
    from nnmnkwii_amd import _f0_hip as FH
    B = BATCH[dt]
    lens = np.array(LENS[B], dtype=np.int32)
    rng = np.random.RandomState(50)
    X = np.full((B, T, C), np.nan)
    for b, n in enumerate(lens):
        for c in range(C):
            X[b, :n, c] = FC.runs(rng, n, (0.3, 0.7)[c])
    X = X.astype(dt)
    want_y, want_v = F0.batch(X, lens, "slinear")
    Ld = torch.from_numpy(lens).cuda()
    wide = FarParent((B, T, LD), dt, low_guard_bytes=far.low_guard_for(B * T * LD * np.dtype(dt).itemsize))
    n0 = FH.lib().nnmk_f0_launch_count()
    for cx, cy, cv, in_place in ((0, 512, 1024, False), (LD - 3 * C, LD - 2 * C, LD - C, False), (LD - C, LD - C, 7, True)):
        for b, n in enumerate(lens):
            if n:
                wide.place(b, int(n), cx, X[b, :n])
        for b in range(B):
            wide.expect_written(b, T, cy, C)
            wide.expect_written(b, T, cv, C)
        FH.interp(wide.cols(cx, C), Ld, FH.SLINEAR, wide.cols(cy, C), wide.cols(cv, C))
        torch.cuda.synchronize()
        got_y = np.stack([wide.read(b, T, cy, C) for b in range(B)])
        got_v = np.stack([wide.read(b, T, cv, C) for b in range(B)])
        assert FC.same_bits(got_y, want_y) and FC.same_bits(got_v, want_v), (cx, cy, cv)
        assert WANT[dt] <= wide.crossed(), wide.crossed()
        fails = wide.untouched()
        assert fails == [], (cx, cy, cv, in_place, fails)
        wide.forget()
    assert FH.lib().nnmk_f0_launch_count() == n0 + 3
    wide.free()


def test_a_batch_past_the_grid_limit_goes_in_slices():
    from nnmnkwii_amd import _f0_hip as FH
    limit = (1 << 24) - 1                       # max_workgroups(256)
    B, Tmax = limit + 4, 2
    live = {0: [0.0, 5.0], limit - 1: [5.5, -1e10], limit: [0.0, 4.5], limit + 1: [4.75, 5.25], B - 1: [-1e10, 6.0]}
    lengths = torch.zeros(B, dtype=torch.int32, device="cuda")
    x = torch.full((B, Tmax, 1), float("nan"), dtype=torch.float32, device="cuda")
    for b, track in live.items():
        lengths[b] = 2
        x[b, :, 0] = torch.tensor(track)
    y = torch.full((B, Tmax, 1), -7.0, dtype=torch.float32, device="cuda")
    v = torch.full((B, Tmax, 1), -7.0, dtype=torch.float32, device="cuda")
    n0 = FH.lib().nnmk_f0_launch_count()
    FH.interp(x, lengths, FH.SLINEAR, y, v)
    torch.cuda.synchronize()
    assert FH.lib().nnmk_f0_launch_count() == n0 + 1
    for b, track in live.items():
        t = np.array(track, dtype=np.float32)
        assert FC.same_bits(y[b, :, 0].cpu().numpy(), F0.literal(t)), b
        assert FC.same_bits(v[b, :, 0].cpu().numpy(), F0.vuv(t)), b
        y[b].zero_()
        v[b].zero_()
    assert not bool(y.any().item()) and not bool(v.any().item())
    assert bool((y.view(torch.int32) == 0).all().item()) and bool((v.view(torch.int32) == 0).all().item())   # (+0.0: no -0.0)
