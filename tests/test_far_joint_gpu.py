"""GPU tests (-m gpu) of nnmk_joint_count / nnmk_joint_write far from their pointers (tests/far.py).

Far sources: x and y are column slices of ONE parent of few rows and a huge row stride -- Tmax = 130 and ld = 2064888, so that in
float64 utterance b starts b * (2^31 - 128) bytes from the pointer and three utterances cross 2^31 and 2^32 bytes, and in float32
nine utterances reach 2^31 elements.  The columns sit at the start of the row and at its end.  The rows at or past a length hold
the parent's fill byte and are never read; the kept rows equal tools/joint_model.py bit for bit.

Far output: five kept rows go to a column slice of a parent of five rows whose stride ld_out (2^27 + 24 elements of float64,
2^29 + 24 of float32) puts row 4 past 2^32 bytes, and in float32 past 2^31 elements, from the pointer.

After each call FarParent.untouched() checks that every byte of the parent outside the columns the call may write is what it
was: a row offset that wrapped in 32 bits shows up as a stray write or a wrong value, not as a fault.

Grid limit: one batch of more tiles than a launch takes workgroups, see test_more_tiles_than_one_grid_takes_go_in_slices."""
import functools
import gc

import numpy as np
import pytest
import torch

import far
import joint_cases as JC
from far import FarParent
from joint_cases import JM

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TORCH_DT = {F32: torch.float32, F64: torch.float64}
T, LD = 130, 2064888
BATCH = {F64: 3, F32: 9}
LENS = {3: ([130, 67, 3], [130, 70, 0]), 9: ([130, 67, 1, 130, 0, 65, 64, 129, 130], [130, 70, 0, 128, 2, 65, 64, 130, 130])}
WANT = {F64: {"2^31 bytes", "2^32 bytes"}, F32: {"2^31 bytes", "2^32 bytes", "2^31 elements"}}
LD_OUT = {F64: (1 << 27) + 24, F32: (1 << 29) + 24}
DX, DY = 3, 2


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
def test_joint_rows_from_far_sources(dt):
    from nnmnkwii_amd import _joint_hip as JH
    B = BATCH[dt]
    lx, ly = (np.array(n, dtype=np.int32) for n in LENS[B])
    rng = np.random.RandomState(51)
    X, Y = JC.frames(rng, B, T, DX).astype(dt), JC.frames(rng, B, T, DY).astype(dt)
    for b, t in ((0, 0), (0, 63), (0, 64), (1, 30), (B - 1, 129)):
        X[b, t] = 0.0
        Y[b, t] = 0.0
    want, want_offs = JM.literal(X, Y, lx, ly, JC.W3, JM.NONZERO, 1e-7, F64)
    lxt, lyt = torch.from_numpy(lx).cuda(), torch.from_numpy(ly).cuda()
    wide = FarParent((B, T, LD), dt, low_guard_bytes=far.low_guard_for(B * T * LD * np.dtype(dt).itemsize))
    n0 = JH.lib().nnmk_joint_launch_count()
    for cx, cy in ((0, 512), (LD - DX - DY, LD - DY)):
        for b in range(B):
            if lx[b]:
                wide.place(b, int(lx[b]), cx, X[b, :lx[b]])
            if ly[b]:
                wide.place(b, int(ly[b]), cy, Y[b, :ly[b]])
        out = torch.full((len(want) + 2, want.shape[1]), -7.0, dtype=torch.float64, device="cuda")
        plan, offsets = JH.count(wide.cols(cx, DX), wide.cols(cy, DY), lxt, lyt, JC.W3, JH.NONZERO, 1e-7, torch.float64)
        plan.write(out)
        torch.cuda.synchronize()
        assert JC.same_bits(offsets.cpu().numpy(), want_offs), (cx, cy)
        got = out.cpu().numpy()
        assert JC.same_bits(got[:len(want)], want) and (got[len(want):] == -7.0).all(), (cx, cy)
        assert WANT[dt] <= wide.crossed(), wide.crossed()
        fails = wide.untouched()
        assert fails == [], (cx, cy, fails)
        wide.forget()
    assert JH.lib().nnmk_joint_launch_count() == n0 + 4
    wide.free()


@pytest.mark.parametrize("dt", [F64, F32], ids=["float64", "float32"])
@far_test
def test_five_rows_into_a_far_output(dt):
    from nnmnkwii_amd import _joint_hip as JH
    rng = np.random.RandomState(52)
    X = JC.frames(rng, 2, 5, DX)
    X[0, 1] = X[0, 2] = X[0, 3] = 0.0                      # frame 2 alone has zero statics AND zero deltas; utterance 1 has one live frame
    lx = np.array([5, 1], dtype=np.int32)
    want, want_offs = JM.literal(X, None, lx, None, JC.W3, JM.NONZERO, 1e-7, dt)
    W = want.shape[1]
    assert want.shape == (5, 9) and want_offs.tolist() == [0, 4, 5] and not want[1, :DX].any()
    ld = LD_OUT[dt]
    wide = FarParent((1, 5, ld), dt, low_guard_bytes=far.low_guard_for(5 * ld * np.dtype(dt).itemsize))
    Xt, lxt = torch.from_numpy(X).cuda(), torch.from_numpy(lx).cuda()
    for c0 in (0, ld - W):
        wide.expect_written(0, 5, c0, W)
        plan, offsets = JH.count(Xt, None, lxt, None, JC.W3, JH.NONZERO, 1e-7, TORCH_DT[dt])
        plan.write(wide.cols(c0, W)[0])
        torch.cuda.synchronize()
        assert JC.same_bits(offsets.cpu().numpy(), want_offs)
        assert JC.same_bits(wide.read(0, 5, c0, W), want), c0
        assert WANT[dt] <= wide.crossed(), wide.crossed()
        fails = wide.untouched()
        assert fails == [], (c0, fails)
        wide.forget()
    wide.free()


def test_more_tiles_than_one_grid_takes_go_in_slices():
    """2^24 + 3 utterances of one tile each -- more than the 2^24 - 1 workgroups of 256 threads one launch takes -- of which all
    but five have length 0: both tiled stages walk them in two slices, the scan carries across all of them, and the live
    utterances on either side of the seam come out in order.  Each call still counts once."""
    from nnmnkwii_amd import _joint_hip as JH
    limit = (1 << 24) - 1                       # max_workgroups(256)
    B, Tmax = limit + 4, 2
    live = {0: [0.0, 5.0], limit - 1: [5.5, -1e10], limit: [0.0, 4.5], limit + 1: [4.75, 5.25], B - 1: [-1e10, 6.0]}
    lengths = torch.zeros(B, dtype=torch.int32, device="cuda")
    x = torch.full((B, Tmax, 1), float("nan"), dtype=torch.float32, device="cuda")
    for b, frames in live.items():
        lengths[b] = 2
        x[b, :, 0] = torch.tensor(frames)
    want = [v for b in sorted(live) for v in live[b] if v != 0.0]
    out = torch.full((len(want) + 3, 1), -7.0, dtype=torch.float32, device="cuda")
    n0 = JH.lib().nnmk_joint_launch_count()
    plan, offsets = JH.count(x, None, lengths, None, [], JH.NONZERO, 1e-7, torch.float32)
    plan.write(out)
    torch.cuda.synchronize()
    assert JH.lib().nnmk_joint_launch_count() == n0 + 2
    assert JC.same_bits(out[:, 0].cpu().numpy(), np.array(want + [-7.0] * 3, dtype=np.float32))
    offs = offsets.cpu().numpy()
    assert offs[-1] == len(want) == 8 and [int(offs[b]) for b in sorted(live)] == [0, 1, 3, 4, 6] and (np.diff(offs) >= 0).all()
    assert int(offs[limit - 1]) == 1 and int(offs[limit + 2]) == 6 and int(offs[B - 1]) == 6
