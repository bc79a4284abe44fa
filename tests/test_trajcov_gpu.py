"""GPU tests (-m gpu) of nnmk_traj_covariance (csrc/mlpg_trajcov.hip) against tools/trajcov_model.py: the band BIT
FOR BIT (it is made of + - x / alone, and the kernel is compiled without contraction), logdet within (T + 4) 2^-53 sum |log D_t|
(the sequential sum plus log's last place), the padding rows, a planted non-positive pivot, the forward sweep alone, the same
bits under a permutation of the batch and on a repeated call, and the refusals.  Shapes: the lengths around the edge rule (1 .. 5)
and around a wavefront's worth of frames, static dims around the lane and wavefront boundaries."""
import numpy as np
import pytest
import torch

import trajcov_cases as C
from trajcov_cases import TM

pytestmark = pytest.mark.gpu
DT = {np.float32: torch.float32, np.float64: torch.float64}


def device_inputs(var, lengths):
    v = None if var is None else torch.from_numpy(var).cuda()
    L = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
    return v, L


def run(var, wname, lengths, B, Tmax, sd, dtype, **kw):
    from nnmnkwii_amd import _trajectory_calls as TC
    v, L = device_inputs(var, lengths)
    nw = len(C.WINDOWS[wname])
    band, logdet, status = TC.covariance(v, C.WINDOWS[wname], L, B, Tmax, nw * sd, dtype=DT[dtype], device=torch.device("cuda", 0), **kw)
    torch.cuda.synchronize()
    return (None if band is None else band.cpu().numpy()), logdet.cpu().numpy(), status.cpu().numpy()


def check(var, wname, lengths, B, Tmax, sd, dtype):
    band, logdet, status = run(var, wname, lengths, B, Tmax, sd, dtype)
    mband, mlogdet, mstatus = TM.covariance_batch(var, C.WINDOWS[wname], lengths, B, Tmax, sd)
    assert np.array_equal(status, mstatus) and not status.any()
    assert C.same_bits(band, mband), (wname, np.abs(band - mband).max())          # the live rows AND the zeros at or past T
    live = TM.live_frames(lengths, B, Tmax)
    for b in range(B):
        v = None if var is None else (var if var.ndim == 1 else var[b])
        bound = C.logdet_bound(v, wname, int(live[b]), sd)
        err = np.abs(logdet[b] - mlogdet[b])
        print("logdet: worst %.3g of the bound" % (err / np.maximum(bound, 1e-300)).max() if live[b] else "empty utterance")
        assert (err <= bound).all(), (b, err.max(), bound.min())
    return band, logdet


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sd", [1, 3, 60, 64, 65, 130])
def test_static_dims_across_lane_and_wavefront_boundaries(sd, dtype):
    for i, (wname, mode) in enumerate([("std3", TM.VAR_FRAME), ("std2", TM.VAR_GLOBAL), ("asym", TM.VAR_FRAME)]):
        B, Tmax, lengths = (3, 9, [9, 0, 4]) if i != 1 else (1, 5, None)
        check(C.variances(sd + i, B, Tmax, sd, wname, mode, dtype), wname, lengths, B, Tmax, sd, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 63, 64, 65])
def test_lengths_around_the_edge_rule_and_the_ring(T, dtype):
    for i, wname in enumerate(C.WINDOWS):
        for mode in C.MODES:
            lengths = [T, 0, max(T - 1, 0)]
            check(C.variances(T + i, 3, T, 3, wname, mode, dtype), wname, lengths, 3, T, 3, dtype)
    check(C.variances(T, 1, T, 3, "std3", TM.VAR_FRAME, dtype, tight=True), "std3", None, 1, T, 3, dtype)


def test_non_positive_pivot_names_the_frame_and_spares_the_neighbours():
    from nnmnkwii_amd import paramgen
    B, Tmax, sd, lengths = 2, 9, 3, [9, 6]
    var = C.variances(5, B, Tmax, sd, "std3", TM.VAR_FRAME)
    var[0, 5, 1] = -1e-3
    band, logdet, status = run(var, "std3", lengths, B, Tmax, sd, np.float64)
    mband, mlogdet, mstatus = TM.covariance_batch(var, C.WINDOWS["std3"], lengths, B, Tmax, sd)
    assert np.array_equal(status, mstatus) and status[0, 1] == 6 and status.sum() == 6
    assert np.isnan(band[:, 0, :, 1]).all() and np.isnan(logdet[0, 1])
    assert C.same_bits(band, mband)                                               # the neighbours bit for bit, the pad rows zero
    with pytest.raises(np.linalg.LinAlgError, match=r"6-th leading minor not positive definite \(utterance 0, dim 1, frame 5\)"):
        paramgen.mlpg_covariance_batch(var, C.WINDOWS["std3"], lengths)
    with pytest.raises(np.linalg.LinAlgError):
        paramgen.mlpg_variance(var[0], C.WINDOWS["std3"])


def test_forward_sweep_alone_gives_the_same_logdet_bits():
    B, Tmax, sd, lengths = 3, 65, 65, [65, 0, 17]
    var = C.variances(1, B, Tmax, sd, "std3", TM.VAR_FRAME)
    band, logdet, _ = run(var, "std3", lengths, B, Tmax, sd, np.float64)
    none, logdet2, status2 = run(var, "std3", lengths, B, Tmax, sd, np.float64, want_band=False)
    assert none is None and C.same_bits(logdet, logdet2) and not status2.any()


def test_same_bits_when_the_batch_is_permuted_or_the_call_repeated():
    B, Tmax, sd, lengths = 3, 17, 5, [17, 3, 9]
    var = C.variances(2, B, Tmax, sd, "std3", TM.VAR_FRAME)
    band, logdet, _ = run(var, "std3", lengths, B, Tmax, sd, np.float64)
    again = run(var, "std3", lengths, B, Tmax, sd, np.float64)
    assert C.same_bits(band, again[0]) and C.same_bits(logdet, again[1])
    perm = [2, 0, 1]
    pb, pl, _ = run(np.ascontiguousarray(var[perm]), "std3", [lengths[i] for i in perm], B, Tmax, sd, np.float64)
    assert C.same_bits(pb, np.ascontiguousarray(band[:, perm])) and C.same_bits(pl, np.ascontiguousarray(logdet[perm]))
    # a system's bits do not depend on the padding either
    wide = np.concatenate([var, np.full((B, 4, var.shape[2]), np.nan)], axis=1)
    wb, wl, _ = run(wide, "std3", lengths, B, Tmax + 4, sd, np.float64)
    assert C.same_bits(np.ascontiguousarray(wb[:, :, :Tmax]), band) and (wb[:, :, Tmax:] == 0).all() and C.same_bits(wl, logdet)


def test_refusals_launch_nothing_and_leave_out_alone():
    from nnmnkwii_amd import _hip, _trajectory_calls as TC, _trajectory_hip as TH
    L = TH.lib()
    var = torch.from_numpy(C.variances(1, 2, 9, 3, "std3", TM.VAR_FRAME)).cuda()
    out = torch.full((3, 2, 9, 3), -7.0, dtype=torch.float64, device="cuda")
    n0 = L.nnmk_traj_launch_count()
    wide = [(0, 0, np.array([1.0])), (2, 2, np.array([1.0, -8.0, 0.0, 8.0, -1.0]) / 12)]
    with pytest.raises(_hip.HipExtensionError, match="extents"):
        TC.covariance(var[:, :, :6], wide, None, 2, 9, 6, band=torch.full((5, 2, 9, 3), -7.0, dtype=torch.float64, device="cuda"))
    with pytest.raises(_hip.HipExtensionError, match="overlap"):
        TC.covariance(var, C.WINDOWS["std3"], None, 2, 9, 9, band=var.view(-1)[:162].view(3, 2, 9, 3))
    with pytest.raises(ValueError):
        TC.covariance(var, C.WINDOWS["std3"], None, 2, 9, 9, band=out[:2])
    torch.cuda.synchronize()
    assert L.nnmk_traj_launch_count() == n0 and (out == -7).all()
    TC.covariance(var, C.WINDOWS["std3"], None, 2, 9, 9, band=out)
    torch.cuda.synchronize()
    assert L.nnmk_traj_launch_count() == n0 + 1 and not (out == -7).any()


def test_paramgen_numpy_and_tensor_interfaces():
    from nnmnkwii_amd import paramgen
    win = C.WINDOWS["std3"]
    var = C.variances(9, 2, 9, 3, "std3", TM.VAR_FRAME, np.float32)
    mband, mlogdet, _ = TM.covariance_batch(var, win, [9, 4], 2, 9, 3)
    band, logdet = paramgen.mlpg_covariance_batch(var, win, [9, 4])
    assert isinstance(band, np.ndarray) and C.same_bits(band, mband) and np.allclose(logdet, mlogdet, rtol=0, atol=1e-12)
    tb, tl = paramgen.mlpg_covariance_batch(torch.from_numpy(var).cuda(), win, [9, 4])
    assert tb.is_cuda and tb.dtype == torch.float64 and C.same_bits(tb.cpu().numpy(), mband)
    assert paramgen.mlpg_covariance_batch(var, win, [9, 4], band=False)[0] is None
    assert C.same_bits(paramgen.mlpg_variance(var[0], win), mband[0, 0])
    assert np.allclose(paramgen.mlpg_logdet(var[0], win), mlogdet[0], rtol=0, atol=1e-12)
    # global and unit variances are read in place: the batch shape comes from lengths / B / Tmax
    g = C.variances(3, 1, 1, 3, "std3", TM.VAR_GLOBAL)
    gb, gl = paramgen.mlpg_covariance_batch(g, win, [7, 2], Tmax=8)
    assert C.same_bits(gb, TM.covariance_batch(g, win, [7, 2], 2, 8, 3)[0])
    ub, ul = paramgen.mlpg_covariance_batch(None, win, B=1, Tmax=6)
    assert ub.shape == (3, 1, 6, 1) and C.same_bits(ub, TM.covariance_batch(None, win, None, 1, 6, 1)[0])
