"""GPU tests (-m gpu) of nnmk_traj_covariance and nnmk_traj_nll far from their pointers (tests/far.py): a few live rows of per-frame
variances past the 2^31- and 2^32-byte offsets of ONE parent allocation, band planes past them, and the likelihood's means and
gradient rows past them.  Only the addresses are far apart: every utterance has a handful of live frames, everything else is the
fill byte, and the whole allocation is checked afterwards -- a row offset that wrapped in 32 bits lands inside the caller's own
buffer and shows as a stray write or a wrong value, not as a fault."""
import gc

import numpy as np
import pytest
import torch

import far as F
import trajcov_cases as C
from trajcov_cases import TM

pytestmark = pytest.mark.gpu
WNAME = "std3"
WIN = C.WINDOWS[WNAME]


def _call(var_ptr, mode, ld_in, lengths, B, Tmax, sd, band_ptr, ld_band, logdet, status):
    from nnmnkwii_amd import _hip, _trajectory_hip as TH
    L = TH.lib()
    wl, wu, wc = _hip.pack_windows(WIN)
    dev = torch.device("cuda", torch.cuda.current_device())
    rc = L.nnmk_traj_covariance(dev.index, _hip._stream(dev), 1, var_ptr, mode, ld_in, lengths.data_ptr(), B, Tmax, 3 * sd, sd, 3,
                                wl.ctypes.data, wu.ctypes.data, wc.ctypes.data, 1, band_ptr, ld_band, logdet.data_ptr(), status.data_ptr())
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()


def test_variance_rows_past_the_2g_and_4g_offsets():
    B, Tmax, sd, ld_in, col0, lengths = 3, 70000, 3, 4096, 5, [5, 4, 3]       # an utterance is 2.29e9 bytes of rows
    parent = F.FarParent((B, Tmax, ld_in), np.float64, F.low_guard_for(B * Tmax * ld_in * 8))
    var = C.variances(1, B, 5, sd, WNAME, TM.VAR_FRAME)
    for b in range(B):
        parent.place(b, lengths[b], col0, var[b, :lengths[b]])
    assert {"2^31 bytes", "2^32 bytes"} <= parent.crossed(col0)
    L = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    band = torch.full((3, B, Tmax, sd), -7.0, dtype=torch.float64, device="cuda")
    logdet, status = torch.empty((B, sd), dtype=torch.float64, device="cuda"), torch.empty((B, sd), dtype=torch.int32, device="cuda")
    _call(parent.ptr(col0), TM.VAR_FRAME, ld_in, L, B, Tmax, sd, band.data_ptr(), sd, logdet, status)
    assert parent.untouched() == []
    mband, mlogdet, mstatus = TM.covariance_batch(var, WIN, lengths, B, 5, sd)
    assert C.same_bits(band[:, :, :5].cpu().numpy(), mband) and bool((band[:, :, 5:] == 0).all()) and not status.any().item()
    for b in range(B):
        assert (np.abs(logdet[b].cpu().numpy() - mlogdet[b]) <= C.logdet_bound(var[b], WNAME, lengths[b], sd)).all()
    parent.free()
    del parent, band
    gc.collect()
    torch.cuda.empty_cache()


def test_band_planes_past_the_2g_and_4g_offsets():
    B, Tmax, sd, ld_band, col0, lengths = 3, 70000, 3, 1024, 7, [5, 4, 3]     # a plane of one utterance is 5.7e8 bytes: nine of them
    parent = F.FarParent((3 * B, Tmax, ld_band), np.float64, F.low_guard_for(9 * Tmax * ld_band * 8))
    for pb in range(3 * B):
        parent.expect_written(pb, Tmax, col0, sd)
    assert {"2^31 bytes", "2^32 bytes"} <= parent.crossed(col0)
    g = C.variances(2, 1, 1, sd, WNAME, TM.VAR_GLOBAL)
    gv = torch.from_numpy(g).cuda()
    L = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    logdet, status = torch.empty((B, sd), dtype=torch.float64, device="cuda"), torch.empty((B, sd), dtype=torch.int32, device="cuda")
    _call(gv.data_ptr(), TM.VAR_GLOBAL, 3 * sd, L, B, Tmax, sd, parent.ptr(col0), ld_band, logdet, status)
    mband, mlogdet, _ = TM.covariance_batch(g, WIN, lengths, B, 5, sd)
    for k in range(3):
        for b in range(B):
            assert C.same_bits(parent.read(k * B + b, 5, col0, sd), mband[k, b])
            assert bool((parent.view[k * B + b, 5:, col0:col0 + sd] == 0).all())
    assert parent.untouched() == [] and not status.any().item()
    parent.free()
    del parent
    gc.collect()
    torch.cuda.empty_cache()


def _nll(means_ptr, ld_in, gvar, L, B, Tmax, sd, cb, tg, band, logdet, nll, gm_ptr, gv, work):
    from nnmnkwii_amd import _hip, _trajectory_hip as TH
    lib = TH.lib()
    wl, wu, wc = _hip.pack_windows(WIN)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.nnmk_traj_nll(dev.index, _hip._stream(dev), 1, means_ptr, gvar.data_ptr(), TM.VAR_GLOBAL, ld_in, L.data_ptr(), B, Tmax, 3 * sd, sd, 3,
                           wl.ctypes.data, wu.ctypes.data, wc.ctypes.data, cb.data_ptr(), sd, tg.data_ptr(), sd, p(band), sd, logdet.data_ptr(),
                           nll.data_ptr(), gm_ptr, p(gv), p(work), 0 if work is None else work.numel() * 8)
    assert rc == 0, lib.mlpg_hip_last_error()
    torch.cuda.synchronize()


def _small_case(seed, B, sd, lengths, Tl=5):
    g = C.variances(seed, 1, 1, sd, WNAME, TM.VAR_GLOBAL)
    mean, target = C.features(seed + 1, B, Tl, 3 * sd), C.features(seed + 2, B, Tl, sd)
    cbar = np.zeros((B, Tl, sd))
    for b in range(B):
        cbar[b, :lengths[b]] = TM.mean_trajectory(mean[b], g, WIN, lengths[b], sd)
    return g, mean, target, cbar


def _padded(a, Tmax):
    t = torch.zeros((a.shape[0], Tmax, a.shape[2]), dtype=torch.float64, device="cuda")
    t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return t


def test_likelihood_means_past_the_2g_and_4g_offsets():
    """The means are read for the variance gradient alone: global variances with their gradient wanted, the means a column
    slice of a far parent; the likelihood, both gradients and the inputs are checked."""
    B, Tmax, sd, ld_in, col0, lengths = 3, 70000, 3, 4096, 5, [5, 4, 3]
    D = 3 * sd
    g, mean, target, cbar = _small_case(7, B, sd, lengths)
    means = F.FarParent((B, Tmax, ld_in), np.float64, F.low_guard_for(B * Tmax * ld_in * 8))
    for b in range(B):
        means.place(b, lengths[b], col0, mean[b, :lengths[b]])
    assert {"2^31 bytes", "2^32 bytes"} <= means.crossed(col0)
    gvar, L = torch.from_numpy(g).cuda(), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    band = torch.empty((3, B, Tmax, sd), dtype=torch.float64, device="cuda")
    logdet, status = torch.empty((B, sd), dtype=torch.float64, device="cuda"), torch.empty((B, sd), dtype=torch.int32, device="cuda")
    _call(gvar.data_ptr(), TM.VAR_GLOBAL, D, L, B, Tmax, sd, band.data_ptr(), sd, logdet, status)
    nll = torch.empty((B, sd), dtype=torch.float64, device="cuda")
    gm = torch.full((B, Tmax, D), -7.0, dtype=torch.float64, device="cuda")
    gv, work = torch.empty((D,), dtype=torch.float64, device="cuda"), torch.empty((B * D,), dtype=torch.float64, device="cuda")
    _nll(means.ptr(col0), ld_in, gvar, L, B, Tmax, sd, _padded(cbar, Tmax), _padded(target, Tmax), band, logdet, nll, gm.data_ptr(), gv, work)
    want = TM.nll_batch(mean, g, WIN, cbar, target, lengths, band[:, :, :5].cpu().numpy(), logdet.cpu().numpy())
    assert C.same_bits(nll.cpu().numpy(), want[0]) and C.same_bits(gm[:, :5].cpu().numpy(), want[1]) and bool((gm[:, 5:] == 0).all())
    assert C.same_bits(gv.cpu().numpy(), want[2]) and means.untouched() == []
    means.free()
    del means, band, gm
    gc.collect()
    torch.cuda.empty_cache()


def test_likelihood_gradient_rows_past_the_2g_offset():
    """The gradient is dense, (B, Tmax, D): wide rows (1024 static dims, D = 3072) put the second utterance's rows past 2^31
    bytes.  Means of the same size must exist beside it, so a second utterance past 2^32 bytes would not fit the memory a far
    test may use (far.MEM_CAP): this case crosses 2^31 alone.  Every row of the parent is written: zeros at or past T."""
    B, Tmax, sd, lengths = 2, 90000, 1024, [5, 4]
    D = 3 * sd
    g, mean, target, cbar = _small_case(11, B, sd, lengths)
    grads = F.FarParent((B, Tmax, D), np.float64, 4096, boundaries=F.BOUNDARIES[:1])
    for b in range(B):
        grads.expect_written(b, lengths[b], 0, D)
    assert grads.crossed(0) == {"2^31 bytes"}
    gvar, L = torch.from_numpy(g).cuda(), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    logdet, status = torch.empty((B, sd), dtype=torch.float64, device="cuda"), torch.empty((B, sd), dtype=torch.int32, device="cuda")
    from nnmnkwii_amd import _trajectory_calls as TC
    TC.covariance(gvar, WIN, L, B, Tmax, D, want_band=False, logdet=logdet, status=status)
    nll = torch.empty((B, sd), dtype=torch.float64, device="cuda")
    m = _padded(mean, Tmax)
    _nll(m.data_ptr(), D, gvar, L, B, Tmax, sd, _padded(cbar, Tmax), _padded(target, Tmax), None, logdet, nll, grads.ptr(0), None, None)
    want = TM.nll_batch(mean, g, WIN, cbar, target, lengths, None, logdet.cpu().numpy(), want_grad=False)
    assert C.same_bits(nll.cpu().numpy(), want[0]) and not status.any().item()
    for b in range(B):
        assert C.same_bits(grads.read(b, lengths[b], 0, D), want[1][b, :lengths[b]])
    assert grads.untouched(rest=0) == []
    grads.free()
    del grads, m
    gc.collect()
    torch.cuda.empty_cache()
