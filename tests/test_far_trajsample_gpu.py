"""GPU tests (-m gpu) of nnmk_draw_factor, nnmk_draw_sample and nnmk_draw_whiten far from their pointers (tests/far.py): factor
planes past the 2^31- and 2^32-byte offsets of ONE parent allocation (written by the factor entry, read by the other two), the
noise / x rows past them, and the rows of the draws / the whitened rows past them.  Only the addresses are far apart: every
utterance has a handful of live frames, everything else is the fill byte, and the whole allocation is checked afterwards -- a row
offset that wrapped in 32 bits lands inside the caller's own buffer and shows as a stray write or a wrong value, not as a fault.

Every case fits the memory a far test may use (far.MEM_CAP): the input and the output of one call are never far at once -- two
parents past 2^32 bytes each, of three 2.3e9-byte slabs, would be 13.8e9 bytes -- so the inputs' case has a dense output and the
outputs' case dense inputs."""
import gc

import numpy as np
import pytest
import torch

import far as F
import trajcov_cases as C
import trajsample_cases as S
from trajcov_cases import TM
from trajsample_cases import SM

pytestmark = pytest.mark.gpu
WNAME = "std3"
WIN = C.WINDOWS[WNAME]
TL = 5                      # the live rows looked at


def _lib():
    from nnmnkwii_amd import _hip, _sample_hip as SH
    dev = torch.device("cuda", torch.cuda.current_device())
    return SH.lib(), dev.index, _hip._stream(dev), _hip.pack_windows(WIN)


def _factor(var, lengths, B, Tmax, sd, fac_ptr, ld_fac, logdet, status):
    L, di, st, (wl, wu, wc) = _lib()
    rc = L.nnmk_draw_factor(di, st, 1, var.data_ptr(), TM.VAR_GLOBAL, 3 * sd, lengths.data_ptr(), B, Tmax, 3 * sd, sd, 3, wl.ctypes.data,
                            wu.ctypes.data, wc.ctypes.data, fac_ptr, ld_fac, logdet.data_ptr(), status.data_ptr())
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()


def _draw(name, fac_ptr, ld_fac, status, lengths, B, Tmax, sd, K, src_ptr, ld_src, mean, dst_ptr, ld_dst):
    L, di, st, _ = _lib()
    rc = getattr(L, name)(di, st, 1, fac_ptr, ld_fac, status.data_ptr(), lengths.data_ptr(), B, Tmax, sd, 2, K, src_ptr, ld_src,
                          None if mean is None else mean.data_ptr(), sd, dst_ptr, ld_dst)
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()


def _padded(a, Tmax):
    """(..., TL, sd) -> the dense device tensor (..., Tmax, sd), zeros behind the live rows."""
    t = torch.zeros(a.shape[:-2] + (Tmax, a.shape[-1]), dtype=torch.float64, device="cuda")
    t[..., :a.shape[-2], :] = torch.from_numpy(a).cuda()
    return t


def _release(*parents):
    for p in parents:
        p.free()
    gc.collect()
    torch.cuda.empty_cache()


def _small(seed, K, B, sd, lengths):
    g = C.variances(seed, 1, 1, sd, WNAME, TM.VAR_GLOBAL)
    rng = np.random.RandomState(seed)
    noise, mean = rng.randn(K, B, TL, sd), rng.randn(B, TL, sd)
    fac, _, status = SM.factor_batch(g, WIN, lengths, B, TL, sd)
    x = SM.sample_batch(fac, status, lengths, noise, mean)
    z = SM.whiten_batch(fac, status, lengths, x, mean)
    unit = S.units(g, WNAME, lengths, B, TL, sd)
    return g, noise, mean, fac, status, x, z, unit


def test_factor_planes_past_the_2g_and_4g_offsets():
    K, B, Tmax, sd, ld_fac, col0, lengths = 2, 3, 70000, 3, 1024, 7, [5, 4, 3]  # a plane of one utterance is 5.7e8 bytes: nine of them
    g, noise, mean, mfac, _, mx, mz, unit = _small(2, K, B, sd, lengths)
    parent = F.FarParent((3 * B, Tmax, ld_fac), np.float64, F.low_guard_for(9 * Tmax * ld_fac * 8))
    for pb in range(3 * B):
        parent.expect_written(pb, Tmax, col0, sd)
    assert {"2^31 bytes", "2^32 bytes"} <= parent.crossed(col0)
    gv, L = torch.from_numpy(g).cuda(), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    logdet, status = torch.empty((B, sd), dtype=torch.float64, device="cuda"), torch.empty((B, sd), dtype=torch.int32, device="cuda")
    _factor(gv, L, B, Tmax, sd, parent.ptr(col0), ld_fac, logdet, status)
    for k in range(3):
        for b in range(B):
            assert C.same_bits(parent.read(k * B + b, TL, col0, sd), mfac[k, b])
            assert bool((parent.view[k * B + b, TL:, col0:col0 + sd] == 0).all())
    assert not status.any().item()
    # ... and read from there: the draws and the whitened rows
    out = torch.full((K, B, Tmax, sd), -7.0, dtype=torch.float64, device="cuda")
    z = torch.full((K, B, Tmax, sd), -7.0, dtype=torch.float64, device="cuda")
    m, nz = _padded(mean, Tmax), _padded(noise, Tmax)
    _draw("nnmk_draw_sample", parent.ptr(col0), ld_fac, status, L, B, Tmax, sd, K, nz.data_ptr(), sd, m, out.data_ptr(), sd)
    _draw("nnmk_draw_whiten", parent.ptr(col0), ld_fac, status, L, B, Tmax, sd, K, out.data_ptr(), sd, m, z.data_ptr(), sd)
    S.within_bound(out[:, :, :TL].cpu().numpy(), mx, unit, lengths, False)
    S.within_bound(z[:, :, :TL].cpu().numpy(), SM.whiten_batch(mfac, status.cpu().numpy(), lengths, out[:, :, :TL].cpu().numpy(), mean), unit, lengths, False)
    assert bool((out[:, :, TL:] == 0).all()) and bool((z[:, :, TL:] == 0).all())
    assert parent.untouched() == []
    del out, z, m, nz
    _release(parent)


def test_noise_and_x_rows_past_the_2g_and_4g_offsets():
    """K = 3 draws of one utterance: the draw stride B Tmax ld is 2.29e9 bytes, so draw 1 begins past 2^31 and draw 2 past 2^32."""
    K, B, Tmax, sd, ld, col0, lengths = 3, 1, 70000, 3, 4096, 5, [5]
    g, noise, mean, mfac, mstatus, mx, mz, unit = _small(3, K, B, sd, lengths)
    parent = F.FarParent((K * B, Tmax, ld), np.float64, F.low_guard_for(K * B * Tmax * ld * 8))
    for k in range(K):
        parent.place(k, TL, col0, noise[k, 0])
    assert {"2^31 bytes", "2^32 bytes"} <= parent.crossed(col0)
    L = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    fac, status = _padded(mfac, Tmax), torch.zeros((B, sd), dtype=torch.int32, device="cuda")
    m = _padded(mean, Tmax)
    out = torch.full((K, B, Tmax, sd), -7.0, dtype=torch.float64, device="cuda")
    _draw("nnmk_draw_sample", fac.data_ptr(), sd, status, L, B, Tmax, sd, K, parent.ptr(col0), ld, m, out.data_ptr(), sd)
    S.within_bound(out[:, :, :TL].cpu().numpy(), mx, unit, lengths, False)
    assert bool((out[:, :, TL:] == 0).all()) and parent.untouched() == []
    # the same parent as the x of the inverse map: the model's draws placed where the noise was
    parent.forget()
    for k in range(K):
        parent.place(k, TL, col0, mx[k, 0])
    out.fill_(-7.0)
    _draw("nnmk_draw_whiten", fac.data_ptr(), sd, status, L, B, Tmax, sd, K, parent.ptr(col0), ld, m, out.data_ptr(), sd)
    S.within_bound(out[:, :, :TL].cpu().numpy(), mz, unit, lengths, False)
    assert bool((out[:, :, TL:] == 0).all()) and parent.untouched() == []
    del out, fac, m
    _release(parent)


def test_output_rows_past_the_2g_and_4g_offsets():
    """The draws, then the whitened rows, as a column slice of a far parent: every row of the slice is written (zeros at or past
    T), nothing outside it."""
    K, B, Tmax, sd, ld, col0, lengths = 3, 1, 70000, 3, 4096, 9, [5]
    g, noise, mean, mfac, mstatus, mx, mz, unit = _small(4, K, B, sd, lengths)
    parent = F.FarParent((K * B, Tmax, ld), np.float64, F.low_guard_for(K * B * Tmax * ld * 8))
    for k in range(K):
        parent.expect_written(k, Tmax, col0, sd)
    assert {"2^31 bytes", "2^32 bytes"} <= parent.crossed(col0)
    L = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    fac, status = _padded(mfac, Tmax), torch.zeros((B, sd), dtype=torch.int32, device="cuda")
    m = _padded(mean, Tmax)
    for name, src, ref in (("nnmk_draw_sample", noise, mx), ("nnmk_draw_whiten", mx, mz)):
        dense = _padded(src, Tmax)
        _draw(name, fac.data_ptr(), sd, status, L, B, Tmax, sd, K, dense.data_ptr(), sd, m, parent.ptr(col0), ld)
        got = np.stack([parent.read(k, TL, col0, sd) for k in range(K)])[:, None]
        S.within_bound(got, ref, unit, lengths, False)
        for k in range(K):
            assert bool((parent.view[k, TL:, col0:col0 + sd] == 0).all())
        assert parent.untouched() == []                            # (refills the slice: the second entry starts from the fill byte)
    del fac, m, dense
    _release(parent)
