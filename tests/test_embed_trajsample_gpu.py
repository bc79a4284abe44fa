"""GPU tests (-m gpu): nnmk_draw_factor, nnmk_draw_sample and nnmk_draw_whiten on buffers at odd element offsets between guard
bands (tests/embed.py), every array of its exact size: the variances, the noise, the mean, the draws and the whitened rows as
column slices of wider rows whose other columns hold the fill byte, the factor planes as a column slice of wider planes.  A store
before or behind an output, into a foreign column or into an input shows in the guards, in the fill of the foreign columns or in
the inputs' snapshot."""
import numpy as np
import pytest
import torch

import embed as E
import trajcov_cases as C
import trajsample_cases as S
from trajcov_cases import TM
from trajsample_cases import SM

pytestmark = pytest.mark.gpu
FILL = 0xA5


def sliced(a, ld, off):
    """A (rows, width) array as the first `width` columns of rows with stride ld, in an exact-size block (it ends behind the last
    row's last column) at element offset `off`: (the Embedded, the flat indices of the slice's elements)."""
    rows, width = a.shape
    n = (rows - 1) * ld + width
    emb = E.Embedded((n,), a.dtype, off, fill_byte=FILL)
    flat = emb.payload()
    flat.view(torch.uint8).fill_(FILL)
    idx = (torch.arange(rows, device="cuda")[:, None] * ld + torch.arange(width, device="cuda")[None, :]).reshape(-1)
    flat[idx] = torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)
    emb.snapshot()
    return emb, idx


def read(emb, idx, rows, width):
    flat = emb.payload()
    mask = torch.ones(flat.shape, dtype=torch.bool, device="cuda")
    mask[idx] = False
    foreign = flat[mask].view(torch.uint8) if mask.any() else torch.zeros(0, dtype=torch.uint8)
    return flat[idx].reshape(rows, width).cpu().numpy(), bool((foreign == FILL).all())


@pytest.mark.parametrize("dtype,offs", [(np.float64, (1, 3, 5, 7)), (np.float32, (3, 1, 7, 5))])
@pytest.mark.parametrize("mode", C.MODES)
def test_offset_buffers_between_guard_bands(dtype, offs, mode):
    from nnmnkwii_amd import _hip, _sample_hip as SH
    L = SH.lib()
    K, B, Tmax, sd, wname, lengths = SH.draw_group() + 1, 3, 9, 65, "std3", [9, 0, 5]
    win = C.WINDOWS[wname]
    nw, Q = len(win), 2
    D = nw * sd
    rows = B * Tmax
    var, noise, mean = S.inputs(3, K, B, Tmax, sd, wname, mode, dtype, lengths)
    ld_in, ld_fac, ld_n, ld_m, ld_o, ld_z = D + 3, sd + 2, sd + 1, sd + 5, sd + 3, sd + 4
    if mode == TM.VAR_FRAME:
        e_var, _ = sliced(var.reshape(rows, D), ld_in, offs[1])
    else:
        e_var = E.embedded(var, offs[1])
    e_noise, _ = sliced(noise.reshape(K * rows, sd), ld_n, offs[0])
    e_mean, _ = sliced(mean.reshape(rows, sd), ld_m, offs[2])
    e_len = E.embedded(np.array(lengths, dtype=np.int32), 1)
    e_fac, i_fac = sliced(np.full(((Q + 1) * rows, sd), -7.0), ld_fac, offs[3])
    e_out, i_out = sliced(np.full((K * rows, sd), -7.0, dtype=dtype), ld_o, offs[1])
    e_z, i_z = sliced(np.full((K * rows, sd), -7.0, dtype=dtype), ld_z, offs[2])
    e_logdet, e_status = E.Embedded((B, sd), np.float64, 1, fill_byte=FILL), E.Embedded((B, sd), np.int32, 3, fill_byte=FILL)
    wl, wu, wc = _hip.pack_windows(win)
    dev = torch.device("cuda", torch.cuda.current_device())
    st, dt = _hip._stream(dev), int(dtype == np.float64)
    n0 = L.nnmk_draw_launch_count()
    rc = L.nnmk_draw_factor(dev.index, st, dt, E.ptr(e_var), mode, ld_in, e_len.ptr(), B, Tmax, D, sd, nw, wl.ctypes.data, wu.ctypes.data,
                            wc.ctypes.data, e_fac.ptr(), ld_fac, e_logdet.ptr(), e_status.ptr())
    assert rc == 0, L.mlpg_hip_last_error()
    rc = L.nnmk_draw_sample(dev.index, st, dt, e_fac.ptr(), ld_fac, e_status.ptr(), e_len.ptr(), B, Tmax, sd, Q, K, e_noise.ptr(), ld_n,
                            e_mean.ptr(), ld_m, e_out.ptr(), ld_o)
    assert rc == 0, L.mlpg_hip_last_error()
    rc = L.nnmk_draw_whiten(dev.index, st, dt, e_fac.ptr(), ld_fac, e_status.ptr(), e_len.ptr(), B, Tmax, sd, Q, K, e_out.ptr(), ld_o,
                            e_mean.ptr(), ld_m, e_z.ptr(), ld_z)
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert L.nnmk_draw_launch_count() == n0 + 3
    assert E.failed(inputs=dict(var=e_var, noise=e_noise, mean=e_mean, lengths=e_len),
                    outputs=dict(factor=e_fac, logdet=e_logdet, status=e_status, out=e_out, z=e_z), workspaces={}) == []
    fac, clean_f = read(e_fac, i_fac, (Q + 1) * rows, sd)
    out, clean_o = read(e_out, i_out, K * rows, sd)
    z, clean_z = read(e_z, i_z, K * rows, sd)
    assert clean_f and clean_o and clean_z                                        # the foreign columns still hold the fill
    mfac, mlogdet, mstatus = SM.factor_batch(var, win, lengths, B, Tmax, sd)
    assert C.same_bits(fac.reshape(Q + 1, B, Tmax, sd), mfac) and np.array_equal(e_status.host(), mstatus)
    logdet = e_logdet.host()
    for b in range(B):
        v = None if var is None else (var if var.ndim == 1 else var[b])
        assert (np.abs(logdet[b] - mlogdet[b]) <= C.logdet_bound(v, wname, lengths[b], sd)).all()
    unit = S.units(var, wname, lengths, B, Tmax, sd)
    out, z = out.reshape(K, B, Tmax, sd), z.reshape(K, B, Tmax, sd)
    m64 = mean.astype(np.float64)
    S.within_bound(out, SM.sample_batch(mfac, mstatus, lengths, noise.astype(np.float64), m64), unit, lengths, dtype == np.float32)
    S.within_bound(z, SM.whiten_batch(mfac, mstatus, lengths, out.astype(np.float64), m64), unit, lengths, dtype == np.float32)
