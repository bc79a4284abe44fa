"""GPU tests (-m gpu): nnmk_traj_covariance and nnmk_traj_nll on buffers at odd element offsets between guard bands
(tests/embed.py), every array of its exact size: the variances, the means, cbar and the target as column slices of wider rows
whose other columns hold the fill byte, the band planes as a column slice of wider planes.  A store before or behind an output,
into a foreign column or into an input shows in the guards, in the fill of the foreign columns or in the inputs' snapshot."""
import numpy as np
import pytest
import torch

import embed as E
import trajcov_cases as C
from trajcov_cases import TM

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
    from nnmnkwii_amd import _hip, _trajectory_hip as TH
    L = TH.lib()
    B, Tmax, sd, wname, lengths = 3, 9, 65, "std3", [9, 0, 5]
    win = C.WINDOWS[wname]
    nw, Q = len(win), 2
    D = nw * sd
    rows = B * Tmax
    var = C.variances(3, B, Tmax, sd, wname, mode, dtype)
    mean, target = C.features(4, B, Tmax, D, dtype), C.features(5, B, Tmax, sd, dtype)
    cbar = np.zeros((B, Tmax, sd), dtype=dtype)
    for b in range(B):
        v = None if var is None else (var if var.ndim == 1 else var[b])
        cbar[b, :lengths[b]] = TM.mean_trajectory(mean[b], v, win, lengths[b], sd).astype(dtype)
    ld_in, ld_band, ld_c, ld_t = D + 3, sd + 2, sd + 1, sd + 5
    e_mean, i_mean = sliced(mean.reshape(rows, D), ld_in, offs[0])
    if mode == TM.VAR_FRAME:
        e_var, _ = sliced(var.reshape(rows, D), ld_in, offs[1])
    else:
        e_var = E.embedded(var, offs[1])
    e_cbar, _ = sliced(cbar.reshape(rows, sd), ld_c, offs[2])
    e_tgt, _ = sliced(target.reshape(rows, sd), ld_t, offs[3])
    e_len = E.embedded(np.array(lengths, dtype=np.int32), 1)
    e_band, i_band = sliced(np.full(((Q + 1) * rows, sd), -7.0), ld_band, offs[0])
    e_logdet, e_status = E.Embedded((B, sd), np.float64, 1, fill_byte=FILL), E.Embedded((B, sd), np.int32, 3, fill_byte=FILL)
    e_nll = E.Embedded((B, sd), np.float64, 5, fill_byte=FILL)
    e_gm = E.Embedded((B, Tmax, D), dtype, 3, fill_byte=FILL)
    e_gv = None if mode == TM.VAR_UNIT else E.Embedded((B, Tmax, D) if mode == TM.VAR_FRAME else (D,), dtype, 1, fill_byte=FILL)
    need = TH.nll_workspace(mode, True, B, D)
    e_work = E.Workspace(need) if need else None
    wl, wu, wc = _hip.pack_windows(win)
    dev = torch.device("cuda", torch.cuda.current_device())
    st, dt = _hip._stream(dev), int(dtype == np.float64)
    esz = np.dtype(dtype).itemsize
    n0 = L.nnmk_traj_launch_count()
    rc = L.nnmk_traj_covariance(dev.index, st, dt, E.ptr(e_var), mode, ld_in, e_len.ptr(), B, Tmax, D, sd, nw, wl.ctypes.data, wu.ctypes.data,
                                wc.ctypes.data, 1, e_band.ptr(), ld_band, e_logdet.ptr(), e_status.ptr())
    assert rc == 0, L.mlpg_hip_last_error()
    rc = L.nnmk_traj_nll(dev.index, st, dt, e_mean.ptr(), E.ptr(e_var), mode, ld_in, e_len.ptr(), B, Tmax, D, sd, nw, wl.ctypes.data,
                         wu.ctypes.data, wc.ctypes.data, e_cbar.ptr(), ld_c, e_tgt.ptr(), ld_t, e_band.ptr(), ld_band, e_logdet.ptr(),
                         e_nll.ptr(), e_gm.ptr(), E.ptr(e_gv), E.ptr(e_work), need)
    assert rc == 0, L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert L.nnmk_traj_launch_count() == n0 + 2 and esz in (4, 8)
    assert E.failed(inputs=dict(mean=e_mean, var=e_var, cbar=e_cbar, target=e_tgt, lengths=e_len),
                    outputs=dict(band=e_band, logdet=e_logdet, status=e_status, nll=e_nll, gm=e_gm, gv=e_gv), workspaces=dict(work=e_work)) == []
    band, clean = read(e_band, i_band, (Q + 1) * rows, sd)
    assert clean                                                                   # the planes' foreign columns still hold the fill
    mband, mlogdet, mstatus = TM.covariance_batch(var, win, lengths, B, Tmax, sd)
    assert C.same_bits(band.reshape(Q + 1, B, Tmax, sd), mband) and np.array_equal(e_status.host(), mstatus)
    logdet = e_logdet.host()
    for b in range(B):
        v = None if var is None else (var if var.ndim == 1 else var[b])
        assert (np.abs(logdet[b] - mlogdet[b]) <= C.logdet_bound(v, wname, lengths[b], sd)).all()
    nll, gm, gv = TM.nll_batch(mean, var, win, cbar, target, lengths, mband, logdet)
    assert C.same_bits(e_nll.host(), nll) and C.same_bits(e_gm.host(), gm)
    if e_gv is not None:
        assert C.same_bits(e_gv.host(), gv)
