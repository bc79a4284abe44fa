"""The device calls of include/nnmnkwii_trajectory.h on CUDA tensors (csrc/mlpg_trajcov.hip): the two wrappers that
hand the current torch stream to the library.  The ctypes binding itself is ``_trajectory_hip``.  They live apart from it because
tests/test_stream_contract_cpu.py pins the set of ``_*_hip.py`` modules whose wrappers take the stream, and the table those
wrappers must be named in, to what they were; tests/test_trajcov_stream_gpu.py applies the same checks to the two wrappers here
and walks this module for wrappers it does not cover."""
from . import _hip
from ._trajectory_hip import half_bandwidth, lib, nll_workspace


def _band_stride(band, Q, B, Tmax, sd):
    """The row stride ld of band (Q + 1, B, Tmax, sd): the planes of a dense (Q + 1, B, Tmax, ld) tensor, columns contiguous."""
    s0, s1, s2, s3 = band.stride()
    ld = s2 if Tmax > 1 else (s1 if B > 1 else (s0 if Q > 0 else sd))
    if B * Tmax * sd and ((sd > 1 and s3 != 1) or ld < sd or (Tmax > 1 and B > 1 and s1 != Tmax * ld)
                          or (Q > 0 and B * Tmax > 1 and s0 != B * Tmax * ld)):
        raise ValueError("trajectory: band must be a column slice of a dense (Q + 1, B, Tmax, ld) tensor, got strides %s" % ((s0, s1, s2, s3),))
    return ld


def _variances(var, ref_dtype, dev, B, Tmax, D):
    """(var_mode, ld_in) of the variances: None, a contiguous (D,) tensor, or a column slice of a dense (B, Tmax, ld) tensor."""
    torch = _hip.torch_mod()
    if var is None:
        return _hip.VAR_UNIT, D
    if not (torch.is_tensor(var) and var.device == dev and var.dtype == ref_dtype):
        raise ValueError("trajectory: the variances must be a %s tensor on %s" % (ref_dtype, dev))
    if var.dim() == 1:
        if tuple(var.shape) != (D,) or not var.is_contiguous():
            raise ValueError("trajectory: global variances must be a contiguous (%d,) tensor" % D)
        return _hip.VAR_GLOBAL, D
    if tuple(var.shape) != (B, Tmax, D):
        raise ValueError("trajectory: per-frame variances must be (%d, %d, %d), got %s" % (B, Tmax, D, tuple(var.shape)))
    return _hip.VAR_FRAME, _hip._pf_row_stride(var, B, Tmax, D, "trajectory")


def covariance(variances, windows, lengths, B, Tmax, D, dtype=None, device=None, want_band=True, band=None, logdet=None, status=None):
    """nnmk_traj_covariance on CUDA tensors.  variances: (B, Tmax, D) float32 / float64 (a column slice of a dense (B, Tmax, ld)
    tensor is fine), a contiguous (D,) tensor or None (unit variances: ``dtype`` and ``device`` say what ``variances`` cannot);
    lengths int32 (B) on the device or None.  band: float64 (Q + 1, B, Tmax, sd), the planes of a dense (Q + 1, B, Tmax, ld)
    tensor of which it may be a column slice (None: a new dense tensor; not needed without ``want_band``).  Returns (band or None,
    logdet float64 (B, sd), status int32 (B, sd)), all on the device.  One launch on the current stream, no synchronisation."""
    torch = _hip.torch_mod()
    nw, pl, pu, pc, _keep = _hip._win_args(windows)
    if nw < 1 or D % nw:
        raise ValueError("trajectory: D = %d is not a multiple of the %d windows" % (D, nw))
    sd = D // nw
    if variances is not None:
        dev, dtype = variances.device, variances.dtype
    else:
        dev = _hip.require_gpu(device)
        dtype = dtype or torch.float64
    if dev.type != "cuda":
        raise ValueError("trajectory: needs CUDA tensors")
    mode, ld_in = _variances(variances, dtype, dev, B, Tmax, D)
    _hip._check_lengths(lengths, B, dev)
    Q = half_bandwidth(windows)
    ld_band = sd
    if want_band:
        if band is None:
            band = torch.empty((Q + 1, B, Tmax, sd), dtype=torch.float64, device=dev)
        if not (torch.is_tensor(band) and band.device == dev and band.dtype == torch.float64 and tuple(band.shape) == (Q + 1, B, Tmax, sd)):
            raise ValueError("trajectory: band must be a float64 (%d, %d, %d, %d) tensor on %s" % (Q + 1, B, Tmax, sd, dev))
        ld_band = _band_stride(band, Q, B, Tmax, sd)
    else:
        band = None
    if logdet is None:
        logdet = torch.empty((B, sd), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty((B, sd), dtype=torch.int32, device=dev)
    for name, t, dt in (("logdet", logdet, torch.float64), ("status", status, torch.int32)):
        if not (t.device == dev and t.dtype == dt and tuple(t.shape) == (B, sd) and t.is_contiguous()):
            raise ValueError("trajectory: %s must be a contiguous %s (%d, %d) tensor on %s" % (name, dt, B, sd, dev))
    rc = lib().nnmk_traj_covariance(dev.index, _hip._stream(dev), _hip.F32 if dtype == torch.float32 else _hip.F64, _hip._p(variances), mode,
                                    ld_in, _hip._p(lengths), B, Tmax, D, sd, nw, pl, pu, pc, int(bool(want_band)), _hip._p(band), ld_band,
                                    _hip._p(logdet), _hip._p(status))
    _hip._check(rc, "nnmk_traj_covariance")
    if B * Tmax * sd == 0:            # nothing was launched: an utterance without frames has log det 0
        logdet.zero_()
        status.zero_()
    return band, logdet, status


def nll(means, variances, windows, cbar, target, lengths, band, logdet, want_grad_means=True, want_grad_vars=True, workspace=None):
    """nnmk_traj_nll on CUDA tensors.  means (B, Tmax, D) float32 / float64 and per-frame variances: column slices of dense
    (B, Tmax, ld) tensors with ONE row stride, or (D,) / None variances; cbar, target (B, Tmax, sd) of the same dtype (column
    slices are fine); band, logdet: what :func:`covariance` returned (band may be None unless the variance gradient is wanted).
    Returns (nll float64 (B, sd), grad_means (B, Tmax, D) or None, grad_vars like the variances or None), new dense tensors.
    One launch on the current stream, two with a global-variance gradient; no synchronisation."""
    torch = _hip.torch_mod()
    if not (torch.is_tensor(means) and means.is_cuda and means.dim() == 3 and means.dtype in (torch.float32, torch.float64)):
        raise ValueError("trajectory: means must be a float32 / float64 (B, Tmax, D) CUDA tensor")
    B, Tmax, D = means.shape
    dev = means.device
    nw, pl, pu, pc, _keep = _hip._win_args(windows)
    if nw < 1 or D % nw:
        raise ValueError("trajectory: D = %d is not a multiple of the %d windows" % (D, nw))
    sd = D // nw
    ld_in = _hip._pf_row_stride(means, B, Tmax, D, "trajectory")
    mode, ld_var = _variances(variances, means.dtype, dev, B, Tmax, D)
    if mode == _hip.VAR_FRAME and B * Tmax * D and ld_var != ld_in:
        raise ValueError("trajectory: means and per-frame variances must share one row stride (%d, %d)" % (ld_in, ld_var))
    _hip._check_lengths(lengths, B, dev)
    lds = []
    for name, t in (("cbar", cbar), ("target", target)):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == means.dtype and tuple(t.shape) == (B, Tmax, sd)):
            raise ValueError("trajectory: %s must be a %s (%d, %d, %d) tensor on %s" % (name, means.dtype, B, Tmax, sd, dev))
        lds.append(_hip._pf_row_stride(t, B, Tmax, sd, "trajectory"))
    want_grad_vars = bool(want_grad_vars) and mode != _hip.VAR_UNIT
    Q = half_bandwidth(windows)
    ld_band = sd
    if band is not None:
        if not (band.device == dev and band.dtype == torch.float64 and tuple(band.shape) == (Q + 1, B, Tmax, sd)):
            raise ValueError("trajectory: band must be a float64 (%d, %d, %d, %d) tensor on %s" % (Q + 1, B, Tmax, sd, dev))
        ld_band = _band_stride(band, Q, B, Tmax, sd)
    elif want_grad_vars:
        raise ValueError("trajectory: the variance gradient needs the band")
    if not (logdet.device == dev and logdet.dtype == torch.float64 and tuple(logdet.shape) == (B, sd) and logdet.is_contiguous()):
        raise ValueError("trajectory: logdet must be a contiguous float64 (%d, %d) tensor on %s" % (B, sd, dev))
    out = torch.empty((B, sd), dtype=torch.float64, device=dev)
    gm = torch.empty((B, Tmax, D), dtype=means.dtype, device=dev) if want_grad_means else None
    gv = None
    if want_grad_vars:
        gv = torch.empty((D,) if mode == _hip.VAR_GLOBAL else (B, Tmax, D), dtype=means.dtype, device=dev)
    need = nll_workspace(mode, want_grad_vars, B, D)
    if need and workspace is None:
        workspace = torch.empty((need // 8,), dtype=torch.float64, device=dev)
    have = workspace.numel() * workspace.element_size() if workspace is not None else 0
    rc = lib().nnmk_traj_nll(dev.index, _hip._stream(dev), _hip._dt(means), _hip._p(means), _hip._p(variances), mode, ld_in, _hip._p(lengths),
                             B, Tmax, D, sd, nw, pl, pu, pc, _hip._p(cbar), lds[0], _hip._p(target), lds[1], _hip._p(band), ld_band,
                             _hip._p(logdet), _hip._p(out), _hip._p(gm), _hip._p(gv), _hip._p(workspace), have)
    _hip._check(rc, "nnmk_traj_nll")
    if B * Tmax * sd == 0:            # nothing was launched
        for t in (out, gm, gv):
            if t is not None:
                t.zero_()
    return out, gm, gv
