"""The device calls of include/nnmnkwii_sample.h on CUDA tensors (csrc/mlpg_trajsample.hip): the three wrappers
that hand the current torch stream to the library.  The ctypes binding itself is ``_sample_hip``; the wrappers live apart from it
for the reason ``_trajectory_calls`` gives (tests/test_stream_contract_cpu.py pins the ``_*_hip.py`` modules that take the stream);
tests/test_trajsample_stream_gpu.py applies the same checks to the wrappers here and walks this module for ones it does not cover."""
from . import _hip
from ._sample_hip import draw_group, lib  # noqa: F401
from ._trajectory_calls import _variances
from ._trajectory_hip import half_bandwidth


def _planar_stride(t, name):
    """The row stride ld of a (P, B, Tmax, sd) tensor: the planes of a dense (P, B, Tmax, ld) tensor, columns contiguous."""
    P, B, Tmax, sd = t.shape
    s0, s1, s2, s3 = t.stride()
    ld = s2 if Tmax > 1 else (s1 if B > 1 else (s0 if P > 1 else sd))
    if P * B * Tmax * sd and ((sd > 1 and s3 != 1) or ld < sd or (Tmax > 1 and B > 1 and s1 != Tmax * ld)
                              or (P > 1 and B * Tmax > 1 and s0 != B * Tmax * ld)):
        raise ValueError("sample: %s must be a column slice of a dense (%d, B, Tmax, ld) tensor, got strides %s" % (name, P, (s0, s1, s2, s3)))
    return ld


def factor(variances, windows, lengths, B, Tmax, D, dtype=None, device=None, factor=None, logdet=None, status=None):
    """nnmk_draw_factor on CUDA tensors, with the arguments of ``_trajectory_calls.covariance``.  factor: float64
    (Q + 1, B, Tmax, sd), the planes of a dense (Q + 1, B, Tmax, ld) tensor of which it may be a column slice (None: a new dense
    tensor).  Returns (factor, logdet float64 (B, sd), status int32 (B, sd)).  One launch on the current stream, no synchronisation."""
    torch = _hip.torch_mod()
    nw, pl, pu, pc, _keep = _hip._win_args(windows)
    if nw < 1 or D % nw:
        raise ValueError("sample: D = %d is not a multiple of the %d windows" % (D, nw))
    sd = D // nw
    if variances is not None:
        dev, dtype = variances.device, variances.dtype
    else:
        dev = _hip.require_gpu(device)
        dtype = dtype or torch.float64
    if dev.type != "cuda":
        raise ValueError("sample: needs CUDA tensors")
    mode, ld_in = _variances(variances, dtype, dev, B, Tmax, D)
    _hip._check_lengths(lengths, B, dev)
    Q = half_bandwidth(windows)
    if factor is None:
        factor = torch.empty((Q + 1, B, Tmax, sd), dtype=torch.float64, device=dev)
    if not (torch.is_tensor(factor) and factor.device == dev and factor.dtype == torch.float64 and tuple(factor.shape) == (Q + 1, B, Tmax, sd)):
        raise ValueError("sample: factor must be a float64 (%d, %d, %d, %d) tensor on %s" % (Q + 1, B, Tmax, sd, dev))
    ld_fac = _planar_stride(factor, "factor")
    if logdet is None:
        logdet = torch.empty((B, sd), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty((B, sd), dtype=torch.int32, device=dev)
    for name, t, dt in (("logdet", logdet, torch.float64), ("status", status, torch.int32)):
        if not (t.device == dev and t.dtype == dt and tuple(t.shape) == (B, sd) and t.is_contiguous()):
            raise ValueError("sample: %s must be a contiguous %s (%d, %d) tensor on %s" % (name, dt, B, sd, dev))
    rc = lib().nnmk_draw_factor(dev.index, _hip._stream(dev), _hip.F32 if dtype == torch.float32 else _hip.F64, _hip._p(variances), mode, ld_in,
                                _hip._p(lengths), B, Tmax, D, sd, nw, pl, pu, pc, _hip._p(factor), ld_fac, _hip._p(logdet), _hip._p(status))
    _hip._check(rc, "nnmk_draw_factor")
    if B * Tmax * sd == 0:            # nothing was launched: an utterance without frames has log det 0
        logdet.zero_()
        status.zero_()
    return factor, logdet, status


def _draw_args(name, fac, status, lengths, src, mean, out):
    """(device, what the two draw entries take behind the stream, out)"""
    torch = _hip.torch_mod()
    if not (torch.is_tensor(src) and src.is_cuda and src.dim() == 4 and src.dtype in (torch.float32, torch.float64)):
        raise ValueError("sample: %s must be a float32 / float64 (K, B, Tmax, sd) CUDA tensor" % name)
    K, B, Tmax, sd = src.shape
    dev = src.device
    if not (torch.is_tensor(fac) and fac.device == dev and fac.dtype == torch.float64 and fac.dim() == 4 and tuple(fac.shape[1:]) == (B, Tmax, sd)
            and 1 <= fac.shape[0] <= 3):
        raise ValueError("sample: factor must be a float64 (Q + 1, %d, %d, %d) tensor on %s with Q <= 2" % (B, Tmax, sd, dev))
    Q = fac.shape[0] - 1
    if not (status.device == dev and status.dtype == torch.int32 and tuple(status.shape) == (B, sd) and status.is_contiguous()):
        raise ValueError("sample: status must be a contiguous int32 (%d, %d) tensor on %s" % (B, sd, dev))
    _hip._check_lengths(lengths, B, dev)
    ld_mean = sd
    if mean is not None:
        if not (torch.is_tensor(mean) and mean.device == dev and mean.dtype == src.dtype and tuple(mean.shape) == (B, Tmax, sd)):
            raise ValueError("sample: mean must be a %s (%d, %d, %d) tensor on %s" % (src.dtype, B, Tmax, sd, dev))
        ld_mean = _hip._pf_row_stride(mean, B, Tmax, sd, "sample")
    if out is None:
        out = torch.empty((K, B, Tmax, sd), dtype=src.dtype, device=dev)
    if not (torch.is_tensor(out) and out.device == dev and out.dtype == src.dtype and tuple(out.shape) == (K, B, Tmax, sd)):
        raise ValueError("sample: out must be a %s (%d, %d, %d, %d) tensor on %s" % (src.dtype, K, B, Tmax, sd, dev))
    return dev, (_hip._dt(src), _hip._p(fac), _planar_stride(fac, "factor"), _hip._p(status), _hip._p(lengths), B, Tmax, sd, Q, K, _hip._p(src),
                 _planar_stride(src, name), _hip._p(mean), ld_mean, _hip._p(out), _planar_stride(out, "out")), out


def sample(fac, status, lengths, noise, mean=None, out=None):
    """nnmk_draw_sample on CUDA tensors.  fac, status: what :func:`factor` returned; noise (K, B, Tmax, sd) float32 / float64 (a
    column slice of a dense tensor is fine); mean (B, Tmax, sd) of the same dtype or None; out like noise (None: a new dense
    tensor).  Returns out.  One launch on the current stream, no synchronisation."""
    dev, rest, out = _draw_args("noise", fac, status, lengths, noise, mean, out)
    _hip._check(lib().nnmk_draw_sample(dev.index, _hip._stream(dev), *rest), "nnmk_draw_sample")
    return out


def whiten(fac, status, lengths, x, mean=None, out=None):
    """nnmk_draw_whiten on CUDA tensors: the inverse of :func:`sample`, with the same arguments (x in the place of the noise)."""
    dev, rest, out = _draw_args("x", fac, status, lengths, x, mean, out)
    _hip._check(lib().nnmk_draw_whiten(dev.index, _hip._stream(dev), *rest), "nnmk_draw_whiten")
    return out
