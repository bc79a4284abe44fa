"""Continuous F0: the unvoiced gaps of an F0 / log-F0 track filled, and the voiced / unvoiced flag, on the device
(mirror of nnmnkwii/preprocessing/f0.py; csrc/f0_interp.hip; tools/f0_model.py is the specification).

    X[:, :, LF0], X[:, :, VUV] <- interp1d_batch(X[:, :, LF0:LF0 + 1], lengths, out=..., vuv=...)     # in place, one launch
    D = delta_features(X[:, :, :LF0 + 1], windows); column_stats(D, lengths); scale(D, mean, std, lengths)
"""
import numpy as np

from .. import _f0_hip, _hip
from .generic import _device_lengths

KINDS = _f0_hip.KINDS


def _float_dtype(x):
    return x.dtype if x.dtype in (np.float32, np.float64) else np.dtype(np.float64)


def interp1d(f0, kind="slinear"):
    """Continuous F0 interpolation from a discontinuous F0 trajectory.

    Drop-in for ``nnmnkwii.preprocessing.interp1d`` (preprocessing/f0.py:5-68): ``f0`` is a ``(T,)`` or ``(T, 1)`` array, the
    result has its shape and dtype; anything else raises ``RuntimeError("1d array is only supported")``.  Frames with
    ``f0 <= 0`` are filled from the voiced frames around them; frame 0 and frame T-1 hold the first and the last voiced value.
    ``kind``: "slinear" / "linear", "previous" / "zero", "next", "nearest", "nearest-up" (``ValueError`` otherwise: the spline
    kinds of order 2 and above are global solves and not provided).  Linear values agree with SciPy's within 8 ulp of the larger
    knot in float64 and 1 ulp in float32; the step kinds are equal bit for bit.  A track of one frame is returned as it is
    (the reference raises from SciPy when that frame is voiced).

    numpy in, numpy out through the device: one copy in, one launch, one copy out.  A CUDA tensor is accepted and a tensor
    returned, with no synchronisation."""
    torch = _hip.torch_mod()
    is_tensor = torch.is_tensor(f0)
    if not is_tensor:
        f0 = np.asarray(f0)
    nd = f0.dim() if is_tensor else f0.ndim
    size = f0.numel() if is_tensor else f0.size
    if nd == 0 or len(f0) != size:
        raise RuntimeError("1d array is only supported")
    k = _f0_hip.kind_of(kind)
    if is_tensor and not f0.is_cuda:
        return torch.from_numpy(interp1d(f0.numpy(), kind))
    if is_tensor:
        if f0.dtype not in (torch.float32, torch.float64):
            raise ValueError("interp1d: float32 or float64 tensors only, got %s" % f0.dtype)
        _hip.require_gpu(f0.device)
        y = torch.empty(f0.shape, dtype=f0.dtype, device=f0.device)
        _f0_hip.interp(f0.reshape(1, -1, 1), None, k, y.view(1, -1, 1), None)
        return y
    dev = _hip.require_gpu()
    xt = torch.from_numpy(np.ascontiguousarray(f0.astype(_float_dtype(f0), copy=False)).reshape(1, -1, 1)).to(dev)
    y, _ = _f0_hip.interp(xt, None, k, torch.empty_like(xt), None)
    return y.cpu().numpy().reshape(f0.shape).astype(f0.dtype, copy=False)


def interp1d_batch(X, lengths=None, kind="slinear", out=None, vuv=None, return_vuv=False):
    """:func:`interp1d` on every column of every utterance of a padded batch, in one launch.

    ``X``: ``(B, Tmax, C)`` or ``(B, Tmax)``, numpy (numpy out) or a float32 / float64 CUDA tensor (a tensor out, no
    synchronisation); a column slice of a wider tensor is fine.  ``lengths``: one integer per utterance, clamped to
    ``[0, Tmax]`` (None: ``Tmax`` each); frames at or past them are not read and come out as zeros.  ``out`` (tensors only):
    where the result goes, float32 or float64, of ``X``'s shape; ``out=X`` fills in place.  ``vuv`` (tensors only): a tensor of
    ``X``'s shape that receives the flag, 1 where the ORIGINAL ``X > 0`` and 0 elsewhere; ``return_vuv=True`` allocates one.
    Returns the filled batch, or ``(filled, vuv)`` when the flag was asked for.  Argument errors are ``ValueError``s raised
    before any device work.  There is no host fallback: without the extension or a GPU the call raises ``HipExtensionError``."""
    torch = _hip.torch_mod()
    k = _f0_hip.kind_of(kind)
    is_tensor = torch.is_tensor(X)
    if not is_tensor:
        X = np.asarray(X)
    nd = X.dim() if is_tensor else X.ndim
    if nd not in (2, 3):
        raise ValueError("interp1d_batch: X must be (B, Tmax, C) or (B, Tmax), got %d dimensions" % nd)
    B = X.shape[0]
    if lengths is not None:
        if torch.is_tensor(lengths):
            bad = lengths.dtype not in (torch.int32, torch.int64) or tuple(lengths.shape) != (B,)
        else:
            lengths = np.asarray(lengths)
            bad = lengths.dtype.kind not in "iu" or lengths.shape != (B,)
        if bad:
            raise ValueError("interp1d_batch: lengths must hold one integer per utterance (B = %d)" % B)
    for name, t in (("out", out), ("vuv", vuv)):
        if t is not None and not (torch.is_tensor(t) and tuple(t.shape) == tuple(X.shape) and t.dtype in (torch.float32, torch.float64)):
            raise ValueError("interp1d_batch: %s must be a float32 / float64 CUDA tensor of X's shape %s" % (name, tuple(X.shape)))
    if not is_tensor or not X.is_cuda:
        if out is not None or vuv is not None:
            raise ValueError("interp1d_batch: out= and vuv= are for CUDA tensors")
        if is_tensor:
            res = interp1d_batch(X.numpy(), lengths, kind, None, None, return_vuv)
            return tuple(torch.from_numpy(r) for r in res) if return_vuv else torch.from_numpy(res)
        dev = _hip.require_gpu()
        xt = torch.from_numpy(np.ascontiguousarray(X.astype(_float_dtype(X), copy=False))).to(dev)
        res = interp1d_batch(xt, lengths, kind, None, None, return_vuv)
        if return_vuv:
            return tuple(r.cpu().numpy().astype(X.dtype, copy=False) for r in res)
        return res.cpu().numpy().astype(X.dtype, copy=False)
    if X.dtype not in (torch.float32, torch.float64):
        raise ValueError("interp1d_batch: float32 or float64 tensors only, got %s" % X.dtype)
    for name, t in (("out", out), ("vuv", vuv)):
        if t is not None and not (t.is_cuda and t.device == X.device):
            raise ValueError("interp1d_batch: %s must be on X's device" % name)
    dev = _hip.require_gpu(X.device)
    if out is None:
        out = torch.empty(X.shape, dtype=X.dtype, device=dev)
    want_flag = vuv is not None or return_vuv
    if vuv is None and return_vuv:
        vuv = torch.empty(X.shape, dtype=X.dtype, device=dev)
    x3, y3, v3 = ((t if nd == 3 else t.unsqueeze(-1)) if t is not None else None for t in (X, out, vuv))
    _f0_hip.interp(x3, _device_lengths(lengths, B, dev, "interp1d_batch"), k, y3, v3)
    return (out, vuv) if want_flag else out
