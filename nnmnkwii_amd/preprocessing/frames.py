"""Zero-frame removal and the joint feature rows of a voice-conversion recipe on the device (mirror of ``remove_zeros_frames``,
nnmnkwii/preprocessing/generic.py:335-356, and of the composition around it; csrc/joint_rows.hip, DESIGN.md K17;
tools/joint_model.py is the specification).

    aligner = DTWAligner()
    Xa, Ya = aligner.transform((X, Y))                                           # CUDA tensors in, CUDA tensors out
    rows = joint_features_batch(Xa[:, :, 1:], Ya[:, :, 1:], aligner.path_lengths_, windows)
    gmm = fit_gaussian_mixture(rows, n_components)
"""
import numpy as np
import torch

from .. import _hip, _joint_hip
from .generic import _same_window

_NP_OF = {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64)}


class JointRows(object):
    """What :func:`joint_features_batch` returns when it was given ``out``: nothing has been synchronised yet.

    ``out`` is the caller's tensor of ``cap`` rows, ``offsets`` the device int64 ``(B + 1)`` tensor (``offsets[B] = N``).
    ``n`` reads ``N`` back (once: this is the synchronisation) and raises ``ValueError`` if ``N > cap`` -- the rows past ``cap``
    were NOT written; count again with a larger ``out``.  ``rows`` is ``out[:n]``."""

    def __init__(self, out, offsets):
        self.out, self.offsets, self._n = out, offsets, None

    @property
    def n(self):
        if self._n is None:
            n = int(self.offsets[-1].item())
            if n > self.out.shape[0]:
                raise ValueError("joint rows: %d rows were kept but out holds %d: the rows past its capacity were not written" % (n, self.out.shape[0]))
            self._n = n
        return self._n

    @property
    def rows(self):
        return self.out[:self.n]

    def __len__(self):
        return self.n


def _as_windows(windows):
    if windows is None or len(windows) == 0:
        return []
    return [_same_window(w[2] if isinstance(w, tuple) else w) for w in windows]


def _one_lengths(who, n, B):
    if n is None:
        return None
    if torch.is_tensor(n):
        bad = n.dtype not in (torch.int32, torch.int64) or tuple(n.shape) != (B,)
    else:
        n = np.asarray(n)
        bad = n.dtype.kind not in "iu" or n.shape != (B,)
    if bad:
        raise ValueError("%s: lengths must hold one integer per utterance (B = %d)" % (who, B))
    return n


def _split_lengths(who, lengths, B, two):
    """(len_x, len_y): `lengths` is one (B) vector for both sources or a pair of them."""
    first = lengths[0] if isinstance(lengths, (tuple, list)) and len(lengths) == 2 else 0
    if first is None or (first.dim() if torch.is_tensor(first) else np.ndim(first)) == 1:
        if not two:
            raise ValueError("%s: a pair of lengths goes with two sources" % who)
        return _one_lengths(who, lengths[0], B), _one_lengths(who, lengths[1], B)
    n = _one_lengths(who, lengths, B)
    return n, n


def _to_device(n, dev):
    if n is None:
        return None
    if not torch.is_tensor(n):
        n = torch.from_numpy(np.ascontiguousarray(n).astype(np.int32))
    return n.to(device=dev, dtype=torch.int32).contiguous()


def _source(t):
    """The tensor itself where it is a last-axis slice of a dense (B, Tmax, ld) tensor, else a contiguous copy."""
    try:
        _joint_hip.check_source("x", t)
        return t
    except ValueError:
        return t.contiguous()


def _joint(who, X, Y, lengths, windows, eps, dtype, out, return_offsets):
    wins = _as_windows(windows)
    _joint_hip.pack_windows(wins)
    is_np = not torch.is_tensor(X)
    if Y is not None and torch.is_tensor(Y) == is_np:
        raise ValueError("%s: X and Y must both be numpy arrays or both be tensors" % who)
    if is_np:
        X = np.asarray(X)
        Y = None if Y is None else np.asarray(Y)
    for name, t in (("X", X), ("Y", Y)):
        if t is not None and (t.dim() if not is_np else t.ndim) != 3:
            raise ValueError("%s: %s must be (B, Tmax, D), got %d dimensions" % (who, name, t.dim() if not is_np else t.ndim))
    B, Tmax = X.shape[0], X.shape[1]
    if Y is not None and (Y.shape[0], Y.shape[1]) != (B, Tmax):
        raise ValueError("%s: X and Y must share B and Tmax, got %s and %s" % (who, tuple(X.shape), tuple(Y.shape)))
    len_x, len_y = _split_lengths(who, lengths, B, Y is not None)
    keep = _joint_hip.LIVE if eps is None else _joint_hip.NONZERO
    eps = 0.0 if eps is None else float(eps)
    if not eps >= 0.0:
        raise ValueError("%s: eps must be >= 0, got %r" % (who, eps))
    if not isinstance(dtype, torch.dtype):
        dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}.get(np.dtype(dtype), dtype)
    if dtype not in _NP_OF:
        raise ValueError("%s: dtype must be float32 or float64, got %r" % (who, dtype))
    W = (X.shape[2] + (0 if Y is None else Y.shape[2])) * max(len(wins), 1)
    if out is not None:
        if is_np or not X.is_cuda:
            raise ValueError("%s: out= is for CUDA tensors" % who)
        if not (torch.is_tensor(out) and out.dim() == 2 and out.shape[1] == W and out.dtype == dtype and out.device == X.device):
            raise ValueError("%s: out must be a (cap, %d) %s tensor on X's device" % (who, W, dtype))
    if is_np or not X.is_cuda:
        if not is_np:
            X, Y = X.numpy(), None if Y is None else Y.numpy()
        dev = _hip.require_gpu()
        Xd, Yd = (None if t is None else torch.from_numpy(np.ascontiguousarray(t if t.dtype in (np.float32, np.float64) else t.astype(np.float64))).to(dev)
                  for t in (X, Y))
        res = _joint(who, Xd, Yd, (len_x, len_y) if Yd is not None else len_x, wins, None if keep == _joint_hip.LIVE else eps, dtype, None, True)
        rows, offsets = (r.cpu().numpy() for r in res)
        if not is_np:
            rows, offsets = torch.from_numpy(rows), torch.from_numpy(offsets)
        return (rows, offsets) if return_offsets else rows
    for name, t in (("X", X), ("Y", Y)):
        if t is not None and (t.dtype not in _NP_OF or t.device != X.device):
            raise ValueError("%s: %s must be a float32 / float64 tensor on X's device" % (who, name))
    dev = _hip.require_gpu(X.device)
    plan, offsets = _joint_hip.count(_source(X), None if Y is None or Y.shape[2] == 0 else _source(Y), _to_device(len_x, dev),
                                     _to_device(len_y, dev) if Y is not None else None, wins, keep, eps, dtype)
    if out is not None:
        plan.write(out)
        res = JointRows(out, offsets)
    else:
        res = torch.empty((int(offsets[-1].item()), W), dtype=dtype, device=dev)      # the one synchronisation: the shape is data
        plan.write(res)
    return (res, offsets) if return_offsets else res


def joint_features_batch(X, Y, lengths, windows=None, *, eps=1e-7, dtype=torch.float64, out=None, return_offsets=False):
    """The joint rows of two padded batches: ``remove_zeros_frames(concatenate((delta_features(x_b), delta_features(y_b)), -1))`` over
    all utterances, in three launches and without a frame leaving the device.

    ``X``, ``Y``: ``(B, Tmax, Dx)`` / ``(B, Tmax, Dy)`` CUDA tensors (float32 / float64, independently) or numpy arrays (numpy out,
    through the device); ``Y`` may be None.  A last-axis slice of a wider tensor (``X[:, :, 1:]``) is used where it lies.
    ``lengths``: ``(B)`` for both sources, a pair ``(len_x, len_y)``, or None (``Tmax`` each); frames at or past a source's length
    are never read and count as zeros, also as the neighbours of a delta -- what ``apply_each2d_padded(delta_features, ...)`` leaves.
    ``windows``: as :func:`delta_features` takes them ((l, u, coef) triples or coefficient arrays); None: the frames themselves.
    ``eps``: a row is kept iff the float64 sum of its absolute values is ``> eps`` (the reference's rule); ``eps=None`` keeps every
    row below ``max(len_x[b], len_y[b])`` and reads no frame for the decision.  ``dtype``: of the rows.

    Returns the ``(N, W)`` rows, ``W = (Dx + Dy) * len(windows)``, in ``(b, t)`` order.  Without ``out`` the count is read back
    once (the shape is data) and exactly ``N`` rows are allocated.  With ``out``, a ``(cap, W)`` tensor of ``dtype``, nothing is
    synchronised: the result is a :class:`JointRows` whose ``rows`` / ``n`` read ``N`` when asked, and raise ``ValueError`` if
    ``N > cap`` (the rows past ``cap`` were not written).  ``return_offsets=True`` adds the int64 ``(B + 1)`` tensor of every
    utterance's first row, ``offsets[B] = N``.  Argument errors are ``ValueError``s raised before any device work.  There is no
    host fallback: without the extension or a GPU the call raises ``HipExtensionError``."""
    return _joint("joint_features_batch", X, Y, lengths, windows, eps, dtype, out, return_offsets)


def remove_zeros_frames_batch(X, lengths=None, eps=1e-7, *, out=None, return_offsets=False):
    """:func:`remove_zeros_frames` over a padded ``(B, Tmax, D)`` batch: the kept frames of all utterances as dense ``(N, D)`` rows of
    ``X``'s dtype.  Arguments and result as :func:`joint_features_batch` with one source and no windows."""
    who = "remove_zeros_frames_batch"
    if torch.is_tensor(X):
        if X.dtype not in _NP_OF:
            raise ValueError("%s: float32 or float64 tensors only, got %s" % (who, X.dtype))
        return _joint(who, X, None, lengths, None, eps, X.dtype, out, return_offsets)
    X = np.asarray(X)
    dt = X.dtype if X.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    res = _joint(who, X, None, lengths, None, eps, dt, out, return_offsets)
    return (res[0].astype(X.dtype, copy=False), res[1]) if return_offsets else res.astype(X.dtype, copy=False)


def remove_zeros_frames(x, eps=1e-7):
    """Remove all zero frames of a ``(T, D)`` feature matrix, trailing ones included.

    Drop-in for ``nnmnkwii.preprocessing.remove_zeros_frames`` (preprocessing/generic.py:335-356): a frame is kept iff
    ``sum_d |x| > eps``, the sum taken in float64.  numpy in, numpy out of the same dtype (a dtype other than float32 / float64 is
    computed in float64 and cast back); a tensor in, a tensor out on its device."""
    nd = x.dim() if torch.is_tensor(x) else np.ndim(x)
    if nd != 2:
        raise ValueError("remove_zeros_frames: x must be (T, D), got %d dimensions" % nd)
    if eps is None:
        raise ValueError("remove_zeros_frames: eps must be a number")
    return remove_zeros_frames_batch(x[None] if torch.is_tensor(x) else np.asarray(x)[None], None, eps)
