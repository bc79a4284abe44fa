"""Padded-batch glue around the hot path.

Mirrors ``apply_each2d_trim`` / ``apply_each2d_padded`` of /root/reference/nnmnkwii/util/__init__.py:19-66:
apply a ``(T, D) -> (T', D')`` function to every utterance of a zero-padded ``(N, Tmax, D)`` array and
collect the results in a zero-padded ``(N, Tmax, D')`` float64 array.  When the function is one of this
package's batched operations (``paramgen.mlpg``, ``preprocessing.delta_features``,
``postfilters.merlin_post_filter``, ``postfilters.modspec_post_filter``, ``preprocessing.modspec_smoothing``,
``preprocessing.scale`` / ``inv_scale`` / ``minmax_scale`` / ``inv_minmax_scale``, ``preprocessing.interp1d`` on batches
of one column) the whole batch goes
to the GPU in one call instead of N; any other callable is applied per utterance, as in the reference.
"""
import inspect

import numpy as np

from . import _hip
from . import postfilters as _pf
from .paramgen import _mlpg as _pg
from .preprocessing import f0 as _f0, generic as _gen
from .preprocessing.modspec import modspec_smoothing as _smoothing, modspec_smoothing_batch as _smoothing_batch


def _batched(func2d, X, lengths, args, kwargs):
    """One-launch equivalents of the per-utterance loop, or None if func2d is not one of ours."""
    if func2d is _pf.merlin_post_filter and len(args) <= 5:      # (alpha, minimum_phase_order, fftlen, coef, weight)
        return _pf.merlin_post_filter_batch(X, *args, lengths=lengths, **kwargs)
    if func2d is _smoothing or func2d is _pf.modspec_post_filter:
        batch = _smoothing_batch if func2d is _smoothing else _pf.modspec_post_filter_batch
        try:
            bound = inspect.signature(func2d).bind(None, *args, **kwargs)
        except TypeError:
            return None                  # the per-utterance call raises it
        bound.apply_defaults()
        kw = dict(bound.arguments)
        kw.pop("x")
        if X.shape[1] > int(kw["n"]):
            return None                  # utterances may still fit; the per-utterance path raises where one does not
        return batch(X, lengths=lengths, **kw)
    if func2d in (_gen.scale, _gen.inv_scale, _gen.minmax_scale, _gen.inv_minmax_scale) and not {"lengths", "out"} & set(kwargs):
        return func2d(X, *args, lengths=lengths, **kwargs)          # one mlpg_hip_column_affine launch
    if func2d is _f0.interp1d and X.shape[2] == 1 and len(args) + len(kwargs) <= 1 and set(kwargs) <= {"kind"}:
        # (the reference's interp1d takes one column; on a wider batch the per-utterance path raises its RuntimeError)
        return _f0.interp1d_batch(X, lengths, *args, **kwargs)      # one nnmk_f0_interp launch
    if kwargs:
        return None
    if func2d is _pg.mlpg and len(args) == 2:
        variances, windows = args
        variances = np.asarray(variances)
        if variances.ndim != 1:          # per-utterance (T, D) variances cannot be shared by the batch
            return None
        return _pg.mlpg_batch(X, variances, windows, lengths=lengths)
    if func2d is _gen.delta_features and len(args) == 1:
        torch = _hip.torch_mod()
        dev = _hip.require_gpu()
        Xf = np.ascontiguousarray(X if X.dtype in (np.float32, np.float64) else X.astype(np.float64))
        win = [_gen._same_window(w[2] if isinstance(w, tuple) else w) for w in args[0]]
        if len(lengths) and int(np.min(lengths)) < max(len(w[2]) for w in win):
            return None                  # np.correlate swaps its operands there; the per-utterance path raises
        out = _hip.delta_features(torch.from_numpy(Xf).to(dev), win,
                                  torch.as_tensor(np.asarray(lengths), dtype=torch.int32, device=dev))
        return out.cpu().numpy()
    return None


def apply_each2d_padded(func2d, X, lengths, *args, **kwargs):
    """Apply ``func2d`` to ``X[n][:lengths[n]]`` for every n (util/__init__.py:44-66)."""
    assert X.ndim == 3
    N, T, _ = X.shape
    lengths = np.asarray(lengths)
    fast = _batched(func2d, X, lengths, args, kwargs)
    if fast is not None:
        return fast.astype(np.float64, copy=False)      # the reference collects into np.zeros (float64)
    y = func2d(X[0][: lengths[0]], *args, **kwargs)
    assert y.ndim == 2
    Y = np.zeros((N, T, y.shape[1]))
    Y[0][: len(y)] = y
    for idx in range(1, N):
        y = func2d(X[idx][: lengths[idx]], *args, **kwargs)
        Y[idx][: len(y)] = y
    return Y


def apply_each2d_trim(func2d, X, *args, **kwargs):
    """Apply ``func2d`` to every utterance with its trailing zero frames removed (util/__init__.py:19-41).
    The trim of the whole batch is one ``mlpg_hip_trim_lengths`` launch."""
    assert X.ndim == 3
    torch = _hip.torch_mod()
    dev = _hip.require_gpu()
    Xf = np.ascontiguousarray(X if X.dtype in (np.float32, np.float64) else X.astype(np.float64))
    lengths = _hip.trim_lengths(torch.from_numpy(Xf).to(dev)).cpu().numpy()
    return apply_each2d_padded(func2d, X, lengths, *args, **kwargs)
