"""Post-filters on the synthesis path (mirror of nnmnkwii/postfilters/__init__.py:7-62).

``merlin_post_filter`` is the step Merlin-style pipelines run between ``multi_stream_mlpg`` and the vocoder: it emphasises the
formants of mel-cepstra and puts the frame's energy back.  The reference walks the frames on the host through ``pysptk``;
here the whole array goes through one launch of ``mlpg_hip_merlin_post_filter`` (csrc/postfilter.hip).  The
four SPTK operations are restated from their published definitions (tools/postfilter_model.py is the executable specification);
parity with the ``pysptk`` package itself is unpinned: it is pinned wherever that package is installed
(tests/test_postfilter_model.py::test_against_pysptk_when_installed).
"""
import numpy as np

from . import _hip


def _weight(D, coef, weight):
    if weight is None:
        w = np.ones(D, dtype=np.float64) * coef
        w[:2] = 1.0
        return w
    w = np.ascontiguousarray(weight, dtype=np.float64)
    if w.shape != (D,):
        raise ValueError("merlin_post_filter: weight must hold one value per coefficient (D = %d), got shape %s" % (D, w.shape))
    return w


def merlin_post_filter_batch(mgc, alpha, minimum_phase_order=511, fftlen=1024, coef=1.4, weight=None, lengths=None, out=None):
    """``merlin_post_filter`` over a padded batch ``(B, Tmax, D)`` in one launch.

    ``mgc``: a numpy array (float32 / float64; other dtypes are computed as float64) or a CUDA tensor (float32 / float64).  A
    tensor may be a slice of the last dimension of a wider dense tensor -- ``Y[..., 10:70]`` is filtered where it lies.
    ``lengths``: utterance b's frames at or past ``min(max(lengths[b], 0), Tmax)`` are never read and come out as exact zeros.
    ``out`` (tensors only): where the result goes; ``out=mgc`` filters in place.  Returns what it was given: numpy for numpy (a new
    array), a tensor on the same device for a tensor.
    """
    torch = _hip.torch_mod()
    is_tensor = torch.is_tensor(mgc)
    if not is_tensor:
        mgc = np.asarray(mgc)
    if mgc.ndim != 3:
        raise ValueError("merlin_post_filter_batch: mgc must be (B, Tmax, D), got %d dimensions" % mgc.ndim)
    B, T, D = (int(n) for n in mgc.shape)
    alpha, order, fftlen = float(alpha), int(minimum_phase_order), int(fftlen)
    _hip.postfilter_check(D, alpha, order, fftlen)
    w = _weight(D, coef, weight)
    if is_tensor:
        if not mgc.is_cuda:
            if out is not None:
                raise ValueError("merlin_post_filter_batch: out= is for CUDA tensors")
            dev = _hip.require_gpu()
            return merlin_post_filter_batch(mgc.to(dev), alpha, order, fftlen, coef, weight, lengths).to(mgc.device)
        if mgc.dtype not in (torch.float32, torch.float64):
            raise ValueError("merlin_post_filter: float32 or float64 tensors only, got %s" % mgc.dtype)
        dev = _hip.require_gpu(mgc.device)
        x = mgc
    else:
        if out is not None:
            raise ValueError("merlin_post_filter_batch: out= is for CUDA tensors")
        dev = _hip.require_gpu()
        xf = mgc if mgc.dtype in (np.float32, np.float64) else mgc.astype(np.float64)
        x = torch.from_numpy(np.ascontiguousarray(xf)).to(dev)
    if lengths is not None:
        if not torch.is_tensor(lengths):
            lengths = torch.from_numpy(np.asarray(lengths).astype(np.int32))
        lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
        if lengths.shape != (B,):
            raise ValueError("merlin_post_filter_batch: lengths must hold one value per utterance (B = %d)" % B)
    G = _hip.postfilter_table(dev, D, alpha, order, fftlen)
    y = _hip.merlin_post_filter(x, alpha, torch.from_numpy(w).to(dev), G, fftlen, lengths=lengths, out=out if is_tensor else x)
    if is_tensor:
        return y
    return y.cpu().numpy().astype(mgc.dtype if mgc.dtype in (np.float32, np.float64) else np.float64, copy=False)


def merlin_post_filter(mgc, alpha, minimum_phase_order=511, fftlen=1024, coef=1.4, weight=None):
    """Merlin's post-filter for mel-cepstra, ``(T, D) -> (T, D)``.

    Drop-in for ``nnmnkwii.postfilters.merlin_post_filter`` (same signature and defaults).  numpy in, numpy out, float32 and
    float64 keep their dtype (the arithmetic is float64 either way).  A CUDA tensor is filtered IN PLACE and returned.
    Limits (``ValueError`` outside them): ``1 <= D <= 64``, ``fftlen`` a power of two in ``[4, 4096]``,
    ``D - 1 <= minimum_phase_order < fftlen``, ``|alpha| < 1``; ``weight``, if given, holds ``D`` values.
    """
    torch = _hip.torch_mod()
    if torch.is_tensor(mgc):
        if mgc.dim() != 2:
            raise ValueError("merlin_post_filter: mgc must be (T, D), got %d dimensions" % mgc.dim())
        if mgc.is_cuda:
            merlin_post_filter_batch(mgc[None], alpha, minimum_phase_order, fftlen, coef, weight, out=mgc[None])
            return mgc
        return merlin_post_filter_batch(mgc[None], alpha, minimum_phase_order, fftlen, coef, weight)[0]
    mgc = np.asarray(mgc)
    if mgc.ndim != 2:
        raise ValueError("merlin_post_filter: mgc must be (T, D), got %d dimensions" % mgc.ndim)
    return merlin_post_filter_batch(mgc[None], alpha, minimum_phase_order, fftlen, coef, weight)[0]
