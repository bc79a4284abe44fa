"""Post-filters on the synthesis path (mirror of nnmnkwii/postfilters/__init__.py:7-62).

``merlin_post_filter`` is the step Merlin-style pipelines run between ``multi_stream_mlpg`` and the vocoder: it emphasises the
formants of mel-cepstra and puts the frame's energy back.  The reference walks the frames on the host through ``pysptk``;
here the whole array goes through one launch of ``mlpg_hip_merlin_post_filter`` (csrc/postfilter.hip).  The
four SPTK operations are restated from their published definitions (tools/postfilter_model.py is the executable specification);
parity with the ``pysptk`` package itself is unpinned: it is pinned wherever that package is installed
(tests/test_postfilter_model.py::test_against_pysptk_when_installed).

``modspec_post_filter`` / ``modspec_post_filter_batch`` are the modulation-spectrum post-filter (Takamichi et al., ICASSP 2014 /
TASLP 2016: the application the reference's ``preprocessing/modspec.py`` cites and does not contain), with
``modspec_log_stats`` and ``modspec_post_filter_tables`` for its statistics and tables: one launch of ``mlpg_hip_modspec_filter``
(csrc/modspec_filter.hip) per padded batch; tools/msfilter_model.py is the executable specification.
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


# ---- the modulation-spectrum post-filter (tools/msfilter_model.py is the executable specification) -------------
def _ms_mod():
    import importlib                                # (late: preprocessing imports the aligner; by name: the package re-exports a function `modspec`)
    return importlib.import_module(__package__ + ".preprocessing.modspec")


def modspec_log_stats(X, lengths=None, n=4096, norm=None):
    """Mean and population standard deviation (``ddof = 0``) of the log modulation spectrum over the utterances of a padded
    batch ``(B, Tmax, D)`` that have at least one live frame: ``(mean, std)``, each ``(n//2 + 1, D)`` float64, per (bin, column).
    Utterance b contributes ``x[b, :min(lengths[b], Tmax, n)]``.  numpy in, numpy out; CUDA tensor in, CUDA tensors out.  One
    ``modspec_batch`` call and torch reductions in float64: deterministic."""
    torch = _hip.torch_mod()
    ms_mod = _ms_mod()
    n = ms_mod._check_n(n)
    is_tensor = torch.is_tensor(X)
    dev = _hip.require_gpu(X.device if is_tensor and X.is_cuda else None)
    x = (X if is_tensor else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()
    if x.dim() != 3:
        raise ValueError("modspec_log_stats: X must be (B, Tmax, D), got %d dimensions" % x.dim())
    B, T, _ = x.shape
    if lengths is None:
        live = torch.full((B,), min(T, n), dtype=torch.int64, device=dev)
        lengths_d = None
    else:
        lengths_d = (lengths if torch.is_tensor(lengths) else torch.from_numpy(np.asarray(lengths).astype(np.int32)))
        lengths_d = lengths_d.to(device=dev, dtype=torch.int32).contiguous()
        if lengths_d.shape != (B,):
            raise ValueError("modspec_log_stats: lengths must hold one value per utterance (B = %d)" % B)
        live = lengths_d.to(torch.int64).clamp(0, min(T, n))
    keep = torch.nonzero(live > 0)[:, 0]
    if keep.numel() == 0:
        raise ValueError("modspec_log_stats: no utterance with a live frame")
    logms = torch.log(_hip.modspec_batch(x, n, ms_mod._norm_flag(norm), lengths=lengths_d).index_select(0, keep))
    mean = logms.mean(dim=0)
    std = (logms - mean).pow(2).mean(dim=0).sqrt()
    return (mean, std) if is_tensor else (mean.cpu().numpy(), std.cpu().numpy())


def modspec_post_filter_tables(gen_mean, gen_std, nat_mean, nat_std, k=0.85):
    """The tables of the MS post-filter ``s' = (1 - k) s + k [(sigma_N / sigma_G)(s - mu_G) + mu_N]`` on ``s = log MS``:
    ``A = 1 - k + k sigma_N / sigma_G`` and ``C = k (mu_N - (sigma_N / sigma_G) mu_G)``, float64, shaped like the statistics.
    An entry whose inputs are not all finite, or whose ``sigma_G <= 0``, is the identity (``A = 1, C = 0``).  numpy arrays or
    tensors (all four alike)."""
    torch = _hip.torch_mod()
    k = float(k)
    if torch.is_tensor(gen_mean):
        mg, sg, mn, sn = (t.to(torch.float64) for t in (gen_mean, gen_std, nat_mean, nat_std))
        ok = torch.isfinite(mg) & torch.isfinite(sg) & torch.isfinite(mn) & torch.isfinite(sn) & (sg > 0)
        ratio = sn / torch.where(ok, sg, torch.ones_like(sg))
        one, zero = torch.ones_like(mg), torch.zeros_like(mg)
        return torch.where(ok, 1.0 - k + k * ratio, one), torch.where(ok, k * (mn - ratio * mg), zero)
    mg, sg, mn, sn = (np.asarray(t, dtype=np.float64) for t in (gen_mean, gen_std, nat_mean, nat_std))
    ok = np.isfinite(mg) & np.isfinite(sg) & np.isfinite(mn) & np.isfinite(sn) & (sg > 0)
    with np.errstate(all="ignore"):
        ratio = sn / np.where(ok, sg, 1.0)
        return np.where(ok, 1.0 - k + k * ratio, 1.0), np.where(ok, k * (mn - ratio * mg), 0.0)


def modspec_post_filter_batch(X, A, C, n=4096, norm=None, lengths=None, modfs=None, cutoff=None, log_domain=True, out=None):
    """The MS post-filter, the low-pass smoothing of ``modspec_smoothing``, or both, over a padded batch ``(B, Tmax, D)`` in one
    launch (``mlpg_hip_modspec_filter``, csrc/modspec_filter.hip).

    Per utterance and column, with ``S = rfft(x[:live], n)`` and ``P = |S|^2``: bins below ``limit_bin`` get
    ``P' = exp(A log P + C)`` with the phase kept (a zero bin stays zero; ``A = C = None`` leaves them as they are); bins from
    ``limit_bin = min(int(n * cutoff / modfs) + 1, n//2 + 1)`` on are removed as ``modspec_smoothing`` removes them
    (``cutoff=None``: none); the result is ``irfft(S', n)[:live]``, exact zeros from ``live`` on.  ``A``, ``C``:
    ``(n//2 + 1, D)`` from :func:`modspec_post_filter_tables`.  ``X``: numpy (float32 / float64 keep their dtype) or a CUDA
    tensor (float32 / float64), possibly a slice of the last dimension of a wider dense tensor; ``out`` (tensors only), ``out=X``
    filters in place.  ``Tmax <= n`` (``RuntimeError`` otherwise); an even ``n`` (``ValueError``); a length that is no power of
    two or above 4096 is composed from the float64 calls."""
    ms_mod = _ms_mod()
    n = ms_mod._check_n(n)
    if (A is None) != (C is None):
        raise ValueError("modspec_post_filter: the tables A and C go together (both or neither)")
    if n % 2:
        raise ValueError("modspec_post_filter: the DFT length must be even (got %d)" % n)
    return ms_mod.filter_batch("modspec_post_filter", X, A, C, n, norm, lengths, ms_mod.limit_bin_of(n, modfs, cutoff), log_domain, out)


def modspec_post_filter(x, A, C, n=4096, norm=None, modfs=None, cutoff=None, log_domain=True):
    """:func:`modspec_post_filter_batch` for one trajectory, ``(T, D) -> (T, D)``.  numpy in, numpy out; a CUDA tensor is
    filtered IN PLACE and returned."""
    torch = _hip.torch_mod()
    if torch.is_tensor(x):
        if x.dim() != 2:
            raise ValueError("modspec_post_filter: x must be (T, D), got %d dimensions" % x.dim())
        if x.is_cuda:
            modspec_post_filter_batch(x[None], A, C, n, norm, None, modfs, cutoff, log_domain, out=x[None])
            return x
        return modspec_post_filter_batch(x[None], A, C, n, norm, None, modfs, cutoff, log_domain)[0]
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("modspec_post_filter: x must be (T, D), got %d dimensions" % x.ndim)
    return modspec_post_filter_batch(x[None], A, C, n, norm, None, modfs, cutoff, log_domain)[0]
