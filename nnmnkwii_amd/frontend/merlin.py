"""Frame-level linguistic features from phone-level ones and durations: the part of the reference's
``nnmnkwii.frontend.merlin.linguistic_features(..., add_frame_features=True, subphone_features=...)`` that depends on the
durations, on the device (include/nnmnkwii_frontend.h, csrc/frame_expand.hip; tools/frontend_model.py is the
executable specification).

The part that needs text -- the question set's regular expressions -- does not depend on the durations: it gives one
``(N, Dl)`` matrix per utterance (the reference's ``linguistic_features(labels, binary_dict, numeric_dict,
add_frame_features=False, subphone_features=None)``) and is an INPUT here, computed once, anywhere.  ``frame_features`` and
``frame_features_batch`` take it together with durations ``(N, S)`` in frames -- ``S`` states per phone, 1 for a phone
alignment -- as a duration model predicts them, and write one row per frame: the phone's row followed by the sub-phone
columns, bit for bit what the reference computes (float64 arithmetic, one rounding to the output's dtype), optionally followed
by the reference's ``minmax_scale(F, scale_=, min_=)`` in the same pass.  Every kind is defined for every ``S``; the reference
refuses some combinations only because of which of its two label loaders they came through.

Durations: floating-point ones are rounded half to even (``np.round``), integers are taken as they are; then anything not
greater than ``min_frames`` (NaN included) becomes ``min_frames``.  ``min_frames`` defaults to 1 for floating-point durations
(the Merlin recipe's ``<= 0 -> 1``) and to 0 for integers.  States and phones of 0 frames give no rows.

There is no CPU route: numpy arrays and CPU tensors are copied to the device and the result back; without the built library
or a GPU the functions raise ``HipExtensionError``.  CUDA tensors are used where they lie."""
import numpy as np

from .. import _frontend_hip as FH
from .. import _silence_hip as SH

_CC_DEVICE = {}     # device index -> the coarse-coding table on that device


def _kind(subphone_features):
    if subphone_features is None:
        return FH.NONE
    if not isinstance(subphone_features, str):
        raise ValueError("Unknown value for subphone_features: %r" % (subphone_features,))
    name = subphone_features.strip().lower()
    if name == "none":
        raise ValueError("subphone_features = 'none' is deprecated, use None instead")
    if name not in FH.KINDS:
        raise ValueError("Unknown value for subphone_features: %s" % (name,))
    return FH.KINDS.index(name)


def get_frame_feature_size(subphone_features="full"):
    """The number of sub-phone columns of a kind: the reference's function, its ``ValueError`` for ``"none"`` and for unknown
    names included."""
    return FH.SIZES[_kind(subphone_features)]


def coarse_coding_table():
    """The reference's ``compute_coarse_coding_features()``: three normal densities (sigma 0.4; mu 0, 0.5 and 1) on 600 points
    each, float64 ``(3, 600)``, from the closed form with numpy (the same bits as the reference's scipy table)."""
    cc = np.zeros((3, FH.CC_POINTS))
    for k, (lo, hi, mu) in enumerate(((-1.5, 1.5, 0.0), (-1.0, 2.0, 0.5), (-0.5, 2.5, 1.0))):
        z = (np.linspace(lo, hi, FH.CC_POINTS) - mu) / 0.4
        cc[k] = np.exp(-z ** 2 / 2.0) / np.sqrt(2 * np.pi) / 0.4
    return cc


def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "is_cuda")


def _shape_dtype(a, name):
    """(shape, numpy dtype kind and itemsize) of a numpy array or tensor."""
    if _is_tensor(a):
        kind = "f" if a.dtype.is_floating_point else ("i" if not a.dtype.is_complex and str(a.dtype) != "torch.bool" else "?")
        return tuple(a.shape), kind, a.element_size()
    a = np.asarray(a)
    return a.shape, a.dtype.kind, a.dtype.itemsize


def _validate(phone_features, durations, num_phones, subphone_features, min_frames, scale_, min_, Tmax, out, dtype, who, ndim):
    """Everything that can be refused from shapes and dtypes alone -- before any device work.  Returns (kind, min_frames, output
    numpy dtype)."""
    kind = _kind(subphone_features)
    (ps, pk, pz), (ds, dk, dz) = _shape_dtype(phone_features, "phone_features"), _shape_dtype(durations, "durations")
    want = "(N, Dl) and (N, S)" if ndim == 2 else "(B, Nmax, Dl) and (B, Nmax, S)"
    if len(ps) != ndim or len(ds) != ndim or ps[:-1] != ds[:-1]:
        raise ValueError("%s: phone_features and durations must be %s, got %s and %s" % (who, want, ps, ds))
    if pk != "f" or pz not in (4, 8):
        raise ValueError("%s: phone_features must be float32 or float64" % who)
    if dk not in "fiu" or (dk == "f" and dz not in (4, 8)):
        raise ValueError("%s: durations must be integers, float32 or float64" % who)
    S = ds[-1]
    if not 1 <= S <= FH.MAX_S:
        raise ValueError("%s: S (states per phone, the durations' last dimension) must be in 1 .. %d, got %d" % (who, FH.MAX_S, S))
    if ds[-2] * S > FH.MAX_STATES:
        raise ValueError("%s: %d phones x %d states, at most %d states fit one utterance" % (who, ds[-2], S, FH.MAX_STATES))
    mf = (1 if dk == "f" else 0) if min_frames is None else int(min_frames)
    if mf < 0:
        raise ValueError("%s: min_frames must be at least 0, got %d" % (who, mf))
    W = ps[-1] + FH.SIZES[kind]
    if (scale_ is None) != (min_ is None):
        raise ValueError("%s: scale_ and min_ go together" % who)
    for name, t in (("scale_", scale_), ("min_", min_)):
        if t is not None and tuple(t.shape) != (W,):
            raise ValueError("%s: %s must have one value per output column (%d), got shape %s" % (who, name, W, tuple(t.shape)))
    if num_phones is not None and tuple(num_phones.shape if hasattr(num_phones, "shape") else np.shape(num_phones)) != (ps[0],):
        raise ValueError("%s: num_phones must have one entry per utterance (%d)" % (who, ps[0]))
    if Tmax is not None and int(Tmax) < 0:
        raise ValueError("%s: Tmax must be at least 0, got %d" % (who, Tmax))
    if dtype is None:
        odt = np.dtype(np.float32 if pz == 4 else np.float64)
    else:
        odt = np.dtype({"torch.float32": np.float32, "torch.float64": np.float64}.get(str(dtype), dtype))
        if odt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("%s: dtype must be float32 or float64, got %s" % (who, dtype))
    if out is not None:
        if not (_is_tensor(out) and out.dim() == 3 and out.shape[0] == ps[0]):
            raise ValueError("%s: out must be a (B, Tmax, Dl + F) tensor" % who)
        if out.shape[2] != W:
            raise ValueError("%s: out has %d columns, the features have %d (Dl = %d, %d sub-phone columns)" % (who, out.shape[2], W, ps[-1], W - ps[-1]))
        if Tmax is not None and int(Tmax) != out.shape[1]:
            raise ValueError("%s: Tmax = %d but out has %d rows per utterance" % (who, Tmax, out.shape[1]))
        if dtype is not None and np.dtype(str(out.dtype).replace("torch.", "")) != odt:
            raise ValueError("%s: out is %s, dtype asks for %s" % (who, out.dtype, odt))
        if not out.is_cuda:
            raise ValueError("%s: out must be a CUDA tensor" % who)
    return kind, mf, odt


def _validate_silence(silence, durations, who, ndim):
    """The flags: one bool or integer per phone."""
    if _is_tensor(silence):
        shape, ok = tuple(silence.shape), not (silence.dtype.is_floating_point or silence.dtype.is_complex)
    else:
        silence = np.asarray(silence)
        shape, ok = silence.shape, silence.dtype.kind in "biu"
    want = tuple(durations.shape[:-1])
    if not ok or shape != want:
        raise ValueError("%s: silence must hold one bool or integer flag per phone, %s, got shape %s"
                         % (who, "(N,)" if ndim == 2 else "(B, Nmax)", shape))


def _to_device(a, dev, torch, dtype=None):
    if a is None:
        return None
    t = a if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype) if dtype is not None else t.to(dev)


def _cc_on(dev, torch):
    t = _CC_DEVICE.get(dev.index)
    if t is None:
        t = _CC_DEVICE[dev.index] = torch.from_numpy(coarse_coding_table()).to(dev)
    return t


def _batch(who, phone_features, durations, num_phones, subphone_features, silence, min_frames, scale_, min_, Tmax, out, dtype, strict):
    """frame_features_batch (silence None) and kept_frame_features_batch: validation, placement, the counts where they are
    needed, one launch."""
    kind, mf, odt = _validate(phone_features, durations, num_phones, subphone_features, min_frames, scale_, min_, Tmax, out, dtype, who, 3)
    if silence is not None:
        _validate_silence(silence, durations, who, 3)
    from .. import _hip
    as_tensor = _is_tensor(phone_features)
    on_device = as_tensor and phone_features.is_cuda
    dev = _hip.require_gpu(phone_features.device if on_device else (out.device if out is not None else None))
    torch = _hip.torch_mod()
    P = _to_device(phone_features, dev, torch)
    if _is_tensor(durations):
        d = durations if durations.dtype in (torch.int32, torch.int64, torch.float32, torch.float64) else durations.to(torch.int64)
    else:
        d = np.ascontiguousarray(durations)
        d = torch.from_numpy(d if d.dtype in (np.int32, np.int64, np.float32, np.float64) else d.astype(np.int64))
    d = d.to(dev).contiguous()
    sil = None if silence is None else (_to_device(silence if _is_tensor(silence) else np.asarray(silence) != 0, dev, torch) != 0).contiguous()
    n = _to_device(num_phones if num_phones is None or _is_tensor(num_phones) else np.asarray(num_phones), dev, torch, torch.int32)
    sc, mn = _to_device(scale_, dev, torch, torch.float64), _to_device(min_, dev, torch, torch.float64)
    B, W = P.shape[0], P.shape[2] + FH.SIZES[kind]
    T = out.shape[1] if out is not None else Tmax
    if T is None or strict:
        counts = (FH.frame_counts(d, n, mf) if sil is None else SH.frame_counts(d, n, sil, mf)[:, 0]).cpu().numpy()
        if T is None:
            T = int(counts.max()) if B else 0
        elif (counts > int(T)).any():
            b = int(np.argmax(counts > int(T)))
            raise ValueError("%s: utterance %d has %d %sframes, Tmax is %d" % (who, b, counts[b], "" if sil is None else "kept ", int(T)))
    if out is None:
        out = torch.empty((B, int(T), W), dtype=torch.float32 if odt == np.float32 else torch.float64, device=dev)
    cc = _cc_on(dev, torch) if kind == FH.COARSE_CODING else None
    sc, mn = None if sc is None else sc.contiguous(), None if mn is None else mn.contiguous()
    lengths = FH.expand(P, d, n, kind, mf, cc, sc, mn, out) if sil is None else SH.expand(P, d, n, sil, kind, mf, cc, sc, mn, out)
    if on_device:
        return out, lengths
    if as_tensor:
        return out.cpu(), lengths.cpu()
    return out.cpu().numpy(), lengths.cpu().numpy()


def frame_features_batch(phone_features, durations, num_phones=None, subphone_features="full", *, min_frames=None, scale_=None, min_=None,
                         Tmax=None, out=None, dtype=None, strict=True):
    """A padded batch in one launch.  phone_features ``(B, Nmax, Dl)`` float32 / float64, durations ``(B, Nmax, S)`` (int32,
    int64, float32 or float64), num_phones ``(B)`` or None (every utterance has Nmax phones).  Returns ``(out, lengths)``:
    out ``(B, Tmax, Dl + F)`` with zeros behind each utterance's frames, lengths int32 ``(B)``.

    scale_, min_ ``(Dl + F)``: every value becomes ``v * scale_[c] + min_[c]`` in float64 (the reference's
    ``minmax_scale(F, scale_=, min_=)``) before the one rounding to the output's dtype.  dtype: float32 or float64 (None:
    phone_features' own).  out: a CUDA tensor to write into, ``(B, Tmax, Dl + F)``; a column slice of a wider dense tensor is
    fine, and its other columns are not touched.

    If neither Tmax nor out is given the frame counts are computed first and their maximum read back: one synchronisation.  If
    one is given, ``strict=True`` reads the counts back too and raises ``ValueError`` naming the first utterance that does not
    fit; ``strict=False`` synchronises nothing (for stream capture) and truncation shows only in ``lengths``, which are then
    ``Tmax``."""
    return _batch("frame_features_batch", phone_features, durations, num_phones, subphone_features, None, min_frames, scale_, min_, Tmax, out,
                  dtype, strict)


def frame_features(phone_features, durations, subphone_features="full", *, min_frames=None, scale_=None, min_=None, dtype=None):
    """One utterance: phone_features ``(N, Dl)`` and durations ``(N, S)`` in, ``(T, Dl + F)`` out, T the sum of the durations in
    frames -- what the reference's ``linguistic_features(labels, binary_dict, numeric_dict, subphone_features=...,
    add_frame_features=True)`` returns for labels with these durations.  Takes numpy arrays or tensors and returns the same
    kind; the keywords are those of ``frame_features_batch``."""
    _validate(phone_features, durations, None, subphone_features, min_frames, scale_, min_, None, None, dtype, "frame_features", 2)
    out, _ = frame_features_batch(phone_features[None], durations[None], None, subphone_features, min_frames=min_frames, scale_=scale_, min_=min_,
                                  dtype=dtype)
    return out[0]


def kept_frame_features_batch(phone_features, durations, silence, num_phones=None, subphone_features="full", *, min_frames=None, scale_=None,
                              min_=None, Tmax=None, out=None, dtype=None, strict=True):
    """:func:`frame_features_batch` without the frames of silent phones, in one launch: the reference's

        X = linguistic_features(labels, binary_dict, numeric_dict, add_frame_features=True, subphone_features=...)
        X = np.delete(X, labels.silence_frame_indices(regex), axis=0)

    for every utterance of a padded batch (include/nnmnkwii_silence.h, csrc/frame_keep.hip).  The regular
    expression is text processing and gives one flag per phone, computed once, anywhere:

        sil = np.zeros(N, bool); sil[labels.silence_phone_indices(regex)] = True

    silence ``(B, Nmax)``: bool or integers, non-zero: the phone is silent and none of its frames is written (or computed).  The
    sub-phone columns of the kept frames come from their places in the original phones.  Everything else is
    :func:`frame_features_batch`'s, with ``K_b`` -- the frames of utterance ``b`` whose phone is not flagged -- in the place of
    ``T_b``: out ``(B, Tmax, Dl + F)`` has zeros behind each utterance's ``K_b`` kept rows, lengths are ``min(K_b, Tmax)``,
    ``Tmax=None`` reads the largest ``K_b`` back, and ``strict=True`` raises ``ValueError`` naming the first utterance whose
    kept frames do not fit.  Flags at or past ``num_phones[b]`` are not read."""
    return _batch("kept_frame_features_batch", phone_features, durations, num_phones, subphone_features, silence, min_frames, scale_, min_, Tmax,
                  out, dtype, strict)


def kept_frame_features(phone_features, durations, silence, subphone_features="full", *, min_frames=None, scale_=None, min_=None, dtype=None):
    """One utterance: :func:`frame_features` without the frames of the phones flagged in silence ``(N,)`` -- ``(K, Dl + F)``, what
    ``np.delete(linguistic_features(..., add_frame_features=True), labels.silence_frame_indices(regex), axis=0)`` returns for
    labels with these durations and ``sil = np.zeros(N, bool); sil[labels.silence_phone_indices(regex)] = True``."""
    who = "kept_frame_features"
    _validate(phone_features, durations, None, subphone_features, min_frames, scale_, min_, None, None, dtype, who, 2)
    _validate_silence(silence, durations, who, 2)
    silence = silence if _is_tensor(silence) else np.asarray(silence)
    out, _ = kept_frame_features_batch(phone_features[None], durations[None], silence[None], None, subphone_features, min_frames=min_frames,
                                       scale_=scale_, min_=min_, dtype=dtype)
    return out[0]
