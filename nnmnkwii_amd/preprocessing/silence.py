"""Silence frames removed from any frame-level matrix on the device: the reference recipes'

    Y = np.delete(Y, labels.silence_frame_indices(regex), axis=0)

over padded batches (include/nnmnkwii_silence.h, csrc/frame_keep.hip; tools/silence_model.py is the
specification).  The regular expression is text processing and gives one flag per phone, computed once, anywhere:

    sil = np.zeros(N, bool); sil[labels.silence_phone_indices(regex)] = True

With the durations ``(N, S)`` in frames that ``frontend.merlin.frame_features`` takes, a frame is silent iff its phone is flagged.
``frontend.merlin.kept_frame_features_batch`` removes the same frames from the linguistic matrix while it writes it.

There is no CPU route: numpy arrays and CPU tensors are copied to the device and the result back; without the built library or
a GPU the functions raise ``HipExtensionError``.  CUDA tensors are used where they lie."""
import numpy as np

from .. import _frontend_hip as FH
from .. import _silence_hip as SH
from ..frontend.merlin import _is_tensor, _shape_dtype, _to_device, _validate_silence


def _validate(Y, durations, silence, lengths, num_phones, min_frames, Tmax, out, dtype, who, ndim):
    """Everything that can be refused from shapes and dtypes alone -- before any device work.  Returns (min_frames, output
    numpy dtype)."""
    (ys, yk, yz), (ds, dk, dz) = _shape_dtype(Y, "Y"), _shape_dtype(durations, "durations")
    if len(ys) != ndim or len(ds) != ndim or (ndim == 3 and ys[0] != ds[0]):
        raise ValueError("%s: the matrix and the durations must be %s, got %s and %s"
                         % (who, "(T, D) and (N, S)" if ndim == 2 else "(B, Tmax, D) and (B, Nmax, S)", ys, ds))
    if yk != "f" or yz not in (4, 8):
        raise ValueError("%s: the matrix must be float32 or float64" % who)
    if dk not in "fiu" or (dk == "f" and dz not in (4, 8)):
        raise ValueError("%s: durations must be integers, float32 or float64" % who)
    S = ds[-1]
    if not 1 <= S <= FH.MAX_S:
        raise ValueError("%s: S (states per phone, the durations' last dimension) must be in 1 .. %d, got %d" % (who, FH.MAX_S, S))
    if ds[-2] * S > FH.MAX_STATES:
        raise ValueError("%s: %d phones x %d states, at most %d states fit one utterance" % (who, ds[-2], S, FH.MAX_STATES))
    _validate_silence(silence, durations, who, ndim)
    mf = (1 if dk == "f" else 0) if min_frames is None else int(min_frames)
    if mf < 0:
        raise ValueError("%s: min_frames must be at least 0, got %d" % (who, mf))
    for name, v in (("lengths", lengths), ("num_phones", num_phones)):
        if v is not None and tuple(v.shape if hasattr(v, "shape") else np.shape(v)) != (ys[0],):
            raise ValueError("%s: %s must have one entry per utterance (%d)" % (who, name, ys[0]))
    if Tmax is not None and int(Tmax) < 0:
        raise ValueError("%s: Tmax must be at least 0, got %d" % (who, Tmax))
    if dtype is None:
        odt = np.dtype(np.float32 if yz == 4 else np.float64)
    else:
        odt = np.dtype({"torch.float32": np.float32, "torch.float64": np.float64}.get(str(dtype), dtype))
        if odt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("%s: dtype must be float32 or float64, got %s" % (who, dtype))
    if out is not None:
        if not (_is_tensor(out) and out.dim() == 3 and out.shape[0] == ys[0]):
            raise ValueError("%s: out must be a (B, Tmax, D) tensor" % who)
        if out.shape[2] != ys[2]:
            raise ValueError("%s: out has %d columns, the matrix has %d" % (who, out.shape[2], ys[2]))
        if Tmax is not None and int(Tmax) != out.shape[1]:
            raise ValueError("%s: Tmax = %d but out has %d rows per utterance" % (who, Tmax, out.shape[1]))
        if dtype is not None and np.dtype(str(out.dtype).replace("torch.", "")) != odt:
            raise ValueError("%s: out is %s, dtype asks for %s" % (who, out.dtype, odt))
        if out is Y:
            raise ValueError("%s: out must not be the matrix itself (rows move across workgroups)" % who)
        if not out.is_cuda:
            raise ValueError("%s: out must be a CUDA tensor" % who)
    return mf, odt


def remove_silence_frames_batch(Y, durations, silence, lengths=None, num_phones=None, *, min_frames=None, Tmax=None, out=None, dtype=None,
                                strict=True):
    """A padded batch in one launch.  Y ``(B, Tmax_in, D)`` float32 / float64 (a column slice of a wider dense tensor is used where
    it lies), durations ``(B, Nmax, S)`` (int32, int64, float32 or float64), silence ``(B, Nmax)`` bool or integers (non-zero:
    silent), lengths ``(B)`` or None (every utterance has ``Tmax_in`` frames), num_phones ``(B)`` or None.  Returns
    ``(out, lengths_out)``: out ``(B, Tmax, D)`` holds each utterance's kept rows, in order, and zeros behind them; lengths_out
    int32 ``(B)`` their number.  The flags come from the labels, one per phone:
    ``sil = np.zeros(N, bool); sil[labels.silence_phone_indices(regex)] = True``.

    With ``T_b`` the frames the durations give: frame ``t < lengths[b]`` is dropped iff ``t < T_b`` and its phone is flagged.
    Frames at or past ``T_b`` are kept, as ``np.delete`` keeps them; silent frames at or past ``lengths[b]`` do not exist (the
    acoustic matrix is shorter than its labels).  Rows at or past ``lengths[b]`` are never read.  min_frames: as in
    ``frontend.merlin.frame_features_batch``.

    dtype: float32 or float64 (None: Y's own); the kept values are converted, rounded once.  out: a CUDA tensor to write into,
    ``(B, Tmax, D)``; a column slice of a wider dense tensor is fine, and its other columns are not touched; it must not be Y.

    If neither Tmax nor out is given the launch writes ``Tmax_in`` rows per utterance (nothing is lost), the lengths are read back
    and out is cut to the longest: one synchronisation.  If one is given, ``strict=True`` reads the lengths back too and raises
    ``ValueError`` naming the first utterance that does not fit; ``strict=False`` synchronises nothing (for stream capture) and
    truncation shows only in ``lengths_out``, which are then ``Tmax``."""
    who = "remove_silence_frames_batch"
    mf, odt = _validate(Y, durations, silence, lengths, num_phones, min_frames, Tmax, out, dtype, who, 3)
    from .. import _hip
    as_tensor = _is_tensor(Y)
    on_device = as_tensor and Y.is_cuda
    dev = _hip.require_gpu(Y.device if on_device else (out.device if out is not None else None))
    torch = _hip.torch_mod()
    src = _to_device(Y, dev, torch)
    try:
        _hip._pf_row_stride(src, src.shape[0], src.shape[1], src.shape[2], who)
    except _hip.HipExtensionError:
        src = src.contiguous()
    if _is_tensor(durations):
        d = durations if durations.dtype in (torch.int32, torch.int64, torch.float32, torch.float64) else durations.to(torch.int64)
    else:
        d = np.ascontiguousarray(durations)
        d = torch.from_numpy(d if d.dtype in (np.int32, np.int64, np.float32, np.float64) else d.astype(np.int64))
    d = d.to(dev).contiguous()
    sil = (_to_device(silence if _is_tensor(silence) else np.asarray(silence) != 0, dev, torch) != 0).contiguous()
    ln, n = (_to_device(v if v is None or _is_tensor(v) else np.asarray(v), dev, torch, torch.int32) for v in (lengths, num_phones))
    ln, n = (None if v is None else v.contiguous() for v in (ln, n))
    B, Tin, D = src.shape
    T = out.shape[1] if out is not None else Tmax
    tdt = torch.float32 if odt == np.float32 else torch.float64
    if T is None:
        full = torch.empty((B, Tin, D), dtype=tdt, device=dev)       # no output is longer than its source
        lengths_out = SH.gather(src, ln, d, n, sil, mf, full)
        longest = int(lengths_out.max().item()) if B else 0
        out = full if longest == Tin else full[:, :longest].contiguous()
    else:
        if strict:
            # the lengths alone: the same launch over no columns, with room for every source row (nothing is read or stored)
            need = SH.gather(src[:, :, :0], ln, d, n, sil, mf, torch.empty((B, Tin, 0), dtype=tdt, device=dev)).cpu().numpy()
            if (need > int(T)).any():
                b = int(np.argmax(need > int(T)))
                raise ValueError("%s: utterance %d keeps %d frames, Tmax is %d" % (who, b, need[b], int(T)))
        if out is None:
            out = torch.empty((B, int(T), D), dtype=tdt, device=dev)
        lengths_out = SH.gather(src, ln, d, n, sil, mf, out)
    if on_device:
        return out, lengths_out
    if as_tensor:
        return out.cpu(), lengths_out.cpu()
    return out.cpu().numpy(), lengths_out.cpu().numpy()


def remove_silence_frames(y, durations, silence, *, min_frames=None):
    """One utterance: y ``(T, D)``, durations ``(N, S)`` and silence ``(N,)`` in, ``(T', D)`` out -- what
    ``np.delete(y, labels.silence_frame_indices(regex), axis=0)`` returns for labels with these durations and
    ``sil = np.zeros(N, bool); sil[labels.silence_phone_indices(regex)] = True`` (for a y shorter than the labels' frames: with
    the indices at or past T left out).  Takes numpy arrays or tensors and returns the same kind."""
    _validate(y, durations, silence, None, None, min_frames, None, None, None, "remove_silence_frames", 2)
    silence = silence if _is_tensor(silence) else np.asarray(silence)
    out, _ = remove_silence_frames_batch(y[None], durations[None], silence[None], min_frames=min_frames)
    return out[0]
