"""Executable specification of silence-frame removal (include/nnmnkwii_silence.h; csrc/frame_keep.hip): the
reference's

    idx = labels.silence_frame_indices(regex)
    X = np.delete(X, idx, axis=0); Y = np.delete(Y, idx, axis=0)

for the frame-level linguistic matrix X and any other frame-level matrix Y of an utterance.  The regular expression is text
processing and gives one flag per phone (``sil = np.zeros(N, bool); sil[labels.silence_phone_indices(regex)] = True``); a frame
is silent iff its phone is flagged, so the keep mask is constant over each phone.

The plain forms are defined through tools/frontend_model.py -- its duration rule (``frames``), its sub-phone columns
(``subphone_row``) and its ``frame_features`` -- plus boolean indexing and padding.  The ``tiled`` forms walk as the kernels do:
two running counts behind every state (frames, kept frames, saturated at 2^31 - 1), blocks of BLOCK_ROWS OUTPUT rows, a binary
search on the kept counts for each row, the source frame from the frame count in front of the found state."""
import numpy as np

import frontend_model as FM

BLOCK_ROWS = 64          # NNMK_SIL_BLOCK_ROWS
frames = FM.frames                  # the duration rule and the sub-phone columns are the frontend model's own functions
subphone_row = FM.subphone_row


def _clip_phones(num_phones, B, Nmax):
    return np.full(B, Nmax, dtype=np.int64) if num_phones is None else np.clip(np.asarray(num_phones, dtype=np.int64), 0, Nmax)


def keep_mask(durations, silence, min_frames=None):
    """One utterance: durations (n, S), silence (n,) -> the keep mask over its T frames (bool (T,))."""
    r = frames(durations, min_frames)
    return np.repeat(~(np.asarray(silence).reshape(-1) != 0), r.sum(axis=1))


def frame_counts(durations, silence, num_phones=None, min_frames=None):
    """(B, 2) int64: K_b (the frames whose phone is not flagged) and T_b (all frames)."""
    d, s = np.asarray(durations), np.asarray(silence)
    B, Nmax = d.shape[:2]
    n = _clip_phones(num_phones, B, Nmax)
    out = np.zeros((B, 2), dtype=np.int64)
    for b in range(B):
        r = frames(d[b, :n[b]], min_frames).sum(axis=1)
        out[b] = r[s[b, :n[b]] == 0].sum(), r.sum()
    return out


def kept_frame_features(P, durations, silence, subphone_features="full", min_frames=None, scale_=None, min_=None, dtype=np.float64,
                        cc=None):
    """One utterance: the frontend model's frame_features without the rows of flagged phones -- (K, Dl + F)."""
    out = FM.frame_features(P, durations, subphone_features, min_frames, scale_, min_, dtype, cc)
    return out[keep_mask(durations, silence, min_frames)]


def _pad(each, Tcap, width, dtype):
    counts = np.array([len(e) for e in each], dtype=np.int64)
    if Tcap is None:
        Tcap = int(counts.max()) if len(each) else 0
    out = np.zeros((len(each), Tcap, width), dtype=dtype)
    for b, e in enumerate(each):
        out[b, :min(len(e), Tcap)] = e[:Tcap]
    return out, np.minimum(counts, Tcap).astype(np.int32), counts


def kept_frame_features_batch(P, durations, silence, num_phones=None, subphone_features="full", min_frames=None, scale_=None, min_=None,
                              Tcap=None, dtype=np.float64, cc=None):
    """A padded batch: P (B, Nmax, Dl), durations (B, Nmax, S), silence (B, Nmax).  Returns (out (B, Tcap, Dl + F) with zeros
    behind each utterance's kept rows, lengths = min(K_b, Tcap), counts = K_b).  Tcap None: the largest K_b."""
    P, d, s = np.asarray(P), np.asarray(durations), np.asarray(silence)
    B, Nmax = d.shape[:2]
    n = _clip_phones(num_phones, B, Nmax)
    each = [kept_frame_features(P[b, :n[b]], d[b, :n[b]], s[b, :n[b]], subphone_features, min_frames, scale_, min_, dtype, cc)
            for b in range(B)]
    return _pad(each, Tcap, P.shape[2] + FM.get_frame_feature_size(subphone_features), dtype)


def remove_silence_frames(y, durations, silence, min_frames=None):
    """One utterance: y (T', D) without the rows t < T whose phone is flagged.  Rows at or past the labels' T frames are kept
    (np.delete keeps them); silent frames at or past T' do not exist (np.delete of older numpy ignored such indices, newer
    numpy raises)."""
    y = np.asarray(y)
    keep = np.ones(len(y), dtype=bool)
    m = keep_mask(durations, silence, min_frames)
    k = min(len(y), len(m))
    keep[:k] = m[:k]
    return y[keep]


def remove_silence_frames_batch(Y, durations, silence, lengths=None, num_phones=None, min_frames=None, Tcap=None, dtype=None):
    """A padded batch: Y (B, Tmax, D), lengths (B) or None (clamped to [0, Tmax]).  Returns (out (B, Tcap, D), lengths_out,
    counts).  Tcap None: the largest count."""
    Y, d, s = np.asarray(Y), np.asarray(durations), np.asarray(silence)
    B, Tmax = Y.shape[:2]
    Nmax = d.shape[1]
    n = _clip_phones(num_phones, B, Nmax)
    ln = np.full(B, Tmax, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)
    dtype = Y.dtype if dtype is None else dtype
    each = [remove_silence_frames(Y[b, :ln[b]], d[b, :n[b]], s[b, :n[b]], min_frames).astype(dtype) for b in range(B)]
    return _pad(each, Tcap, Y.shape[2], dtype)


# ---- the kernels' walk --------------------------------------------------------------------------------------------------------------

def _running_counts(r, sil, S):
    """The two running counts behind every state, int32-saturated, and the int64 totals."""
    flat = r.reshape(-1).astype(np.int64)
    kept = np.where(np.repeat(np.asarray(sil) != 0, S), 0, flat)
    ca, ck = np.cumsum(flat), np.cumsum(kept)
    total = (int(ca[-1]), int(ck[-1])) if len(flat) else (0, 0)
    return np.minimum(ca, FM.MAX_FRAMES), np.minimum(ck, FM.MAX_FRAMES), total[0], total[1]


def _first_above(cum, v):
    lo, hi = 0, len(cum) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if cum[mid] > v:
            hi = mid
        else:
            lo = mid + 1
    return lo


def tiled_kept_frame_features_batch(P, durations, silence, num_phones=None, subphone_features="full", min_frames=None, scale_=None,
                                    min_=None, Tcap=None, dtype=np.float64, cc=None):
    """kept_frame_features_batch, block by block and row by row as keep_expand_kernel walks."""
    kind = FM.kind_of(subphone_features)
    P, d, s = np.asarray(P), np.asarray(durations), np.asarray(silence)
    B, Nmax, S = d.shape
    Dl, F = P.shape[2], FM.SIZES[kind]
    n = _clip_phones(num_phones, B, Nmax)
    if kind == FM.COARSE_CODING and cc is None:
        cc = FM.coarse_coding_table()
    counts = frame_counts(d, s, num_phones, min_frames)[:, 0]
    if Tcap is None:
        Tcap = int(counts.max()) if B else 0
    out = np.full((B, Tcap, Dl + F), np.nan)
    lengths = np.zeros(B, dtype=np.int32)
    for b in range(B):
        r = frames(d[b, :n[b]], min_frames)
        ca, ck, _, total_kept = _running_counts(r, s[b, :n[b]], S)
        live = lengths[b] = min(total_kept, Tcap)
        for t0 in range(0, Tcap, BLOCK_ROWS):
            for row in range(t0, min(t0 + BLOCK_ROWS, Tcap)):
                if row >= live:
                    out[b, row] = 0.0
                    continue
                lo = _first_above(ck, row)
                ph, si = divmod(lo, S)
                i = row - (int(ck[lo - 1]) if lo else 0)
                pd, base, fn = int(r[ph].sum()), int(r[ph, :si].sum()), int(r[ph, si])
                v = np.concatenate([P[b, ph].astype(np.float64), subphone_row(kind, cc, S, si + 1, i, fn, base, pd)])
                if scale_ is not None:
                    v = v * np.asarray(scale_, dtype=np.float64) + np.asarray(min_, dtype=np.float64)
                out[b, row] = v
    return out.astype(dtype), lengths, counts


def tiled_remove_silence_frames_batch(Y, durations, silence, lengths=None, num_phones=None, min_frames=None, Tcap=None, dtype=None):
    """remove_silence_frames_batch, block by block and row by row as keep_gather_kernel walks."""
    Y, d, s = np.asarray(Y), np.asarray(durations), np.asarray(silence)
    B, Tmax, D = Y.shape
    Nmax, S = d.shape[1:]
    n = _clip_phones(num_phones, B, Nmax)
    ln = np.full(B, Tmax, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)
    dtype = Y.dtype if dtype is None else dtype
    counts = np.zeros(B, dtype=np.int64)
    walks = []
    for b in range(B):
        r = frames(d[b, :n[b]], min_frames)
        ca, ck, total_all, total_kept = _running_counts(r, s[b, :n[b]], S)
        length = int(ln[b])
        if length >= total_all:
            counts[b] = total_kept + (length - total_all)
        else:
            lo = _first_above(ca, length)
            before = int(ca[lo - 1]) if lo else 0
            counts[b] = (int(ck[lo - 1]) if lo else 0) + (0 if s[b, lo // S] else length - before)
        walks.append((ca, ck, total_all, total_kept, length))
    if Tcap is None:
        Tcap = int(counts.max()) if B else 0
    out = np.zeros((B, Tcap, D), dtype=dtype)
    for b, (ca, ck, total_all, total_kept, length) in enumerate(walks):
        for t0 in range(0, Tcap, BLOCK_ROWS):
            for row in range(t0, min(t0 + BLOCK_ROWS, Tcap)):
                if row < total_kept:
                    lo = _first_above(ck, row)
                    t = (int(ca[lo - 1]) if lo else 0) + (row - (int(ck[lo - 1]) if lo else 0))
                else:
                    t = total_all + (row - total_kept)
                if t < length:
                    out[b, row] = Y[b, t]
    return out, np.minimum(counts, Tcap).astype(np.int32), counts
