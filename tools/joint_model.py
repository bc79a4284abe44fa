"""Executable specification of the joint-rows kernels (csrc/joint_rows.hip, include/nnmnkwii_joint.h) in numpy.

The recipe it serves, in the reference's words (padded (B, T, D) pairs from DTWAligner):

    Xa = apply_each2d_trim(delta_features, Xa, windows); Ya = ...      # per utterance, zeros past its frames
    XY = np.concatenate((Xa, Ya), axis=-1).reshape(-1, 2 * D')           # joint rows
    XY = remove_zeros_frames(XY)                                         # padding and silent frames out

``literal``  utterance by utterance, frame by frame: the row, its sum s, the keep rule, the kept rows one after another.
``tiled``    the kernels' form: tiles of TILE frames, one keep mask per tile, the exclusive scan of the masks' popcounts, a
             row's number as its tile's offset plus the popcount below its bit, `cap`.  Equal to ``literal`` bit for bit.

A row (width W = (Dx + Dy) * nw): ``row[w * Dx + d] = sum_k coef_w[l_w + k] * x[t + k, d]`` in float64 from 0.0 with k ascending,
each tap one rounded multiplication and one rounded addition, taps outside [0, len_x) skipped, the block 0 for t >= len_x,
rounded once to the output's dtype; without windows the value itself, converted.  The y block follows.  s: lane i of 64 sums
|row[j]| for j = i, i + 64, ... ascending from 0.0; then for m = 32, 16, .. 1 every lane adds the sum of lane i ^ m."""
import numpy as np

TILE = 64                       # NNMK_JOINT_TILE
NONZERO, LIVE = 0, 1
MAX_WINDOWS, MAX_EXTENT = 8, 8


def same_window(window):
    """np.correlate(x, window, "same") as (l, u, coef): out[t] = sum_k coef[l + k] x[t + k]."""
    w = np.asarray(window, dtype=np.float64).ravel()
    u = (len(w) - 1) // 2
    return (len(w) - 1 - u, u, w)


def clamp(lengths, B, Tmax):
    if lengths is None:
        return np.full(B, Tmax, dtype=np.int64)
    return np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)


def workspace_bytes(B, Tmax):
    return -1 if B < 0 or Tmax < 0 else 16 * B * (-(-Tmax // TILE))


def block(x, L, wins, dtype_out):
    """The block of one source of one utterance: x (Tmax, D), L live frames -> (Tmax, D * nw) of dtype_out."""
    Tmax, D = x.shape
    x = x.astype(np.float64)
    if not wins:
        out = np.zeros((Tmax, D))
        out[:L] = x[:L]
        return out.astype(dtype_out)
    out = np.zeros((Tmax, D * len(wins)))
    for w, (l, u, c) in enumerate(wins):
        acc = np.zeros((Tmax, D))
        for k in range(-l, u + 1):
            lo, hi = max(0, -k), min(L, L - k)          # frames t < L with 0 <= t + k < L
            if hi > lo:
                acc[lo:hi] = acc[lo:hi] + np.float64(c[l + k]) * x[lo + k:hi + k]
        out[:, w * D:(w + 1) * D] = acc
    return out.astype(dtype_out)


def abs_sums(rows):
    """s of every row of (T, W), in the kernel's order."""
    T, W = rows.shape
    n = -(-max(W, 1) // 64)
    a = np.zeros((T, n * 64))
    a[:, :W] = np.abs(rows.astype(np.float64))
    a = a.reshape(T, n, 64)
    v = np.zeros((T, 64))
    with np.errstate(all="ignore"):
        for i in range(n):
            v = v + a[:, i]
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lanes ^ m]
    return v[:, 0]


def utterance(x, y, lx, ly, wins, keep, eps, dtype_out):
    """(all Tmax rows, the keep flags) of one utterance; y may be None."""
    blocks = [block(x, lx, wins, dtype_out)]
    if y is not None:
        blocks.append(block(y, ly, wins, dtype_out))
    rows = np.concatenate(blocks, axis=1)
    L = max(lx, ly if y is not None else 0)
    flags = np.arange(len(rows)) < L
    if keep == NONZERO:
        with np.errstate(invalid="ignore"):
            flags &= abs_sums(rows) > eps                  # (a NaN sum: False)
    return rows, flags


def _sources(X, Y, len_x, len_y):
    X = np.asarray(X)
    B, Tmax, Dx = X.shape
    Y = None if Y is None or np.asarray(Y).shape[2] == 0 else np.asarray(Y)
    lx = clamp(len_x, B, Tmax) if Dx else np.zeros(B, dtype=np.int64)
    ly = clamp(len_y, B, Tmax) if Y is not None else np.zeros(B, dtype=np.int64)
    return X, Y, lx, ly


def literal(X, Y, len_x, len_y, wins, keep=NONZERO, eps=1e-7, dtype_out=np.float64):
    """(rows (N, W), offsets (B + 1) int64)."""
    X, Y, lx, ly = _sources(X, Y, len_x, len_y)
    B, Tmax, Dx = X.shape
    W = (Dx + (Y.shape[2] if Y is not None else 0)) * max(len(wins), 1)
    kept, offsets = [np.zeros((0, W), dtype=dtype_out)], [0]
    for b in range(B):
        rows, flags = utterance(X[b], None if Y is None else Y[b], int(lx[b]), int(ly[b]), wins, keep, eps, dtype_out)
        if W == 0:
            flags[:] = False                                # (B * Tmax * W == 0: nothing is launched)
        kept.append(rows[flags])
        offsets.append(offsets[-1] + int(flags.sum()))
    return np.concatenate(kept, axis=0), np.array(offsets, dtype=np.int64)


def tiled(X, Y, len_x, len_y, wins, keep=NONZERO, eps=1e-7, dtype_out=np.float64, cap=None, out=None):
    """The three stages.  Returns (out, offsets, masks, tile offsets): `out` is (cap, W) (given, or zeros) with the first
    min(N, cap) rows written."""
    X, Y, lx, ly = _sources(X, Y, len_x, len_y)
    B, Tmax, Dx = X.shape
    W = (Dx + (Y.shape[2] if Y is not None else 0)) * max(len(wins), 1)
    tpu = -(-Tmax // TILE)
    masks = np.zeros(B * tpu, dtype=np.uint64)
    rows_of = []
    # stage 1: one mask per tile
    for b in range(B):
        rows, flags = utterance(X[b], None if Y is None else Y[b], int(lx[b]), int(ly[b]), wins, keep, eps, dtype_out)
        rows_of.append(rows)
        if W == 0:
            continue
        for i in range(tpu):
            bits = 0
            for f, kept in enumerate(flags[i * TILE:(i + 1) * TILE]):
                bits |= int(kept) << f
            masks[b * tpu + i] = bits
    # stage 2: exclusive scan of the popcounts
    counts = np.array([bin(int(m)).count("1") for m in masks], dtype=np.int64)
    toff = np.concatenate(([0], np.cumsum(counts)))[:-1].astype(np.int64) if len(counts) else np.zeros(0, dtype=np.int64)
    N = int(counts.sum())
    offsets = np.array([toff[b * tpu] if tpu else 0 for b in range(B)] + [N], dtype=np.int64)
    # stage 3: rank = tile offset + popcount of the mask below the frame's bit
    cap = N if cap is None else cap
    if out is None:
        out = np.zeros((cap, W), dtype=dtype_out)
    for b in range(B):
        for i in range(tpu):
            m = int(masks[b * tpu + i])
            for f in range(TILE):
                if (m >> f) & 1:
                    r = int(toff[b * tpu + i]) + bin(m & ((1 << f) - 1)).count("1")
                    if r < cap:
                        out[r, :W] = rows_of[b][i * TILE + f]
    return out, offsets, masks, toff


def remove_zeros_frames(x, eps=1e-7):
    """The reference's function on one (T, D) matrix, through `literal`."""
    x = np.asarray(x)
    dt = x.dtype if x.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    rows, _ = literal(x.astype(dt)[None], None, None, None, [], NONZERO, eps, dt)
    return rows.astype(x.dtype, copy=False)
