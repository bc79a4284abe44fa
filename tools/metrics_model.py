"""Executable specification of the objective metrics on the device (csrc/frame_metrics.hip): numpy only.

A term is a dict with the fields of ``nnmk_metrics_term`` (``term(...)`` builds one); it yields the pair (sum, count) in float64.

* ``literal``: the definition, utterance by utterance, with numpy's own sums (the reference's loop in float64).
* ``kernel_order``: the kernel's form on padded batches -- the same partition into workgroups, waves and lanes and the same order
  of every addition as ``metrics_kernel`` and ``metrics_finish_kernel``.  With -ffp-contract=off and correctly rounded sqrt the
  device computes these very bits (terms with the EXP flag: up to the two exponentials).
* ``truth``: every sum in extended precision (np.longdouble, 64-bit significand, pairwise), rounded once at the end: half an ulp
  of float64 plus about 2^-59 from the true value.  Counts are integers.
* ``chain``: the length of the longest chain of additions a sum of ``kernel_order`` goes through for a shape, and ``bound``: the
  relative error bound that follows.  All summands are non-negative, so a sum's relative error is at most the largest relative
  error of a summand plus one rounding per addition of the chain: (chain + 4) 2^-53, the 4 for the difference, the square (twice
  the difference's error, plus its own), and -- FRAME_L2 -- the square root, of which half an ulp is the truth's own rounding.
  EXP: with |x - y| >= 0.1 the difference exp(x) - exp(y) amplifies the two exponentials' errors (one ulp = 2^-52 each at most) by
  (e^x + e^y) / |e^x - e^y| = coth(0.05) < 21, and the square doubles that: 2 * 21 * 2 more units of 2^-53.
"""
import math

import numpy as np

BLOCK_ROWS = 256     # NNMK_METRICS_BLOCK_ROWS
WAVES = 4
FIN_SEG = 256
MAX_TERMS = 8
FRAME_L2, SQUARED, VOICED_SQUARED, MISMATCH = 0, 1, 2, 3
FLAG_EXP = 1
U = 2.0 ** -53
LOGDB = 10.0 / np.log(10.0) * np.sqrt(2.0)     # metrics/__init__.py:5


def term(kind, x_col, y_col=None, width=1, x_mask_col=0, y_mask_col=None, flags=0, threshold=float("nan")):
    return dict(kind=kind, x_col=x_col, y_col=x_col if y_col is None else y_col, width=width, x_mask_col=x_mask_col,
                y_mask_col=x_mask_col if y_mask_col is None else y_mask_col, flags=flags, threshold=threshold)


def live_frames(lengths, B, Tmax):
    if lengths is None:
        return np.full(B, Tmax, dtype=np.int64)
    return np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)


def _operands(x, y, t, dtype=np.float64):
    """x, y: the live (n, ld) rows of one utterance.  (u, v, voiced): the term's columns in `dtype` and its frame mask."""
    w = t["width"]
    u = x[:, t["x_col"]:t["x_col"] + w].astype(dtype)
    v = y[:, t["y_col"]:t["y_col"] + w].astype(dtype)
    voiced = None
    if t["kind"] == VOICED_SQUARED:
        xm, ym = x[:, t["x_mask_col"]].astype(np.float64), y[:, t["y_mask_col"]].astype(np.float64)
        thr = t["threshold"]
        voiced = (xm + ym >= 2.0) if thr != thr else ((xm > thr) & (ym > thr))
    return u, v, voiced


def _elements(x, y, t, dtype=np.float64):
    """(e, count): the (n, width) non-negative summands of a term in `dtype` (FRAME_L2: under the square root) and its count."""
    u, v, voiced = _operands(x, y, t, dtype)
    n, w = u.shape
    with np.errstate(all="ignore"):
        if t["kind"] == MISMATCH:
            thr = t["threshold"]
            ne = (u != v) if thr != thr else ((u > thr) != (v > thr))
            return ne.astype(dtype), n * w
        if t["kind"] == VOICED_SQUARED:
            if t["flags"] & FLAG_EXP:
                u, v = np.exp(u), np.exp(v)
            z = u - v
            return np.where(voiced[:, None], z * z, dtype(0.0)), int(voiced.sum())
        z = u - v
        return z * z, (n if t["kind"] == FRAME_L2 else n * w)


# ---- the literal definition ---------------------------------------------------------------------------------------------------
def literal(X, Y, lengths, terms, dtype=np.float64):
    """per_utt (B, nterms, 2) in `dtype` arithmetic with numpy's sums: the reference's loop body."""
    B, Tmax = X.shape[:2]
    live = live_frames(lengths, B, Tmax)
    out = np.zeros((B, len(terms), 2))
    for b in range(B):
        for i, t in enumerate(terms):
            e, c = _elements(X[b, :live[b]], Y[b, :live[b]], t, dtype)
            out[b, i] = (float(np.sqrt(e.sum(-1)).sum()) if t["kind"] == FRAME_L2 else float(e.sum())), c
    return out


def truth(X, Y, lengths, terms):
    """(per_utt, totals) from extended-precision sums, rounded once."""
    B, Tmax = X.shape[:2]
    live = live_frames(lengths, B, Tmax)
    per = np.zeros((B, len(terms), 2), dtype=np.longdouble)
    for b in range(B):
        for i, t in enumerate(terms):
            e, c = _elements(X[b, :live[b]], Y[b, :live[b]], t, np.longdouble)
            per[b, i] = (np.sqrt(e.sum(-1)).sum() if t["kind"] == FRAME_L2 else e.sum()), c
    return per.astype(np.float64), per.sum(0).astype(np.float64)


# ---- the kernel's form --------------------------------------------------------------------------------------------------------
_LANES = np.arange(64)


def _butterfly(s):
    """mt_wave_sum over the last axis (64 lanes): xor 32, 16, ..., 1; the same bits in every lane."""
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _LANES ^ m]
    return s


def _lanes(e):
    """(n, width) -> (n, K, 64): element d of a frame on lane d % 64 in step d // 64, zeros behind the width."""
    n, w = e.shape
    K = -(-w // 64)
    out = np.zeros((n, K * 64))
    out[:, :w] = e
    return out.reshape(n, K, 64)


def _seq(a):
    """The sum over axis 0 in order, one addition at a time (0 + a[0] is exact)."""
    return np.cumsum(a, axis=0)[-1] if len(a) else np.zeros(a.shape[1:])


def block_partial(x, y, terms):
    """metrics_kernel's (nterms, 2) partial of one workgroup: x, y (n <= BLOCK_ROWS, ld), the live frames it takes."""
    out = np.zeros((len(terms), 2))
    if len(x) == 0:
        return out
    with np.errstate(all="ignore"):
        for i, t in enumerate(terms):
            e, _ = _elements(x, y, t)
            u, v, voiced = _operands(x, y, t)
            L = _lanes(e)                                                    # (n, K, 64)
            s = np.zeros(WAVES)
            c = np.zeros(WAVES)
            for w in range(WAVES):
                Lw = L[w::WAVES]
                lane = np.zeros(64)
                if t["kind"] == FRAME_L2:
                    row = _butterfly(_seq(Lw.transpose(1, 0, 2)))            # (rows of the wave, 64): the lanes' sums over their steps
                    lane[0] = _seq(np.sqrt(row[:, 0]))
                else:
                    lane = _seq(Lw.reshape(-1, 64))                          # a lane's frames in order, within a frame its steps
                s[w] = _butterfly(lane)[0]
                if t["kind"] == VOICED_SQUARED:
                    c[w] = float(voiced[w::WAVES].sum())
            out[i, 0] = _seq(s)
            out[i, 1] = {FRAME_L2: len(x), SQUARED: len(x) * t["width"], MISMATCH: len(x) * t["width"]}.get(t["kind"], _seq(c))
    return out


def partials(X, Y, lengths, terms):
    """Every workgroup's partial in workspace order: (B * ceil(Tmax / BLOCK_ROWS), nterms, 2)."""
    B, Tmax = X.shape[:2]
    live = live_frames(lengths, B, Tmax)
    nblk = -(-Tmax // BLOCK_ROWS)
    out = np.zeros((B * nblk, len(terms), 2))
    for b in range(B):
        for j in range(nblk):
            t0 = j * BLOCK_ROWS
            t1 = max(t0, min(t0 + BLOCK_ROWS, int(live[b])))
            out[b * nblk + j] = block_partial(X[b, t0:t1], Y[b, t0:t1], terms)
    return out


def finish(parts, B, nterms):
    """metrics_finish_kernel: an utterance's blocks in order -> per_utt; FIN_SEG segments of consecutive utterances in order, then
    a tree over adjacent segments -> totals."""
    parts = parts.reshape(B, len(parts) // B if B else 0, nterms, 2)
    per_utt = np.zeros((B, nterms, 2))
    for j in range(parts.shape[1]):
        per_utt = per_utt + parts[:, j]
    per = -(-B // FIN_SEG)
    seg = np.zeros((FIN_SEG, nterms, 2))
    for q in range(FIN_SEG):
        for b in range(q * per, min(B, (q + 1) * per)):
            seg[q] = seg[q] + per_utt[b]
    h = 1
    while h < FIN_SEG:
        seg[::2 * h] = seg[::2 * h] + seg[h::2 * h]
        h *= 2
    return per_utt, seg[0].copy()


def kernel_order(X, Y, lengths, terms):
    """nnmk_metrics_batch on padded (B, Tmax, .) batches: (per_utt (B, nterms, 2), totals (nterms, 2))."""
    return finish(partials(X, Y, lengths, terms), X.shape[0], len(terms))


# ---- the bound ----------------------------------------------------------------------------------------------------------------
def chain(B, Tmax, t):
    """The longest chain of additions behind a total of kernel_order for a (B, Tmax) batch and the term t."""
    K = -(-t["width"] // 64)
    rows = -(-min(BLOCK_ROWS, Tmax) // WAVES)                    # frames of a wave
    nblk = -(-Tmax // BLOCK_ROWS)
    inner = K + 6 if t["kind"] == FRAME_L2 else 0               # under the square root: a lane's steps and the butterfly
    block = (rows if t["kind"] == FRAME_L2 else rows * K) + 6 + (WAVES - 1)
    return inner + block + nblk + -(-B // FIN_SEG) + 8


def bound(B, Tmax, t):
    """Relative error bound of a term's sum against the truth (see the module's docstring)."""
    extra = 2 * 21 * 2 if t["flags"] & FLAG_EXP else 0
    return (chain(B, Tmax, t) + 4 + extra) * U


# ---- the four metrics from the pairs ------------------------------------------------------------------------------------------
def value(name, pair):
    """The reference's figure from (sum, count): melcd, mse (the reference's root of the mean), lf0_mse, vuv_error."""
    s, c = float(pair[0]), float(pair[1])
    if c == 0:
        return float("nan")
    return LOGDB * s / c if name == "melcd" else (s / c if name == "vuv_error" else math.sqrt(s / c))
