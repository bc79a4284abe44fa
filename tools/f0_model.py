"""Executable specification of continuous F0 on the device (include/nnmnkwii_f0.h; csrc/f0_interp.hip): the
reference's ``preprocessing.interp1d`` -- fill the unvoiced gaps of an F0 / log-F0 track -- and the V/UV flag, over padded batches.

One utterance, one column x[0 .. L-1].  A frame is *voiced* (x[t] > 0), *fillable* (x[t] <= 0: 0, -0.0, Merlin's -1e10) or
neither (NaN).  If no frame is voiced, or L < 2, y = x.  (For L == 1 with a voiced frame the reference raises from SciPy, which
wants two knots; the batch form has no use for an exception in the middle of a batch and returns the frame.)  Otherwise, with
f / l the first / last voiced frame, frame 0 takes x[f] and frame L-1 takes x[l], whatever they held (a NaN there is
overwritten): call the result x'.  The knots are the frames with x' > 0; every frame with x'[t] <= 0 lies strictly between two
knots p < t < q with values a = x'[p] and b = x'[q] and becomes

    "slinear", "linear"    a + (b - a) * ((t - p) / (q - p))
    "previous", "zero"     a
    "next"                 b
    "nearest"              a if 2 (t - p) <= q - p else b        (SciPy rounds halves down)
    "nearest-up"           a if 2 (t - p) <  q - p else b

The linear form is float64: t - p and q - p are exact, then one division, one subtraction, one multiplication and one addition,
each rounded (the kernel is compiled with -ffp-contract=off).  It gives exactly a when a == b.  Every other frame keeps x'[t].
Values are read in the input dtype, computed in float64 and rounded once to the output dtype.  vuv[t] = 1 where the ORIGINAL
x[t] > 0, else 0.  Padded batches: L_b = clamp(lengths[b], 0, Tmax) (Tmax without lengths); rows at or past L_b of y and vuv are
zeros; the columns of a (B, Tmax, C) batch are independent.

``literal`` is the definition, frame by frame.  ``tiled`` computes the same the way the kernel partitions it -- tiles of TILE
frames, the nearest voiced frame below and above inside the tile, a carry from the left, a look-ahead to the right that is kept
until the walk passes what it found -- and must equal ``literal`` bit for bit at every tile size.  ``truth`` is exact."""
from fractions import Fraction

import numpy as np

KINDS = ("slinear", "linear", "previous", "zero", "next", "nearest", "nearest-up")
SLINEAR, LINEAR, PREVIOUS, ZERO, NEXT, NEAREST, NEAREST_UP = range(7)
TILE = 256               # NNMK_F0_TILE: frames per step of a workgroup's walk


def kind_of(kind):
    """The kind's number (the order of KINDS); ValueError for anything else -- "quadratic", "cubic" and integer orders are
    global spline solves and no part of this."""
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError("interp1d: kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    return KINDS.index(kind)


def _fill(k, a, b, t, p, q):
    """The value of fillable frame t between the knots p < t < q with values a, b (Python floats: IEEE float64)."""
    if k in (SLINEAR, LINEAR):
        w = float(t - p) / float(q - p)
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.float64(a) + (np.float64(b) - np.float64(a)) * np.float64(w))
    if k in (PREVIOUS, ZERO):
        return a
    if k == NEXT:
        return b
    if k == NEAREST:
        return a if 2 * (t - p) <= q - p else b
    return a if 2 * (t - p) < q - p else b


def _out(x, dtype):
    dtype = np.dtype(x.dtype if dtype is None else dtype)
    if dtype not in (np.float32, np.float64):
        raise ValueError("interp1d: float32 or float64 only, got %s" % dtype)
    return dtype


def _edge_hold(x):
    """(x' as float64, the knots' indices) of a column with a voiced frame and L >= 2."""
    xd = x.astype(np.float64)
    voiced = np.flatnonzero(xd > 0)
    xp = xd.copy()
    xp[0] = xd[voiced[0]]
    xp[-1] = xd[voiced[-1]]
    return xp, np.flatnonzero(xp > 0)


def literal(x, kind="slinear", dtype=None):
    """y of one column x (L,), in `dtype` (x's own by default)."""
    x = np.asarray(x)
    assert x.ndim == 1
    k, dtype = kind_of(kind), _out(x, dtype)
    xd = x.astype(np.float64)
    if len(x) < 2 or not (xd > 0).any():
        return xd.astype(dtype)
    xp, knots = _edge_hold(x)
    y = xp.copy()
    for t in np.flatnonzero(xp <= 0):
        i = np.searchsorted(knots, t)
        p, q = int(knots[i - 1]), int(knots[i])
        y[t] = _fill(k, float(xp[p]), float(xp[q]), int(t), p, q)
    return y.astype(dtype)


def vuv(x, dtype=None):
    """The voiced / unvoiced flag of one column: 1 where x > 0, else 0."""
    x = np.asarray(x)
    return (x > 0).astype(_out(x, dtype))


def truth(x, kind="slinear"):
    """[(t, exact value as a Fraction, max(|a|, |b|))] for the filled frames of one column with finite knots."""
    x = np.asarray(x)
    k = kind_of(kind)
    xd = x.astype(np.float64)
    if len(x) < 2 or not (xd > 0).any():
        return []
    xp, knots = _edge_hold(x)
    res = []
    for t in np.flatnonzero(xp <= 0):
        i = np.searchsorted(knots, t)
        p, q = int(knots[i - 1]), int(knots[i])
        a, b = Fraction(float(xp[p])), Fraction(float(xp[q]))
        if k in (SLINEAR, LINEAR):
            v = a + (b - a) * Fraction(int(t) - p, q - p)
        else:
            v = Fraction(_fill(k, float(xp[p]), float(xp[q]), int(t), p, q))
        res.append((int(t), v, max(abs(float(xp[p])), abs(float(xp[q])))))
    return res


def tiled(x, kind="slinear", tile=TILE, dtype=None, stats=None):
    """`literal`, computed as csrc/f0_interp.hip does.  The walk works on the ORIGINAL voiced flags alone: a frame with no voiced
    frame below it has p = 0 and a = b (frame 0 holds the first voiced value), one with none above it has q = L - 1 and b = a
    (frame L-1 holds the last), one with neither belongs to a column without a voiced frame and keeps its value; frames 0 and
    L-1, where not voiced, take a.  stats: a dict that receives the frames read by the walk and by the look-ahead."""
    x = np.asarray(x)
    assert x.ndim == 1 and tile >= 1
    k, dtype = kind_of(kind), _out(x, dtype)
    xd = x.astype(np.float64)
    L = len(x)
    y = np.zeros(L, dtype=np.float64)
    carry = None                 # (index, value) of the last voiced frame of the tiles behind
    ahead, hold = None, False    # (index, value) of the first voiced frame past the tile; hold: there is none up to L-1
    reads_walk = reads_ahead = 0
    for t0 in range(0, L, tile):
        v = xd[t0:t0 + tile]
        n = len(v)
        reads_walk += n
        flag = v > 0
        below = np.maximum.accumulate(np.where(flag, np.arange(n), -1))                 # the max-scan
        above = np.minimum.accumulate(np.where(flag, np.arange(n), tile)[::-1])[::-1]   # the min-scan
        last = int(below[-1])
        if last < n - 1 and not (hold or (ahead is not None and ahead[0] >= t0 + n)):
            ahead = None
            for tm in range(t0 + tile, L, tile):
                u = xd[tm:tm + tile]
                reads_ahead += len(u)
                hit = np.flatnonzero(u > 0)
                if len(hit):
                    ahead = (tm + int(hit[0]), float(u[hit[0]]))
                    break
            hold = ahead is None
        for i in range(n):
            t = t0 + i
            if below[i] >= 0:
                has_p, p, a = True, t0 + int(below[i]), float(v[below[i]])
            elif carry is not None:
                has_p, (p, a) = True, carry
            else:
                has_p, p, a = False, 0, None
            if above[i] < tile:
                has_q, q, b = True, t0 + int(above[i]), float(v[above[i]])
            elif not hold:
                has_q, (q, b) = True, ahead
            else:
                has_q, q, b = False, L - 1, None
            if not has_p:
                a = b
            if not has_q:
                b = a
            if L < 2 or flag[i] or (not has_p and not has_q):
                y[t] = v[i]
            elif t == 0 or t == L - 1:
                y[t] = a
            elif v[i] <= 0:
                y[t] = _fill(k, a, b, t, p, q)
            else:
                y[t] = v[i]
        if last >= 0:
            carry = (t0 + last, float(v[last]))
    if stats is not None:
        stats["walk"], stats["ahead"] = reads_walk, reads_ahead
    return y.astype(dtype)


def clamp_lengths(lengths, B, Tmax):
    if lengths is None:
        return np.full(B, Tmax, dtype=np.int64)
    lengths = np.asarray(lengths)
    assert lengths.shape == (B,)
    return np.clip(lengths.astype(np.int64), 0, Tmax)


def batch(X, lengths=None, kind="slinear", dtype=None, vuv_dtype=None, fn=literal):
    """(y, vuv) of a padded batch X (B, Tmax, C) or (B, Tmax): every column of every utterance on its own over its L_b live
    frames, zeros behind them."""
    X = np.asarray(X)
    assert X.ndim in (2, 3)
    X3 = X if X.ndim == 3 else X[:, :, None]
    B, Tmax, C = X3.shape
    kind_of(kind)
    Y = np.zeros(X3.shape, dtype=_out(X3, dtype))
    V = np.zeros(X3.shape, dtype=_out(X3, vuv_dtype))
    for b, Lb in enumerate(clamp_lengths(lengths, B, Tmax)):
        for c in range(C):
            Y[b, :Lb, c] = fn(X3[b, :Lb, c], kind, dtype=Y.dtype)
            V[b, :Lb, c] = vuv(X3[b, :Lb, c], V.dtype)
    return (Y, V) if X.ndim == 3 else (Y[:, :, 0], V[:, :, 0])
