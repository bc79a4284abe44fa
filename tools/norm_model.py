"""Executable specification of corpus normalisation (csrc/colstats.hip): numpy only.

* ``literal_meanvar`` / ``literal_minmax``: the definition, utterance by utterance (the reference's loop: per-utterance mean and
  variance merged into the running ones by Chan, Golub and LeVeque's update; a second pass for the extrema).
* ``kernel_state``: the kernel's form on a padded batch -- the same partition into workgroups, waves and chunks, the same shift
  K, the same summation and merge order as ``colstats_kernel`` and ``colstats_finish_kernel``.  With -ffp-contract=off and
  correctly rounded division the device computes these very bits.
* ``exact``: the truth, in integers and ``fractions.Fraction``, rounded once; with the error scales
  ``S_mean = eps mean|x|`` and ``S_var = eps (var + |mean| sigma)``.
* ``affine``: the apply kernel.
"""
from fractions import Fraction

import numpy as np

CHUNK_ROWS = 16      # MLPG_HIP_COLSTATS_CHUNK_ROWS
BLOCK_ROWS = 512     # MLPG_HIP_COLSTATS_BLOCK_ROWS
WAVES = 4
FIN_SEG = 64
EPS = 2.0 ** -52


# ---- the states: (5, D) float64, rows count, mean, M2, min, max --------------------------------------------------------------
def empty_state(D):
    s = np.zeros((5, D))
    s[3], s[4] = np.inf, -np.inf
    return s


def state_from(mean_, var_, count, D):
    """The reference's (mean_, var_, last_sample_count) as a state: M2 = var_ * count; the extrema are unknown (empty)."""
    s = empty_state(D)
    s[0] = float(count)
    s[1] = np.broadcast_to(np.asarray(mean_, dtype=np.float64), (D,))
    s[2] = np.broadcast_to(np.asarray(var_, dtype=np.float64), (D,)) * float(count)
    return s


def _nanmin2(a, b):
    return np.where((b < a) | (b != b), b, a)


def _nanmax2(a, b):
    return np.where((b > a) | (b != b), b, a)


def merge(a, b):
    """cs_merge: a merged with b, a first.  Elementwise over the columns; both (5, D)."""
    with np.errstate(all="ignore"):
        na, nb = a[0], b[0]
        n = na + nb
        delta = b[1] - a[1]
        w = nb / np.where(n == 0, 1.0, n)
        mean = a[1] + delta * w
        m2 = (a[2] + b[2]) + (delta * delta) * (na * w)
        out = np.empty_like(a)
        take_a, take_b = nb == 0, (na == 0) & (nb != 0)
        out[0] = np.where(take_a, na, np.where(take_b, nb, n))
        out[1] = np.where(take_a, a[1], np.where(take_b, b[1], mean))
        out[2] = np.where(take_a, a[2], np.where(take_b, b[2], m2))
        out[3] = _nanmin2(a[3], b[3])
        out[4] = _nanmax2(a[4], b[4])
    return out


def live_frames(lengths, B, Tmax):
    if lengths is None:
        return np.full(B, Tmax, dtype=np.int64)
    return np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)


def pad(utts, Tmax=None, dtype=None):
    """Zero-padded (B, Tmax, D) batch and the lengths of a list of (T_i, D) arrays."""
    lengths = np.array([len(u) for u in utts], dtype=np.int32)
    Tmax = int(lengths.max()) if Tmax is None else Tmax
    X = np.zeros((len(utts), Tmax, utts[0].shape[1]), dtype=dtype or utts[0].dtype)
    for b, u in enumerate(utts):
        X[b, :len(u)] = u
    return X, lengths


# ---- the literal definition -------------------------------------------------------------------------------------------------
def literal_meanvar(utts, mean_=0.0, var_=0.0, count=0):
    """(mean, var, count) in float64: every utterance's own mean and variance, merged into the running ones."""
    D = utts[0].shape[1]
    s = state_from(mean_, var_, count, D)
    for u in utts:
        if len(u) == 0:
            continue
        u = np.asarray(u, dtype=np.float64)
        m = u.mean(axis=0)
        b = empty_state(D)
        b[0], b[1], b[2] = len(u), m, ((u - m) ** 2).sum(axis=0)
        s = merge(s, b)
    return s[1], s[2] / max(s[0, 0], 1.0), int(s[0, 0])


def literal_minmax(utts):
    mn, mx = np.inf, -np.inf
    for u in utts:
        if len(u):
            mn, mx = np.minimum(mn, u.min(axis=0)), np.maximum(mx, u.max(axis=0))
    return mn, mx


# ---- the kernel's form ------------------------------------------------------------------------------------------------------
def _chunk(v, K):
    """One lane's chunk: v (n, D) float64 in row order, K (D,)."""
    n, D = v.shape
    c = empty_state(D)
    s = np.zeros(D)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = s + (v[i] - K)
            c[3] = _nanmin2(c[3], v[i])
            c[4] = _nanmax2(c[4], v[i])
        c[0] = float(n)
        c[1] = K + s / float(n)
        for i in range(n):
            e = v[i] - c[1]
            c[2] = c[2] + e * e
    return c


def block_partial(x):
    """colstats_kernel's partial of one workgroup: x (n <= BLOCK_ROWS, D), the live frames it takes, in order."""
    n, D = x.shape
    if n == 0:
        return empty_state(D)
    x = np.asarray(x, dtype=np.float64)
    K = x[0]
    waves = []
    for w in range(WAVES):
        s = empty_state(D)
        for r0 in range(w * CHUNK_ROWS, n, WAVES * CHUNK_ROWS):
            s = merge(s, _chunk(x[r0:min(r0 + CHUNK_ROWS, n)], K))
        waves.append(s)
    s = waves[0]
    for w in range(1, WAVES):
        s = merge(s, waves[w])
    return s


def partials(X, lengths=None):
    """Every workgroup's partial, in workspace order: (B * ceil(Tmax / BLOCK_ROWS), 5, D)."""
    B, Tmax, D = X.shape
    live = live_frames(lengths, B, Tmax)
    nblk = -(-Tmax // BLOCK_ROWS)
    out = []
    for b in range(B):
        for j in range(nblk):
            t0 = j * BLOCK_ROWS
            out.append(block_partial(X[b, t0:max(t0, min(t0 + BLOCK_ROWS, int(live[b])))]))
    return np.array(out).reshape(B * nblk, 5, D)


def finish(parts, D, state=None):
    """colstats_finish_kernel: FIN_SEG segments of consecutive partials (segment 0 starts from the incoming state), then a tree
    over adjacent segments; NaN in the mean or M2 makes both NaN."""
    P = len(parts)
    per = -(-P // FIN_SEG)
    seg = []
    for q in range(FIN_SEG):
        s = empty_state(D) if (q or state is None) else np.array(state, dtype=np.float64)
        for p in range(q * per, min(P, (q + 1) * per)):
            s = merge(s, parts[p])
        seg.append(s)
    h = 1
    while h < FIN_SEG:
        for q in range(0, FIN_SEG, 2 * h):
            seg[q] = merge(seg[q], seg[q + h])
        h *= 2
    s = seg[0]
    bad = np.isnan(s[1]) | np.isnan(s[2])
    s[1, bad] = np.nan
    s[2, bad] = np.nan
    return s


def kernel_state(X, lengths=None, state=None):
    """mlpg_hip_column_stats on a padded (B, Tmax, D) batch: the outgoing (5, D) state."""
    X = np.asarray(X)
    return finish(partials(X, lengths), X.shape[2], state)


def stats_of(state):
    """(count, mean, var, min, max) of a state; var = M2 / count."""
    with np.errstate(all="ignore"):
        return int(state[0, 0]), state[1].copy(), state[2] / state[0], state[3].copy(), state[4].copy()


# ---- the truth --------------------------------------------------------------------------------------------------------------
def exact(X, lengths=None):
    """Exact mean and variance of every column over the live frames, each rounded once to float64, and the error scales:
    dict(mean, var, s_mean, s_var, count).  Finite inputs."""
    X = np.asarray(X)
    B, Tmax, D = X.shape
    live = live_frames(lengths, B, Tmax)
    rows = np.concatenate([X[b, :live[b]] for b in range(B)]).astype(np.float64)
    n = len(rows)
    mean, var, s_mean, s_var = (np.zeros(D) for _ in range(4))
    for d in range(D):
        ratios = [float(v).as_integer_ratio() for v in rows[:, d]]
        den = max(q for _, q in ratios)                      # powers of two: the largest is the common denominator
        ints = [p * (den // q) for p, q in ratios]
        s1, s2 = sum(ints), sum(i * i for i in ints)
        mu = Fraction(s1, n * den)
        v = Fraction(n * s2 - s1 * s1, n * n * den * den)
        mean[d], var[d] = float(mu), float(v)
        s_mean[d] = EPS * float(Fraction(sum(abs(i) for i in ints), n * den))
        s_var[d] = EPS * (float(v) + abs(float(mu)) * float(v) ** 0.5)
    return dict(mean=mean, var=var, s_mean=s_mean, s_var=s_var, count=n)


def ratios(mean, var, truth, skip_zero_scale=False):
    """Worst |mean - truth| / S_mean and |var - truth| / S_var over the columns.  A column whose scale is 0 -- constant, or all
    zero -- must be exact: any miss there counts as infinite (skip_zero_scale: such columns are left out instead; the
    reference does not promise exactness there)."""
    out = []
    for got, ref, s in ((mean, truth["mean"], truth["s_mean"]), (var, truth["var"], truth["s_var"])):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref)
        with np.errstate(all="ignore"):
            r = np.where(s > 0, err / np.where(s > 0, s, 1.0), np.where((err == 0) | skip_zero_scale, 0.0, np.inf))
        out.append(float(r.max()))
    return tuple(out)


# ---- the apply kernel -------------------------------------------------------------------------------------------------------
def affine(X, a, c, mode, lengths=None, out_dtype=np.float64):
    """colaffine_kernel: mode 0 (x - c) / a, mode 1 a x + c in float64, rounded once; exact zeros on the pad rows."""
    X = np.asarray(X)
    B, Tmax, _ = X.shape
    x = X.astype(np.float64)
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        y = (x - c) / a if mode == 0 else a * x + c
    y[np.arange(Tmax)[None, :] >= live_frames(lengths, B, Tmax)[:, None]] = 0.0
    return y.astype(out_dtype)
