"""Executable specification of batched trajectory GMM conversion (csrc/gmm_traj.hip,
``baseline.gmm.MLPG.transform_padded`` / ``transform_batch``).  numpy only.

Toda's trajectory conversion (the reference's baseline/gmm.py:225-247), per utterance ``x`` (T, D) of static+delta features with
the hard mixture label ``m_t`` of every frame (eq. 37):

    E_t = mu_y[m_t] + S_yx[m_t] S_xx[m_t]^-1 (x_t - mu_x[m_t])                          (eq. 22 / 40)
    D_t = diag(S_yy[m_t]) - diag(S_yx[m_t]) / diag(S_xx[m_t]) * diag(S_xy[m_t])         (eq. 23, diagonal approximation)
    y   = mlpg(E, D, windows)

``stats_literal`` is that text, one ``np.linalg.solve`` per frame.  ``tables`` and ``stats_table`` are the form the kernel uses:
``A[m] = S_yx[m] S_xx[m]^-1`` and ``cvar[m]`` are formed once per model, and a frame costs one matrix-vector product.
``stats_padded`` adds the rules of ``mlpg_hip_gmm_trajectory_stats`` for a padded batch: row (b, t) is live when
``t < min(max(lengths[b], 0), Tmax)``; a live row with a label in [0, M) gets the two rows above, a live row with any other label
gets NaN rows, a pad row gets mean 0 and variance 1 and neither its x nor its label is looked at.  ``error_scale`` is the
per-element scale S of the kernel's rounding-error bound.  ``mlpg_dense`` is MLPG as the dense normal equations (no library
code), and ``transform_padded`` / ``transform_batch`` put the pieces together the way the ``MLPG`` methods do.
"""
import numpy as np

ROW_TILE = 64


def live_frames(lengths, B, T):
    L = np.full(B, T, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    assert L.shape == (B,)
    return np.clip(L, 0, T)


def _diag(a):
    return np.diagonal(a, axis1=1, axis2=2)


def stats_literal(x, labels, src_means, tgt_means, covarXX, covarXY, covarYX, covarYY):
    """(E, D) of gmm.py:228-244, frame by frame."""
    x = np.asarray(x, dtype=np.float64)
    T, F = x.shape
    E, Dv = np.empty((T, F)), np.empty((T, F))
    for t in range(T):
        m = labels[t]
        xx = np.linalg.solve(covarXX[m], x[t] - src_means[m])
        E[t] = tgt_means[m] + np.dot(covarYX[m], xx)
        Dv[t] = np.diag(covarYY[m]) - np.diag(covarYX[m]) / np.diag(covarXX[m]) * np.diag(covarXY[m])
    return E, Dv


def tables(covarXX, covarXY, covarYX, covarYY):
    """(A (M, D, D), cvar (M, D)): the per-model tables."""
    A = np.ascontiguousarray(np.linalg.solve(covarXX, covarYX.transpose(0, 2, 1)).transpose(0, 2, 1))   # S_xx symmetric
    cvar = _diag(covarYY) - _diag(covarYX) / _diag(covarXX) * _diag(covarXY)
    return A, np.ascontiguousarray(cvar)


def stats_table(x, labels, mu_x, mu_y, A, cvar):
    """(mean, var) of live rows with valid labels: x (N, D), labels (N)."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    mean = mu_y[labels] + np.einsum("ndk,nk->nd", A[labels], x - mu_x[labels])
    return mean, cvar[labels].copy()


def stats_padded(x, lengths, labels, mu_x, mu_y, A, cvar):
    """The entry point's semantics: x (B, Tmax, D), labels (B, Tmax) or (B * Tmax) -> (mean, var) (B, Tmax, D)."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    M = mu_x.shape[0]
    labels = np.asarray(labels).reshape(B, T)
    live = np.arange(T)[None, :] < live_frames(lengths, B, T)[:, None]
    mean, var = np.zeros((B, T, D)), np.ones((B, T, D))
    ok = live & (labels >= 0) & (labels < M)
    if ok.any():
        mean[ok], var[ok] = stats_table(x[ok], labels[ok], mu_x, mu_y, A, cvar)
    bad = live & ~ok
    mean[bad] = np.nan
    var[bad] = np.nan
    return mean, var


def error_scale(x, labels, mu_x, mu_y, A):
    """S[n, d] = |mu_y[m, d]| + sum_k |A[m, d, k]| |x[n, k] - mu_x[m, k]| for rows x (N, D) with valid labels: a (D + 1)-term sum in
    any order, one rounding per product and per difference, is within (D + 4) eps S of the exact value."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    return np.abs(mu_y[labels]) + np.einsum("ndk,nk->nd", np.abs(A[labels]), np.abs(x - mu_x[labels]))


def mlpg_dense(mean, var, windows):
    """MLPG of one utterance by the dense normal equations: (T, D), (T, D) -> (T, D // len(windows)).  With W_w the (T, T) matrix
    of window w (row t holds its coefficients at columns t - l .. t + u, clipped at the ends) and P_w = diag(1 / var of window
    w), every static dim solves (sum_w W_w^T P_w W_w) y = sum_w W_w^T P_w mean_w.  As in the reference (paramgen/_mlpg.py:190-193) the
    precisions of every window but the first are zero on the first and last max_w max(l_w, u_w) frames."""
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    T, D = mean.shape
    nw = len(windows)
    sd = D // nw
    if T == 0:
        return np.zeros((0, sd))
    Ws = []
    edge = max(max(l, u) for l, u, _ in windows)
    for l, u, c in windows:
        W = np.zeros((T, T))
        for t in range(T):
            for j in range(-l, u + 1):
                if 0 <= t + j < T:
                    W[t, t + j] = c[j + l]
        Ws.append(W)
    y = np.empty((T, sd))
    for d in range(sd):
        R, r = np.zeros((T, T)), np.zeros(T)
        for w, W in enumerate(Ws):
            p = 1.0 / var[:, w * sd + d]
            if w != 0 and edge > 0:
                p[:edge] = 0.0
                p[-edge:] = 0.0
            R += W.T @ (p[:, None] * W)
            r += W.T @ (p * mean[:, w * sd + d])
        y[:, d] = np.linalg.solve(R, r)
    return y


def transform_padded(X, lengths, labels, mu_x, mu_y, A, cvar, windows):
    """(B, Tmax, D) -> (B, Tmax, static_dim) float64, zero beyond the lengths."""
    X = np.asarray(X, dtype=np.float64)
    B, T, D = X.shape
    mean, var = stats_padded(X, lengths, labels, mu_x, mu_y, A, cvar)
    out = np.zeros((B, T, D // len(windows)))
    for b, n in enumerate(live_frames(lengths, B, T)):
        out[b, :n] = mlpg_dense(mean[b, :n], var[b, :n], windows)
    return out


def transform_batch(utterances, predict, mu_x, mu_y, A, cvar, windows):
    """A list of (T_i, D) arrays -> a list of (T_i, static_dim) float64 arrays; ``predict`` gives the labels of (N, D) rows.  The
    utterances are packed into a zero-padded batch; the pad rows keep label 0 and are never used."""
    utterances = [np.asarray(u) for u in utterances]
    if not utterances:
        return []
    lens = np.array([len(u) for u in utterances])
    D = utterances[0].shape[1]
    X = np.zeros((len(utterances), int(lens.max()), D))
    labels = np.zeros(X.shape[:2], dtype=np.int64)
    for i, u in enumerate(utterances):
        X[i, :len(u)] = u
        if len(u):
            labels[i, :len(u)] = predict(np.asarray(u, dtype=np.float64))
    Y = transform_padded(X, lens, labels, mu_x, mu_y, A, cvar, windows)
    return [Y[i, :n].copy() for i, n in enumerate(lens)]
