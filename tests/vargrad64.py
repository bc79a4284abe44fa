"""MLPG gradients w.r.t. the means AND the variances in float64, numpy only -- TEST INFRASTRUCTURE ONLY.

The anchor of tests/test_var_grad_gpu.py: built from oracle/grad64.py's precisions, _band and banded_solve (imported, not
copied), it loads no compiled library.  For utterance b of length L and static dim d:

* tau_w, W_w and P as in oracle/grad64.py (reciprocals in the input dtype, the edge mask, the [-0:] rule, truncation at L);
* y = P^-1 sum_w W_w^T (tau_w mu_w),  z = P^-1 g;
* grad_mean[t, w*sd+d] = tau_w[t] (W_w z)[t];
* grad_var[t, w*sd+d]  = -grad_mean[t, w*sd+d] tau_w[t] (mu_w[t] - (W_w y)[t])   (dLoss/dtau_w = (W_w z)(mu_w - W_w y)).

Rows at and past L and masked entries are exactly 0; whatever the padding of the inputs or a masked variance entry holds is
never read into a live value.
"""
import numpy as np

from oracle.grad64 import _band, _norm_windows, banded_solve, precisions


def _apply(x, l, u, c, T):
    """(W x)[t] = sum_k c[l + k] x[t + k] for (T, N) x that is 0 at and past each length (the truncation at L)."""
    out = np.zeros_like(x)
    for k in range(-l, u + 1):
        if c[l + k] == 0:
            continue
        lo, hi = max(0, -k), T - max(0, k)
        if hi > lo:
            out[lo:hi] += c[l + k] * x[lo + k:hi + k]
    return out


def _apply_t(v, l, u, c, T):
    """(W^T v)[s] = sum_k c[l + k] v[s - k] for (T, N) v that is 0 at and past each length (mask the result to s < L)."""
    out = np.zeros_like(v)
    for k in range(-l, u + 1):
        if c[l + k] == 0:
            continue
        lo, hi = max(0, -k), T - max(0, k)            # t in [lo, hi): s = t + k
        if hi > lo:
            out[lo + k:hi + k] += c[l + k] * v[lo:hi]
    return out


def mlpg_var_grad64(means, var, grad_out, windows, lengths=None):
    """(y (B, T, sd), grad_mean (B, T, D), grad_var) in float64 for means (B, T, D), var (B, T, D) per-frame or (D,) global
    (the reciprocal taken in var's dtype), grad_out (B, T, sd), lengths (B,) or None.  grad_var is (B, T, D) for per-frame
    variances and the (D,) gradient of the vector (the sum over utterances and live frames) for global ones."""
    windows = _norm_windows(windows)
    means = np.asarray(means)
    grad_out = np.asarray(grad_out)
    var = np.asarray(var)
    B, T, D = means.shape
    nw = len(windows)
    sd = D // nw
    assert nw * sd == D and grad_out.shape == (B, T, sd) and var.shape in ((D,), (B, T, D))
    if lengths is None:
        lengths = np.full(B, T, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.shape == (B,) and (lengths >= 0).all() and (lengths <= T).all()
    N = B * sd
    q = max(l + u for l, u, _ in windows)
    Ls = np.repeat(lengths, sd)[None, :]
    live = np.arange(T)[:, None] < Ls
    tau = precisions(var, windows, lengths, B, T, sd)                       # (nw, T, N), 0 where masked or dead

    def cols(a, w):                                                          # (B, T, D) column block w -> (T, N), live only
        blk = np.asarray(a[:, :, w * sd:(w + 1) * sd], dtype=np.float64).transpose(1, 0, 2).reshape(T, N)
        return np.where(live, blk, 0.0)

    mu = [cols(means, w) for w in range(nw)]
    rhs = np.zeros((T, N))
    for w, (l, u, c) in enumerate(windows):
        rhs += _apply_t(np.where(tau[w] != 0, tau[w] * mu[w], 0.0), l, u, c, T)
    g = np.where(live, np.asarray(grad_out, dtype=np.float64).transpose(1, 0, 2).reshape(T, N), 0.0)
    Pb = _band(tau, windows, Ls, T, q, np.float64)
    yz = banded_solve(np.concatenate([Pb, Pb], axis=2), np.concatenate([rhs, g], axis=1))     # one factorisation pass, both solves
    y = np.where(live, yz[:, :N], 0.0)
    z = np.where(live, yz[:, N:], 0.0)
    gm = np.zeros((T, nw, N))
    gv = np.zeros((T, nw, N))
    for w, (l, u, c) in enumerate(windows):
        on = tau[w] != 0
        gm[:, w] = np.where(on, tau[w] * _apply(z, l, u, c, T), 0.0)
        gv[:, w] = np.where(on, -gm[:, w] * tau[w] * (mu[w] - _apply(y, l, u, c, T)), 0.0)

    def to_btd(a):
        return np.ascontiguousarray(a.reshape(T, nw, B, sd).transpose(2, 0, 1, 3).reshape(B, T, D))

    y_out = np.ascontiguousarray(y.reshape(T, B, sd).transpose(1, 0, 2))
    grad_var = to_btd(gv)
    if var.ndim == 1:
        grad_var = grad_var.sum(axis=(0, 1))
    return y_out, to_btd(gm), grad_var
