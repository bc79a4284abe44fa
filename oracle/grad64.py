"""MLPG gradient w.r.t. the means in float64 (or wider), numpy only -- TEST INFRASTRUCTURE ONLY.

An independent anchor for every backward kernel: it shares no code with ``libmlpg_hip`` or ``liboracle.so`` and
does not call them.  For utterance b of length L and static dim d (the reference's mlpg_grad, _mlpg.py:202-281,
restated per utterance as the batching of util/__init__.py:44-66 applies it):

* tau_w[t] = 1 / var[t, w*sd + d], the reciprocal taken in the input dtype (_mlpg.py:259; oracle/mlpg.py);
  unit variances: tau = 1;
* for w >= 1, tau_w is zeroed where t < mw or t >= L - mw, mw = max_w max(l_w, u_w) (_mlpg.py:177, 192); with
  mw == 0 the whole column is zeroed (the reference's ``[-0:]`` slice: csrc/assemble.h);
* W_w is the window matrix W[t, t+k] = c_w[l_w + k], truncated at 0 and L;
* P = sum_w W_w^T diag(tau_w) W_w,  z = P^-1 g[:L, d],  grad[t, w*sd + d] = tau_w[t] * (W_w z)[t].

Rows at and past L are exactly 0; whatever the padding of ``var`` and ``grad_out`` holds is never read into a live
row.  P is factored as a banded L D L^T with a Python loop over frames, vectorised over all B * sd systems: O(T q^2).
"""
import numpy as np


def _norm_windows(windows):
    out = []
    for l, u, c in windows:
        c = np.asarray(c, dtype=np.float64).ravel()
        assert l >= 0 and u >= 0 and len(c) == l + u + 1
        out.append((int(l), int(u), c))
    return out


def precisions(var, windows, lengths, B, T, sd, dtype=np.float64):
    """tau (nw, T, B*sd) in ``dtype``: reciprocals in the input dtype, edge-masked, exactly 0 at and past each length."""
    windows = _norm_windows(windows)
    nw = len(windows)
    mw = max(max(l, u) for l, u, _ in windows)
    t = np.arange(T)[:, None]
    Ls = np.repeat(np.asarray(lengths, dtype=np.int64), sd)[None, :]          # (1, B*sd): system n = b*sd + d
    live = t < Ls
    tau = np.zeros((nw, T, B * sd), dtype=dtype)
    for w in range(nw):
        if var is None:
            r = np.ones((T, B * sd), dtype=dtype)
        else:
            var = np.asarray(var)
            one = var.dtype.type(1)
            if var.ndim == 1:
                col = (one / var[w * sd:(w + 1) * sd]).astype(dtype)
                r = np.broadcast_to(np.tile(col, B)[None, :], (T, B * sd))
            else:
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    r = (one / var[:, :, w * sd:(w + 1) * sd]).astype(dtype)     # (B, T, sd): padding may be junk
                r = r.transpose(1, 0, 2).reshape(T, B * sd)
        keep = live
        if w >= 1:
            keep = keep & (t >= mw) & (t < Ls - mw) if mw > 0 else np.zeros_like(live)
        tau[w] = np.where(keep, r, 0)
    return tau


def _band(tau, windows, Ls, T, q, dtype):
    """Upper band of P: Pb[m, i, n] = P_n[i, i + m], m = 0..q; rows at and past L_n are the identity's."""
    N = tau.shape[2]
    Pb = np.zeros((q + 1, T, N), dtype=dtype)
    t = np.arange(T)[:, None]
    for w, (l, u, c) in enumerate(windows):
        for k1 in range(-l, u + 1):
            for k2 in range(k1, u + 1):
                cc = c[l + k1] * c[l + k2]
                if cc == 0:
                    continue
                # frame t couples unknowns i = t + k1 and j = t + k2, both inside [0, L)
                ok = (t + k1 >= 0) & (t + k2 < Ls)
                contrib = np.where(ok, tau[w] * cc, 0)
                lo, hi = max(0, -k1), T - max(0, k2)
                if hi > lo:
                    Pb[k2 - k1, lo + k1:hi + k1] += contrib[lo:hi]
    dead = np.arange(T)[:, None] >= Ls
    Pb[0] = np.where(dead, 1, Pb[0])
    return Pb


def banded_solve(Pb, rhs):
    """Solve P z = rhs for every system n: Pb (q+1, T, N) upper band of symmetric positive definite P_n, rhs (T, N).

    Banded L D L^T with unit lower L stored as Lb[m, i] = L[i, i - m]."""
    q, T, N = Pb.shape[0] - 1, Pb.shape[1], Pb.shape[2]
    Lb = np.zeros_like(Pb)
    Dg = np.zeros((T, N), dtype=Pb.dtype)
    for i in range(T):
        for m in range(min(q, i), 0, -1):                 # j = i - m, ascending
            j = i - m
            s = Pb[m, j].copy()
            for m2 in range(m + 1, min(q, i) + 1):        # k = i - m2 < j
                s -= Lb[m2, i] * Lb[m2 - m, j] * Dg[i - m2]
            Lb[m, i] = s / Dg[j]
        d = Pb[0, i].copy()
        for m in range(1, min(q, i) + 1):
            d -= Lb[m, i] * Lb[m, i] * Dg[i - m]
        Dg[i] = d
    y = np.array(rhs, dtype=Pb.dtype)
    for i in range(T):
        for m in range(1, min(q, i) + 1):
            y[i] -= Lb[m, i] * y[i - m]
    y /= Dg
    for i in range(T - 1, -1, -1):
        for m in range(1, min(q, T - 1 - i) + 1):
            y[i] -= Lb[m, i + m] * y[i + m]
    return y


def mlpg_grad64(var, grad_out, windows, lengths=None, dtype=np.float64):
    """Gradient of batched MLPG w.r.t. the means.

    var: (B, T, D) per-frame, (D,) global, or None (unit variances); grad_out: (B, T, sd); lengths: (B,) or None
    (every utterance T frames).  Returns (B, T, D) in ``dtype`` (float64, or np.longdouble to judge float64 kernels
    below 1e-12)."""
    windows = _norm_windows(windows)
    grad_out = np.asarray(grad_out)
    B, T, sd = grad_out.shape
    nw = len(windows)
    D = nw * sd
    if var is not None:
        assert np.asarray(var).shape in ((D,), (B, T, D))
    if lengths is None:
        lengths = np.full(B, T, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.shape == (B,) and (lengths >= 0).all() and (lengths <= T).all()
    q = max(l + u for l, u, _ in windows)
    Ls = np.repeat(lengths, sd)[None, :]
    tau = precisions(var, windows, lengths, B, T, sd, dtype)
    live = np.arange(T)[:, None] < Ls
    g = grad_out.transpose(1, 0, 2).reshape(T, B * sd)
    g = np.where(live, g.astype(dtype), 0)
    z = banded_solve(_band(tau, windows, Ls, T, q, dtype), g)
    z = np.where(live, z, 0)
    out = np.zeros((T, nw, B * sd), dtype=dtype)
    for w, (l, u, c) in enumerate(windows):
        wz = np.zeros((T, B * sd), dtype=dtype)
        for k in range(-l, u + 1):
            if c[l + k] == 0:
                continue
            lo, hi = max(0, -k), T - max(0, k)
            if hi > lo:
                wz[lo:hi] += c[l + k] * z[lo + k:hi + k]      # z is 0 at and past L: the truncation at L
        out[:, w] = tau[w] * wz
    # (T, nw, B, sd) -> (B, T, nw*sd)
    return np.ascontiguousarray(out.reshape(T, nw, B, sd).transpose(2, 0, 1, 3).reshape(B, T, D))
