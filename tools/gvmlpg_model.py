"""Executable specification of MLPG with the likelihood of the trajectory's gv (mlpg_hip_gv_ascent, mlpg_hip_gv; DESIGN.md K11;
Toda, Black, Tokuda 2007, section IV).  numpy only.

For one system (utterance b, static dim d) with T live frames, y in R^T:
    m(y) = (1/T) sum_t y_t,  v(y) = (1/T) sum_t (y_t - m)^2  (the gv),  omega = omega_scale / (2 T)
    L(y) = omega (-1/2 y^T P y + y^T r) - 1/2 p_v (v(y) - mu_v)^2
    g(y) = omega (r - P y) - (2/T) p_v (v(y) - mu_v) (y - m)
    y <- y + alpha g(y), n_iter times
with P = sum_w W_w^T diag(tau_w) W_w and r = sum_w W_w^T diag(tau_w) mu_w as the MLPG forward assembles them.

Three forms:
  * literal: dense W_w, numpy sums (`system_literal`, `ascend_literal`); any float dtype, long double included;
  * banded: the band columns of P as csrc/assemble.h builds them, the chunk-per-lane layout of csrc/mlpg_gv.hip and its
    summation order for m and v -- sequential inside a lane's chunk, then one xor butterfly over the 64 lanes
    (`system_banded`, `ascend_banded`);
  * the padded-batch rules (`gv_ascent_padded`, `gv_padded`).
"""
import numpy as np

LANES = 64
SLACK = 2.0 ** -40          # status 2: L(final) < L(start) - SLACK * max(|L(start)|, |L(final)|)
VAR_FRAME, VAR_GLOBAL, VAR_UNIT = 0, 1, 2


def live_frames(lengths, B, Tmax):
    if lengths is None:
        return np.full(B, Tmax, dtype=np.int64)
    return np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)


def precisions(var, var_mode, windows, T, sd, d):
    """tau (nw, T) float64 of one system: 1/var evaluated in the dtype of `var` (float32 stays float32, as the forward), zero on
    the first and last mw frames of every window but the first (mw = the largest window extent; mw == 0 zeroes them whole)."""
    nw = len(windows)
    mw = max(max(l, u) for l, u, _ in windows)
    tau = np.ones((nw, T))
    for w in range(nw):
        if var_mode == VAR_FRAME:
            col = np.asarray(var)[:T, w * sd + d]
            tau[w] = (col.dtype.type(1) / col).astype(np.float64)
        elif var_mode == VAR_GLOBAL:
            g = np.asarray(var)[w * sd + d]
            tau[w] = np.float64(g.dtype.type(1) / g)
        if w != 0:
            if mw == 0:
                tau[w] = 0.0
            else:
                tau[w, :mw] = 0.0
                tau[w, max(T - mw, 0):] = 0.0
    return tau


def window_matrix(l, u, coef, T, dtype=np.float64):
    W = np.zeros((T, T), dtype=dtype)
    for t in range(T):
        for k in range(-l, u + 1):
            if 0 <= t + k < T:
                W[t, t + k] = coef[l + k]
    return W


def system_literal(mu, tau, windows, dtype=np.float64):
    """Dense (P, r) of one system from mu, tau (nw, T)."""
    T = mu.shape[1]
    P = np.zeros((T, T), dtype=dtype)
    r = np.zeros(T, dtype=dtype)
    for w, (l, u, coef) in enumerate(windows):
        W = window_matrix(l, u, np.asarray(coef, dtype=np.float64), T, dtype)
        tw = tau[w].astype(dtype)
        P += W.T @ (tw[:, None] * W)
        r += W.T @ (tw * mu[w].astype(dtype))
    return P, r


def system_banded(mu, tau, windows, dtype=np.float64):
    """(pk (3, T), r (T)): pk[k, f] = P[f + k, f], summed in the order of assemble_frame (windows, then frames t ascending)."""
    T = mu.shape[1]
    pk = np.zeros((3, T), dtype=dtype)
    r = np.zeros(T, dtype=dtype)
    f = np.arange(T)
    for w, (l, u, coef) in enumerate(windows):
        assert l <= 1 and u <= 1
        c = np.asarray(coef, dtype=np.float64).astype(dtype)
        tw, mw_ = tau[w].astype(dtype), mu[w].astype(dtype)
        for o in range(u, -l - 1, -1):              # t = f - o ascending
            t = f - o
            ok = (t >= 0) & (t <= T - 1)
            a = np.zeros(T, dtype=dtype)
            a[ok] = c[l + o] * tw[t[ok]]
            add = np.zeros(T, dtype=dtype)
            add[ok] = a[ok] * mw_[t[ok]]
            r = r + add
            for k in range(3):
                idx = l + o + k
                if idx <= l + u:
                    okk = ok & (f + k < T)
                    pk[k, okk] = pk[k, okk] + a[okk] * c[idx]
    return pk, r


def band_to_dense(pk):
    T = pk.shape[1]
    P = np.zeros((T, T), dtype=pk.dtype)
    for k in range(3):
        for f in range(T - k):
            P[f + k, f] = P[f, f + k] = pk[k, f]
    return P


def mean_var(y):
    T = len(y)
    m = y.sum() / T
    return m, ((y - m) ** 2).sum() / T


def objective(P, r, y, mu_v, p_v, omega_scale=1.0):
    T = len(y)
    omega = y.dtype.type(omega_scale) / (2 * T)
    _, v = mean_var(y)
    return omega * (-(y @ (P @ y)) / 2 + y @ r) - p_v * (v - mu_v) ** 2 / 2


def gradient(P, r, y, mu_v, p_v, omega_scale=1.0):
    T = len(y)
    omega = y.dtype.type(omega_scale) / (2 * T)
    m, v = mean_var(y)
    return omega * (r - P @ y) - y.dtype.type(2) / T * p_v * (v - mu_v) * (y - m)


def derived_step(G, T, omega, p_v, v, mu_v):
    return 1 / (omega * G + type(omega)(2) / T * p_v * (abs(v - mu_v) + 2 * max(v, mu_v)))


def status_of(L0, L1, v1):
    if not (np.isfinite(L0) and np.isfinite(L1) and np.isfinite(v1)):
        return 1
    return 2 if L1 < L0 - SLACK * max(abs(L0), abs(L1)) else 0


def ascend_literal(P, r, y0, mu_v, p_v, omega_scale=1.0, n_iter=100, step=None, init=1, trace=False):
    """The literal form in the dtype of y0.  Returns (y, report (4), status[, the objective after every iteration])."""
    dt = y0.dtype.type
    T = len(y0)
    P, r, mu_v, p_v = P.astype(dt), r.astype(dt), dt(mu_v), dt(p_v)
    omega = dt(omega_scale) / (2 * T)
    y = y0.copy()
    m, v0 = mean_var(y)
    if init == 1 and v0 > 0 and mu_v > 0:
        y = m + np.sqrt(mu_v / v0) * (y - m)
    m, v = mean_var(y)
    L0 = objective(P, r, y, mu_v, p_v, omega_scale)
    alpha = dt(step) if step is not None and step > 0 else derived_step(np.abs(P).sum(axis=1).max(), T, omega, p_v, v, mu_v)
    Ls = [L0]
    with np.errstate(all="ignore"):
        for _ in range(n_iter):
            y = y + alpha * gradient(P, r, y, mu_v, p_v, omega_scale)
            if trace:
                Ls.append(objective(P, r, y, mu_v, p_v, omega_scale))
        L1 = objective(P, r, y, mu_v, p_v, omega_scale) if n_iter > 0 else L0
        _, v1 = mean_var(y)
    out = (y, np.array([L0, L1, v0, v1], dtype=dt), status_of(L0, L1, v1))
    return out + (np.array(Ls),) if trace else out


# ---- the kernel's form -------------------------------------------------------------------------------------------------------
def chunk_frames(T):
    """M: the frames per lane; lane p owns frames [p M, p M + M)."""
    return max(2, -(-T // LANES))


def _butterfly(s):
    lanes = np.arange(LANES)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ m]
    return s[0]


def _chunk_sum(x, M):
    """x: (64 M) in frame order (zeros past T): sequential inside each lane's chunk, then the butterfly."""
    a = x.reshape(LANES, M)
    s = np.zeros(LANES, dtype=x.dtype)
    for i in range(M):
        s = s + a[:, i]
    return _butterfly(s)


def _band_apply(pd, p1, p2, y):
    """(P y)_t = Pd y_t + P1[t] y_{t+1} + P2[t] y_{t+2} + P1[t-1] y_{t-1} + P2[t-2] y_{t-2}, summed in this order."""
    z = np.zeros(2, dtype=y.dtype)
    yp = np.concatenate([z, y, z])
    q1 = np.concatenate([z[:1], p1[:-1]])
    q2 = np.concatenate([z, p2[:-2]])
    acc = pd * y
    acc = acc + p1 * yp[3:-1]
    acc = acc + p2 * yp[4:]
    acc = acc + q1 * yp[1:-3]
    acc = acc + q2 * yp[:-4]
    return acc, np.abs(pd) + np.abs(p1) + np.abs(p2) + np.abs(q1) + np.abs(q2)


def ascend_banded(pk, r, y0, mu_v, p_v, omega_scale=1.0, n_iter=100, step=None, init=1, trace=False):
    """The banded, chunk-per-lane form of the kernel in the dtype of y0: same operations in the same order."""
    dt = y0.dtype.type
    T = len(y0)
    M = chunk_frames(T)
    n = LANES * M
    pad = lambda a: np.concatenate([a.astype(dt), np.zeros(n - T, dtype=dt)])  # noqa: E731
    pd, p1, p2, rr, y = pad(pk[0]), pad(pk[1]), pad(pk[2]), pad(r), pad(y0)
    live = np.arange(n) < T
    Td, mu_v, p_v = dt(T), dt(mu_v), dt(p_v)
    omega = dt(omega_scale) / (dt(2) * Td)

    def mv(y):
        m = _chunk_sum(y, M) / Td
        e = np.where(live, y - m, dt(0))
        return m, _chunk_sum(e * e, M) / Td

    def obj(y, v):
        py, rows = _band_apply(pd, p1, p2, y)
        q = _chunk_sum(np.where(live, y * (rr - dt(0.5) * py), dt(0)), M)
        dv = v - mu_v
        return omega * q - dt(0.5) * p_v * (dv * dv), rows[live].max()

    with np.errstate(all="ignore"):
        m, v = mv(y)
        v0 = v
        if init == 1 and v0 > 0 and mu_v > 0:
            y = np.where(live, m + np.sqrt(mu_v / v0) * (y - m), dt(0))
            m, v = mv(y)
        L0, G = obj(y, v)
        if step is not None and step > 0:
            alpha = dt(step)
        else:
            alpha = dt(1) / (omega * G + dt(2) / Td * p_v * (abs(v - mu_v) + dt(2) * max(v, mu_v)))
        Ls = [L0]
        for _ in range(n_iter):
            c = dt(2) / Td * p_v * (v - mu_v)
            py, _ = _band_apply(pd, p1, p2, y)
            g = omega * (rr - py) - c * (y - m)
            y = np.where(live, y + alpha * g, dt(0))
            m, v = mv(y)
            if trace:
                Ls.append(obj(y, v)[0])
        L1 = obj(y, v)[0] if n_iter > 0 else L0
    out = (y[:T], np.array([L0, L1, v0, v], dtype=dt), status_of(L0, L1, v))
    return out + (np.array(Ls),) if trace else out


# ---- padded batches ----------------------------------------------------------------------------------------------------------
def var_mode_of(var):
    return VAR_UNIT if var is None else (VAR_GLOBAL if np.asarray(var).ndim == 1 else VAR_FRAME)


def gv_ascent_padded(mean, var, windows, lengths, y_in, gv_mean, gv_prec, omega_scale=1.0, n_iter=100, step=None, init=1,
                     form="banded", work=np.float64):
    """mean (B, Tmax, D), var (B, Tmax, D) | (D,) | None, y_in (B, Tmax, sd) -> (y_out (B, Tmax, sd) in the dtype of y_in,
    report (B, sd, 4) float64, status (B, sd) int32).  Frames at or past live_b are 0; live_b = 0 gives report 0, status 0.  A
    system's result depends on its own live frames only.  work: the arithmetic's dtype (np.longdouble: the reference run; then
    y_out and report are long double)."""
    mean, y_in = np.asarray(mean), np.asarray(y_in)
    B, Tmax, D = mean.shape
    nw = len(windows)
    sd = D // nw
    mode = var_mode_of(var)
    live = live_frames(lengths, B, Tmax)
    out_dt = y_in.dtype if work == np.float64 else work
    y_out = np.zeros((B, Tmax, sd), dtype=out_dt)
    report = np.zeros((B, sd, 4), dtype=work)
    status = np.zeros((B, sd), dtype=np.int32)
    for b in range(B):
        T = int(live[b])
        if T == 0:
            continue
        for d in range(sd):
            mu = np.stack([mean[b, :T, w * sd + d].astype(np.float64) for w in range(nw)])
            tau = precisions(var[b] if mode == VAR_FRAME else var, mode, windows, T, sd, d)
            y0 = y_in[b, :T, d].astype(work)
            if form == "banded":
                pk, r = system_banded(mu, tau, windows, work)
                y, rep, st = ascend_banded(pk, r, y0, gv_mean[d], gv_prec[d], omega_scale, n_iter, step, init)
            else:
                P, r = system_literal(mu, tau, windows, work)
                y, rep, st = ascend_literal(P, r, y0, gv_mean[d], gv_prec[d], omega_scale, n_iter, step, init)
            y_out[b, :T, d] = y.astype(out_dt)
            report[b, d], status[b, d] = rep, st
    return y_out, report, status


def gv_padded(x, lengths=None):
    """(B, Tmax, D) -> float64 (B, D): two passes over the live frames; live_b = 0 gives 0."""
    x = np.asarray(x)
    B, Tmax, D = x.shape
    live = live_frames(lengths, B, Tmax)
    out = np.zeros((B, D))
    for b in range(B):
        if live[b]:
            out[b] = x[b, :live[b]].astype(np.float64).var(axis=0)
    return out
