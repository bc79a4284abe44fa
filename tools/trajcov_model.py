"""Executable specification of K19 (csrc/mlpg_trajcov.hip, include/nnmnkwii_trajectory.h): the band of the trajectory
covariance S = R^-1, log det R, and the trajectory likelihood with its gradients.  numpy only.

One system is (utterance b, static dim d) with T live frames; R = sum_w W_w^T diag(tau_w) W_w with W_w[t, t + k] = c_w[l + k]
and tau_w[t] the reciprocal of the variance IN THE INPUT DTYPE, zero on the first and last mw frames of every window but the
first (mw = the largest extent; mw = 0 zeroes them all), one for unit variances.

* ``dense_definition``: the literal definition -- R from ``paramgen.build_win_mats`` / ``full_window_mat``, ``numpy.linalg.inv``,
  ``slogdet``.
* ``assemble`` / ``factor`` / ``selected_inverse``: the kernel's recurrences in the kernel's order of operations (every product
  and every sum rounded on its own), vectorised over the static dims.  The band of these is what the kernel gives bit for bit;
  ``logdet`` differs by the last place of ``log``.
* ``covariance_batch``, ``nll_batch``: padded batches, the planar band layout, the rules for rows at or past T, the status.
* ``nll_dense``: the likelihood as a dense expression (what the tests differentiate with torch's float64 autograd).
* ``truth``: S and log det R in extended precision: exact rationals (``fractions.Fraction``) for T <= 12, the same banded
  recurrences in ``numpy.longdouble`` above.

Error of the recurrences, MEASURED (tests/test_trajcov_model.py, its cases: T in {1, 2, 3, 4, 5, 8, 17}, four window sets, three
variance modes, and the tight case): the largest |S_model - S_truth| / (2^-53 cond_2(R) max|S|) seen is WORST_RATIO_BAND, the
largest |logdet_model - logdet_truth| / (2^-53 cond_2(R) max(1, |logdet|)) is WORST_RATIO_LOGDET; the bound the tests use is
BOUND_C = 8 x the larger of the two, rounded up to a power of two.  The margin covers other seeds, not other algorithms."""
from fractions import Fraction

import numpy as np

VAR_FRAME, VAR_GLOBAL, VAR_UNIT = 0, 1, 2
LOG_2PI = 1.8378770664093453
EPS = 2.0 ** -53
WORST_RATIO_BAND = 1.17       # measured 1.160: see the docstring and tests/test_trajcov_model.py::test_error_bound_is_the_measured_one
WORST_RATIO_LOGDET = 5.02     # measured 5.018 (a static-only set: cond_2(R) is 4 and the sum of 17 logarithms carries the error)
BOUND_C = 64.0                # 8 x 5.02 = 40.2 -> 64


def var_mode_of(var):
    return VAR_UNIT if var is None else (VAR_GLOBAL if np.ndim(var) == 1 else VAR_FRAME)


def window_set(windows):
    """[(l, u, c float64)], Q = max (l + u), mw = max max(l, u)."""
    ws = [(int(l), int(u), np.asarray(c, dtype=np.float64).ravel()) for l, u, c in windows]
    return ws, max(l + u for l, u, _ in ws), max(max(l, u) for l, u, _ in ws)


def live_frames(lengths, B, Tmax):
    return np.full(B, Tmax, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, Tmax)


def precisions(var, windows, T, sd, edge_rule=True):
    """tau (nw, T, sd) float64 of one utterance: var (>= T, nw sd) per frame, (nw sd) global or None, float32 or float64."""
    ws, _, mw = window_set(windows)
    nw = len(ws)
    tau = np.ones((nw, T, sd))
    if var is not None:
        var = np.asarray(var)
        one = var.dtype.type(1)
        for w in range(nw):
            v = var[w * sd:(w + 1) * sd][None] if var.ndim == 1 else var[:T, w * sd:(w + 1) * sd]
            with np.errstate(divide="ignore"):
                tau[w] = (one / v).astype(np.float64)
    if edge_rule:
        for w in range(1, nw):
            for t in range(T):
                if mw == 0 or t < mw or t >= T - mw:
                    tau[w, t] = 0.0
    return tau


def dense_definition(var, windows, T, sd, edge_rule=True):
    """(R (sd, T, T), S (sd, T, T), logdet (sd)) by the literal definition."""
    from nnmnkwii_amd.paramgen import build_win_mats, full_window_mat
    tau = precisions(var, windows, T, sd, edge_rule)
    nw = len(windows)
    W = full_window_mat(build_win_mats(windows, T), T).reshape(nw, T, T)
    R = np.zeros((sd, T, T))
    for d in range(sd):
        for w in range(nw):
            R[d] += W[w].T @ (tau[w, :, d][:, None] * W[w])
    S = np.stack([np.linalg.inv(R[d]) for d in range(sd)]) if T else np.zeros((sd, 0, 0))
    logdet = np.array([np.linalg.slogdet(R[d])[1] if T else 0.0 for d in range(sd)])
    return R, S, logdet


def assemble(tau, windows, work=np.float64):
    """Columns of R's lower band in the order csrc/assemble.h adds them up: pk (T, Q + 1, sd), pk[f, k] = R[f + k, f]."""
    ws, Q, _ = window_set(windows)
    nw, T, sd = tau.shape
    pk = np.zeros((T, Q + 1, sd), dtype=work)
    tau = tau.astype(work)
    for f in range(T):
        for w, (l, u, c) in enumerate(ws):
            c = c.astype(work)
            for t in range(max(0, f - u), min(T - 1, f + l) + 1):
                a = c[l + f - t] * tau[w, t]
                for k in range(Q + 1):
                    idx = l + f + k - t
                    if idx <= l + u and f + k < T:
                        pk[f, k] = pk[f, k] + a * c[idx]
    return pk


def factor(pk, defect=None):
    """Banded L D L^T in the kernel's order.  Returns (fac (T, Q + 1, sd): 1 / D_t and the multipliers l_{t+k,t}; logdet (sd);
    status (sd): 0 or the 1-based frame of the first non-positive pivot).  defect "drop_j2": the planted defect of the tests."""
    T, Q1, sd = pk.shape
    Q = Q1 - 1
    work = pk.dtype.type
    pend = np.zeros((Q + 1, Q + 1, sd), dtype=pk.dtype)
    fac = np.zeros_like(pk)
    ld = np.zeros(sd, dtype=pk.dtype)
    status = np.zeros(sd, dtype=np.int32)
    with np.errstate(all="ignore"):
        for f in range(T):
            col = pk[f] + pend[0]
            newly = (status == 0) & (col[0] <= 0)
            status[newly] = f + 1
            iv = work(1) / col[0]
            ld = ld + np.log(col[0])
            m = col * iv
            m[0] = iv
            for j in range(Q):
                for k in range(Q + 1):
                    nv = pend[j + 1, k].copy()
                    if k + j + 1 <= Q and not (defect == "drop_j2" and j + 1 == 2):
                        nv = nv - m[j + 1] * col[k + j + 1]
                    pend[j, k] = nv
            fac[f] = m
    return fac, ld, status


def selected_inverse(fac, defect=None):
    """Takahashi's recurrence in the kernel's order: band (Q + 1, T, sd), band[k, t] = S[t, t + k], 0 where t + k >= T."""
    T, Q1, sd = fac.shape
    Q = Q1 - 1
    band = np.zeros((Q + 1, T, sd), dtype=fac.dtype)
    Z = np.zeros((max(Q, 1), max(Q, 1), sd), dtype=fac.dtype)
    for t in range(T - 1, -1, -1):
        m = fac[t]
        s = np.zeros((Q + 1, sd), dtype=fac.dtype)
        s[0] = m[0]
        if Q > 0:
            for k in range(1, Q + 1):
                acc = m[1] * Z[0, k - 1]
                for j in range(2, Q + 1 if defect != "drop_j2" else 2):
                    acc = acc + m[j] * Z[j - 1, k - 1]
                if t + k < T:
                    s[k] = -acc
            acc = m[1] * s[1]
            for j in range(2, Q + 1):
                acc = acc + m[j] * s[j]
            s[0] = m[0] - acc
            for i in range(Q - 1, 0, -1):
                for j in range(Q - 1, 0, -1):
                    Z[i, j] = Z[i - 1, j - 1]
            for j in range(1, Q):
                Z[0, j] = s[j]
                Z[j, 0] = s[j]
            Z[0, 0] = s[0]
        band[:, t] = s
    return band


def covariance(var, windows, T, sd, edge_rule=True, defect=None, work=np.float64):
    """One utterance: (band (Q + 1, T, sd), logdet (sd), status (sd)); a failed system's band and logdet are NaN."""
    tau = precisions(var, windows, T, sd, edge_rule)
    fac, ld, status = factor(assemble(tau, windows, work), defect)
    with np.errstate(all="ignore"):
        band = selected_inverse(fac, defect)
    band[:, :, status != 0] = np.nan
    ld[status != 0] = np.nan
    return band, ld, status


def covariance_batch(variances, windows, lengths, B, Tmax, sd, want_band=True):
    """The padded batch: band (Q + 1, B, Tmax, sd) float64 with zeros at or past T, logdet (B, sd), status (B, sd) int32."""
    _, Q, _ = window_set(windows)
    live = live_frames(lengths, B, Tmax)
    band = np.zeros((Q + 1, B, Tmax, sd))
    logdet = np.zeros((B, sd))
    status = np.zeros((B, sd), dtype=np.int32)
    mode = var_mode_of(variances)
    for b in range(B):
        T = int(live[b])
        v = None if mode == VAR_UNIT else (variances if mode == VAR_GLOBAL else variances[b])
        bb, logdet[b], status[b] = covariance(v, windows, T, sd)
        band[:, b, :T] = bb
    return (band if want_band else None), logdet, status


def band_to_dense(band, T):
    """(sd, T, T) symmetric matrices whose band is `band` (Q + 1, >= T, sd); zero outside it."""
    Q1, _, sd = band.shape
    S = np.zeros((sd, T, T), dtype=band.dtype)
    for k in range(Q1):
        for t in range(T - k):
            S[:, t, t + k] = band[k, t]
            S[:, t + k, t] = band[k, t]
    return S


def band_get(band, p, q):
    """S[p, q] (any order) from the band; the pair has to lie inside it."""
    lo, hi = (p, q) if p <= q else (q, p)
    return band[hi - lo, lo]


def band_get_transposed(band, p, q):
    """The planted defect: the band read as S[t + k, t] stored at row t + k."""
    lo, hi = (p, q) if p <= q else (q, p)
    return band[hi - lo, hi] if hi < band.shape[1] else 0.0 * band[0, 0]


# ---- the likelihood ---------------------------------------------------------------------------------------------------------------

def nll_utterance(mean, var, windows, cbar, target, band, logdet, T, sd, dtype, want_grad=True, get=band_get):
    """One utterance in the kernel's order: (nll (sd), grad_means (T, D) dtype, grad_tau-based grad_vars (T, D) float64 BEFORE the
    cast, the four-way partial sums of grad_vars per window (nw, sd)).  Frames are walked in four runs of ceil(T / 4)."""
    ws, Q, mw = window_set(windows)
    nw = len(ws)
    D = nw * sd
    tau = precisions(var, windows, T, sd)
    cb = np.asarray(cbar[:T], dtype=np.float64)
    e = np.asarray(target[:T], dtype=np.float64) - cb
    mu = np.asarray(mean[:T], dtype=np.float64)
    gm = np.zeros((T, D), dtype=dtype)
    gv = np.zeros((T, D))
    per = (T + 3) // 4
    quad = np.zeros((4, sd))
    gsum = np.zeros((4, nw, sd))
    for v in range(4):
        for t in range(min(v * per, T), min(v * per + per, T)):
            for w, (l, u, c) in enumerate(ws):
                av = np.zeros(sd)
                gc = np.zeros(sd)
                for s in range(-1, 2):
                    if -l <= s <= u and 0 <= t + s < T:
                        av = av + c[l + s] * e[t + s]
                        gc = gc + c[l + s] * cb[t + s]
                tw = tau[w, t]
                aa = av * av
                quad[v] = quad[v] + tw * aa
                cols = slice(w * sd, (w + 1) * sd)
                gm[t, cols] = (-(tw * av)).astype(dtype)
                if want_grad:
                    forced = w != 0 and (mw == 0 or t < mw or t >= T - mw)
                    if not forced:
                        cov = np.zeros(sd)
                        for i in range(-1, 2):
                            for j in range(-1, 2):
                                if -l <= i <= u and -l <= j <= u and 0 <= t + i < T and 0 <= t + j < T:
                                    cov = cov + (c[l + i] * c[l + j]) * get(band, t + i, t + j)
                        gtau = (0.5 * aa - av * (mu[t, cols] - gc)) - 0.5 * cov
                        gv[t, cols] = -((tw * tw) * gtau)
                    gsum[v, w] = gsum[v, w] + gv[t, cols]
    q = ((quad[0] + quad[1]) + quad[2]) + quad[3]
    nll = (0.5 * q - 0.5 * logdet) + (0.5 * float(T)) * LOG_2PI
    return nll, gm, gv, ((gsum[0] + gsum[1]) + gsum[2]) + gsum[3]


def nll_batch(means, variances, windows, cbar, target, lengths, band, logdet, want_grad=True):
    """The padded batch: nll (B, sd) float64, grad_means (B, Tmax, D) and grad_vars (like the variances; None for unit ones) in
    the inputs' dtype, zeros at or past T.  Without want_grad the band is not read and may be None."""
    B, Tmax, D = means.shape
    nw = len(windows)
    sd = D // nw
    live = live_frames(lengths, B, Tmax)
    mode = var_mode_of(variances)
    nll = np.zeros((B, sd))
    gm = np.zeros((B, Tmax, D), dtype=means.dtype)
    gv = np.zeros((B, Tmax, D))
    part = np.zeros((B, nw, sd))
    for b in range(B):
        T = int(live[b])
        v = None if mode == VAR_UNIT else (variances if mode == VAR_GLOBAL else variances[b])
        nll[b], gm[b, :T], gv[b, :T], part[b] = nll_utterance(means[b], v, windows, cbar[b], target[b], None if band is None else band[:, b], logdet[b], T, sd,
                                                              means.dtype, want_grad and mode != VAR_UNIT)
    if mode == VAR_UNIT or not want_grad:
        return nll, gm, None
    if mode == VAR_FRAME:
        return nll, gm, gv.astype(means.dtype)
    s = np.zeros((nw, sd))
    for b in range(B):
        s = s + part[b]
    return nll, gm, s.reshape(D).astype(means.dtype)


def mean_trajectory(mean, var, windows, T, sd):
    """cbar = R^-1 r of one utterance by the dense definition, float64 (T, sd)."""
    from nnmnkwii_amd.paramgen import build_win_mats, full_window_mat
    tau = precisions(var, windows, T, sd)
    nw = len(windows)
    W = full_window_mat(build_win_mats(windows, T), T).reshape(nw, T, T)
    R, _, _ = dense_definition(var, windows, T, sd)
    out = np.zeros((T, sd))
    for d in range(sd):
        r = sum(W[w].T @ (tau[w, :, d] * np.asarray(mean[:T, w * sd + d], dtype=np.float64)) for w in range(nw))
        out[:, d] = np.linalg.solve(R[d], r) if T else 0.0
    return out


def nll_dense(tau, mu, windows, target):
    """The likelihood of ONE system as a dense expression on torch float64 tensors (differentiable): tau, mu (nw, T), target (T)."""
    import torch
    nw, T = tau.shape
    W = torch.zeros((nw, T, T), dtype=torch.float64)
    for w, (l, u, c) in enumerate(windows):
        for t in range(T):
            for k in range(-l, u + 1):
                if 0 <= t + k < T:
                    W[w, t, t + k] = float(c[l + k])
    R = sum(W[w].T @ (tau[w][:, None] * W[w]) for w in range(nw))
    r = sum(W[w].T @ (tau[w] * mu[w]) for w in range(nw))
    cbar = torch.linalg.solve(R, r)
    e = target - cbar
    return 0.5 * (e @ (R @ e)) - 0.5 * torch.logdet(R) + 0.5 * T * LOG_2PI


# ---- the truth in extended precision ------------------------------------------------------------------------------------------------

def _inverse_exact(R):
    """Inverse and determinant of a matrix of Fractions by Gauss-Jordan elimination (R is positive definite: no pivoting)."""
    n = len(R)
    A = [list(R[i]) + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    det = Fraction(1)
    for i in range(n):
        p = A[i][i]
        det *= p
        A[i] = [x / p for x in A[i]]
        for r in range(n):
            if r != i and A[r][i] != 0:
                f = A[r][i]
                A[r] = [x - f * y for x, y in zip(A[r], A[i])]
    return [row[n:] for row in A], det


def _to_longdouble(x):
    """A Fraction as numpy.longdouble: its float64 rounding plus the float64 rounding of what that leaves."""
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - Fraction(hi)))


def truth(var, windows, T, sd):
    """(S band (Q + 1, T, sd), logdet (sd)) of the float64 tau and coefficients in extended precision, as numpy.longdouble."""
    ws, Q, _ = window_set(windows)
    tau = precisions(var, windows, T, sd)
    if T > 12:
        fac, ld, status = factor(assemble(tau, windows, np.longdouble))
        assert not status.any()
        return selected_inverse(fac), ld
    band = np.zeros((Q + 1, T, sd), dtype=np.longdouble)
    ld = np.zeros(sd, dtype=np.longdouble)
    for d in range(sd):
        R = [[Fraction(0)] * T for _ in range(T)]
        for w, (l, u, c) in enumerate(ws):
            for t in range(T):
                tw = Fraction(float(tau[w, t, d]))
                for i in range(-l, u + 1):
                    for j in range(-l, u + 1):
                        if 0 <= t + i < T and 0 <= t + j < T:
                            R[t + i][t + j] += Fraction(float(c[l + i])) * Fraction(float(c[l + j])) * tw
        if T:
            S, det = _inverse_exact(R)
            for k in range(Q + 1):
                for t in range(T - k):
                    band[k, t, d] = _to_longdouble(S[t][t + k])
            # log of a rational: the binary exponent apart, so that nothing overflows or cancels
            ex = det.numerator.bit_length() - det.denominator.bit_length()
            ld[d] = np.log(_to_longdouble(det / Fraction(2) ** ex)) + np.longdouble(ex) * np.log(np.longdouble(2))
    return band, ld
