"""Executable specification of K20 (csrc/mlpg_trajsample.hip, include/nnmnkwii_sample.h): draws from MLPG's trajectory
distribution N(c; cbar, R^-1) and the whitening map.  numpy only; everything about R, tau and the banded factor comes from
``trajcov_model`` (K19), which this module imports and does not change.

With R = L D L^T (``trajcov_model.factor``: fac[t, 0] = 1 / D_t, fac[t, k] = l_{t+k,t}):

* ``sample_utterance``: x_t = z_t sqrt(fac[t, 0]) - fac[t, 1] x_{t+1} - fac[t, 2] x_{t+2}, t = T - 1 .. 0, in the kernel's order of
  operations (every product and every difference rounded on its own; terms with t + j >= T absent), out = mean + x rounded once
  to the dtype; ``whiten_utterance``: z_t = (e_t + fac[t, 1] e_{t+1} + fac[t, 2] e_{t+2}) / sqrt(fac[t, 0]), e = x - mean.
* ``factor_batch``, ``sample_batch``, ``whiten_batch``: padded batches, the planar layout, zeros at or past T, NaN below T for a
  system whose status is not 0.
* ``dense_sample``, ``dense_whiten``: the definition -- ``numpy.linalg.cholesky`` of ``trajcov_model.dense_definition``'s R
  (R = C C^T, C = L D^1/2): x = C^-T z, z = C^T x.
* ``truth_sample``, ``truth_whiten``: in extended precision: above T = 12 the same recurrences in ``numpy.longdouble``; at or below
  it L D L^T in exact rationals (``fractions.Fraction``), the square roots to SQRT_BITS bits by integer square root, and the
  substitution in exact rationals again.

Error of the recurrences, MEASURED (tests/test_trajsample_model.py, K19's grid: T in {1, 2, 3, 4, 5, 8, 17}, four window sets,
three variance modes and the tight case, sd = 3, two draws): the largest |x_model - x_truth| / (2^-53 cond_2(R) max|x|) seen is
WORST_RATIO_SAMPLE, the same for the whitened rows WORST_RATIO_WHITEN; the bound the tests use is BOUND_C = 8 x the larger of the
two, rounded up to a power of two.  The margin covers other seeds, not other algorithms."""
from fractions import Fraction
from math import isqrt

import numpy as np

import trajcov_model as TM

EPS = TM.EPS
SQRT_BITS = 160
WORST_RATIO_SAMPLE = 1.54     # measured 1.536: see the docstring and tests/test_trajsample_model.py::test_error_bound_is_the_measured_one
WORST_RATIO_WHITEN = 1.55     # measured 1.541
BOUND_C = 16.0                # 8 x 1.55 = 12.4 -> 16


def factor_of(var, windows, T, sd, work=np.float64):
    """(fac (T, Q + 1, sd), logdet (sd), status (sd)) of one utterance: trajcov_model's assemble and factor."""
    return TM.factor(TM.assemble(TM.precisions(var, windows, T, sd), windows, work))


def sample_utterance(fac, z, mean=None, dtype=np.float64, defect=None):
    """fac (T, Q + 1, sd); z (K, T, sd) (any float dtype: used as float64, or as fac's dtype if that is wider); mean (T, sd) or
    None.  Returns out (K, T, sd) of `dtype`.  defect "drop_j2": the planted defect of the tests."""
    T, Q1, sd = fac.shape
    Q = Q1 - 1
    work = fac.dtype
    z = np.asarray(z).astype(work)
    K = z.shape[0]
    x = np.zeros((K, T, sd), dtype=work)
    out = np.zeros((K, T, sd), dtype=dtype)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            sq = np.sqrt(fac[t, 0])
            xt = z[:, t] * sq
            if Q >= 1 and t + 1 < T:
                xt = xt - fac[t, 1] * x[:, t + 1]
            if Q >= 2 and t + 2 < T and defect != "drop_j2":
                xt = xt - fac[t, 2] * x[:, t + 2]
            x[:, t] = xt
            out[:, t] = (xt if mean is None else np.asarray(mean[t]).astype(work) + xt).astype(dtype)
    return out


def whiten_utterance(fac, x, mean=None, dtype=np.float64, defect=None):
    """The inverse map: x (K, T, sd) -> z (K, T, sd) of `dtype`."""
    T, Q1, sd = fac.shape
    Q = Q1 - 1
    work = fac.dtype
    e = np.asarray(x).astype(work)
    if mean is not None:
        e = e - np.asarray(mean[:T]).astype(work)[None]
    z = np.zeros(e.shape, dtype=dtype)
    with np.errstate(all="ignore"):
        for t in range(T):
            acc = e[:, t]
            if Q >= 1 and t + 1 < T:
                acc = acc + fac[t, 1] * e[:, t + 1]
            if Q >= 2 and t + 2 < T and defect != "drop_j2":
                acc = acc + fac[t, 2] * e[:, t + 2]
            z[:, t] = (acc / np.sqrt(fac[t, 0])).astype(dtype)
    return z


def factor_batch(variances, windows, lengths, B, Tmax, sd):
    """The padded batch: factor (Q + 1, B, Tmax, sd) float64 -- zeros at or past T, NaN below T for a failed system --, logdet
    (B, sd) (NaN for a failed system), status (B, sd) int32."""
    _, Q, _ = TM.window_set(windows)
    live = TM.live_frames(lengths, B, Tmax)
    fac = np.zeros((Q + 1, B, Tmax, sd))
    logdet = np.zeros((B, sd))
    status = np.zeros((B, sd), dtype=np.int32)
    mode = TM.var_mode_of(variances)
    for b in range(B):
        T = int(live[b])
        v = None if mode == TM.VAR_UNIT else (variances if mode == TM.VAR_GLOBAL else variances[b])
        f, ld, status[b] = factor_of(v, windows, T, sd)
        f[:, :, status[b] != 0] = np.nan
        ld[status[b] != 0] = np.nan
        fac[:, b, :T] = f.transpose(1, 0, 2)
        logdet[b] = ld
    return fac, logdet, status


def _draw_batch(one, fac, status, lengths, src, mean):
    """sample_batch / whiten_batch: src (K, B, Tmax, sd) of the dtype; rows at or past T of src and mean are not looked at."""
    K, B, Tmax, sd = src.shape
    live = TM.live_frames(lengths, B, Tmax)
    out = np.zeros(src.shape, dtype=src.dtype)
    for b in range(B):
        T = int(live[b])
        f = np.ascontiguousarray(fac[:, b, :T].transpose(1, 0, 2))
        o = one(f, src[:, b, :T], None if mean is None else mean[b, :T], src.dtype)
        o[:, :, status[b] != 0] = np.nan
        out[:, b, :T] = o
    return out


def sample_batch(fac, status, lengths, noise, mean=None):
    """nnmk_draw_sample: out (K, B, Tmax, sd) of the noise's dtype."""
    return _draw_batch(sample_utterance, fac, status, lengths, noise, mean)


def whiten_batch(fac, status, lengths, x, mean=None):
    """nnmk_draw_whiten: z (K, B, Tmax, sd) of x's dtype."""
    return _draw_batch(whiten_utterance, fac, status, lengths, x, mean)


# ---- the definition -------------------------------------------------------------------------------------------------------------------

def dense_cholesky(var, windows, T, sd):
    """(R (sd, T, T), C (sd, T, T) lower with R = C C^T) by numpy.linalg.cholesky of trajcov_model.dense_definition's R."""
    R, _, _ = TM.dense_definition(var, windows, T, sd)
    C = np.stack([np.linalg.cholesky(R[d]) for d in range(sd)]) if T else np.zeros((sd, 0, 0))
    return R, C


def dense_sample(C, z, mean=None):
    """x = mean + C^-T z: z (K, T, sd) -> (K, T, sd)."""
    x = np.zeros(z.shape)
    for d in range(z.shape[2]):
        if z.shape[1]:
            x[:, :, d] = np.linalg.solve(C[d].T, z[:, :, d].T).T
    return x if mean is None else mean[None] + x


def dense_whiten(C, x, mean=None):
    e = x if mean is None else x - mean[None]
    return np.stack([e[:, :, d] @ C[d] for d in range(e.shape[2])], axis=2) if e.shape[2] else np.zeros(e.shape)


# ---- the truth in extended precision ----------------------------------------------------------------------------------------------------

def sqrt_fraction(q, bits=SQRT_BITS):
    """sqrt of a non-negative Fraction as a Fraction, rounded down at `bits` bits behind the binary point of sqrt(n d)."""
    if q == 0:
        return Fraction(0)
    n, d = q.numerator, q.denominator
    return Fraction(isqrt((n * d) << (2 * bits)), d << bits)   # sqrt(n / d) = sqrt(n d) / d


def _exact_factor(var, windows, T, d, sd):
    """L D L^T of system d in exact rationals: (D_t, l[t][k] = l_{t+k,t}, Q)."""
    ws, Q, _ = TM.window_set(windows)
    tau = TM.precisions(var, windows, T, sd)
    R = [[Fraction(0)] * T for _ in range(T)]
    for w, (l, u, c) in enumerate(ws):
        for t in range(T):
            tw = Fraction(float(tau[w, t, d]))
            for i in range(-l, u + 1):
                for j in range(-l, u + 1):
                    if 0 <= t + i < T and 0 <= t + j < T:
                        R[t + i][t + j] += Fraction(float(c[l + i])) * Fraction(float(c[l + j])) * tw
    Dg, Lm = [Fraction(0)] * T, [[Fraction(0)] * (Q + 1) for _ in range(T)]
    for t in range(T):
        Dg[t] = R[t][t]
        for k in range(1, Q + 1):
            if t + k < T:
                Lm[t][k] = R[t + k][t] / Dg[t]
        for i in range(1, Q + 1):
            for j in range(1, i + 1):
                if t + i < T:
                    R[t + i][t + j] -= Lm[t][i] * Lm[t][j] * Dg[t]
                    R[t + j][t + i] = R[t + i][t + j]
    return Dg, Lm, Q


def _truth(var, windows, T, sd, src, mean, whiten):
    src = np.asarray(src, dtype=np.float64)
    K = src.shape[0]
    if T > 12:
        fac, _, status = factor_of(var, windows, T, sd, np.longdouble)
        assert not status.any()
        m = None if mean is None else np.asarray(mean, dtype=np.float64)
        return (whiten_utterance if whiten else sample_utterance)(fac, src, m, np.longdouble)
    out = np.zeros((K, T, sd), dtype=np.longdouble)
    for d in range(sd):
        Dg, Lm, Q = _exact_factor(var, windows, T, d, sd)
        sq = [sqrt_fraction(1 / Dg[t]) for t in range(T)]          # D_t^-1/2
        for k in range(K):
            mu = [Fraction(0) if mean is None else Fraction(float(mean[t, d])) for t in range(T)]
            v = [Fraction(float(src[k, t, d])) for t in range(T)]
            r = [Fraction(0)] * T
            if whiten:
                e = [v[t] - mu[t] for t in range(T)]
                for t in range(T):
                    r[t] = (e[t] + sum(Lm[t][j] * e[t + j] for j in range(1, Q + 1) if t + j < T)) / sq[t]
            else:
                for t in range(T - 1, -1, -1):
                    r[t] = v[t] * sq[t] - sum(Lm[t][j] * r[t + j] for j in range(1, Q + 1) if t + j < T)
                r = [r[t] + mu[t] for t in range(T)]
            for t in range(T):
                out[k, t, d] = TM._to_longdouble(r[t])
    return out


def truth_sample(var, windows, T, sd, z, mean=None):
    """The draws (K, T, sd) of the float64 tau, coefficients, noise and mean in extended precision, as numpy.longdouble."""
    return _truth(var, windows, T, sd, z, mean, False)


def truth_whiten(var, windows, T, sd, x, mean=None):
    return _truth(var, windows, T, sd, x, mean, True)
