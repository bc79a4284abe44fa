"""tools/trajsample_model.py, the executable specification of K20 (-m "not gpu"), on K19's grid: the model's draws and whitened
rows against the dense definition (numpy's Cholesky factor of the dense R) and against the truth in extended precision, the
measured constant of the error bound, A A^T = S for the model's map A (the draws have covariance R^-1), whiten(sample(z)) = z,
the quadratic term of trajcov_model's likelihood from the whitened target, the padded-batch rules, and a planted defect that
the bound must catch."""
import os
import sys

import numpy as np
import pytest

import trajcov_cases as C
from trajcov_cases import TM

sys.path.insert(0, os.path.join(C.ROOT, "tools"))
import trajsample_model as SM  # noqa: E402

LENGTHS = [1, 2, 3, 4, 5, 8, 17]
SD, K = 3, 2


def all_cases():
    for wname in C.WINDOWS:
        for mode in C.MODES:
            for T in LENGTHS:
                yield wname, mode, T, False
    for T in LENGTHS:
        yield "std3", TM.VAR_FRAME, T, True


def one(wname, mode, T, tight, seed=0):
    v = C.variances(seed + T, 1, T, SD, wname, mode, tight=tight)
    return v[0] if mode == TM.VAR_FRAME else v


def inputs(T, seed=0):
    rng = np.random.RandomState(100 + seed + T)
    return rng.randn(K, T, SD), rng.randn(T, SD)


def ratios(wname, mode, T, tight, defect=None):
    """(worst draw error, worst whitened-row error) of the recurrences per system in units of 2^-53 cond_2(R) max|x| (max|z|),
    against the truth in extended precision; the dense definition is held to a bound of the same form on the way."""
    win = C.WINDOWS[wname]
    var = one(wname, mode, T, tight)
    z, mean = inputs(T)
    fac, _, status = SM.factor_of(var, win, T, SD)
    assert not status.any()
    x = SM.sample_utterance(fac, z, mean, defect=defect)
    xin = SM.sample_utterance(fac, z, mean)                     # what is whitened: a trajectory of natural size
    w = SM.whiten_utterance(fac, xin, mean, defect=defect)
    tx = SM.truth_sample(var, win, T, SD, z, mean)
    tw = SM.truth_whiten(var, win, T, SD, xin, mean)
    R, Cf = SM.dense_cholesky(var, win, T, SD)
    dx, dw = SM.dense_sample(Cf, z, mean), SM.dense_whiten(Cf, xin, mean)
    rs = rw = 0.0
    for d in range(SD):
        unit = C.EPS * C.cond2(R[d])
        xmax, wmax = float(np.abs(tx[:, :, d]).max()), float(np.abs(tw[:, :, d]).max())
        rs = max(rs, float(np.abs(x[:, :, d] - tx[:, :, d]).max()) / (unit * xmax))
        rw = max(rw, float(np.abs(w[:, :, d] - tw[:, :, d]).max()) / (unit * wmax))
        if defect is None:                                      # numpy's own factor and solve: LAPACK's error, not ours
            assert np.abs(dx[:, :, d] - tx[:, :, d]).max() <= 64 * unit * xmax
            assert np.abs(dw[:, :, d] - tw[:, :, d]).max() <= 64 * unit * max(wmax, float(np.abs(xin[:, :, d] - mean[:, d]).max()))
    return rs, rw


def measured():
    worst_s = worst_w = 0.0
    for wname, mode, T, tight in all_cases():
        rs, rw = ratios(wname, mode, T, tight)
        worst_s, worst_w = max(worst_s, rs), max(worst_w, rw)
    return worst_s, worst_w


def test_error_bound_is_the_measured_one():
    """The recurrences against the truth on every case; the largest ratios are printed and must not exceed the recorded ones,
    and the bound is 8 x the recorded worst, rounded up to a power of two."""
    worst_s, worst_w = measured()
    print("worst draw ratio %.3f (recorded %.2f), worst whitened ratio %.3f (recorded %.2f), bound c = %g"
          % (worst_s, SM.WORST_RATIO_SAMPLE, worst_w, SM.WORST_RATIO_WHITEN, SM.BOUND_C))
    assert worst_s <= SM.WORST_RATIO_SAMPLE and worst_w <= SM.WORST_RATIO_WHITEN
    assert worst_s > 0.9 * SM.WORST_RATIO_SAMPLE and worst_w > 0.9 * SM.WORST_RATIO_WHITEN      # ... and are the recorded ones
    c = 8 * max(SM.WORST_RATIO_SAMPLE, SM.WORST_RATIO_WHITEN)
    assert SM.BOUND_C == 2.0 ** np.ceil(np.log2(c))


@pytest.mark.parametrize("wname", list(C.WINDOWS))
def test_model_agrees_with_the_dense_definition(wname):
    """x = mean + C^-T z and z = C^T (x - mean) with numpy's Cholesky factor C of the dense R, to the bound (LAPACK's own error is
    of the same form, so the two share c 2^-53 cond_2(R) max|.| twice over)."""
    win = C.WINDOWS[wname]
    for mode in C.MODES:
        for T in LENGTHS:
            var = one(wname, mode, T, False)
            z, mean = inputs(T)
            fac, _, _ = SM.factor_of(var, win, T, SD)
            R, Cf = SM.dense_cholesky(var, win, T, SD)
            x = SM.sample_utterance(fac, z, mean)
            dx = SM.dense_sample(Cf, z, mean)
            w = SM.whiten_utterance(fac, x, mean)
            dw = SM.dense_whiten(Cf, x, mean)
            for d in range(SD):
                tol = 2 * SM.BOUND_C * C.EPS * C.cond2(R[d])
                assert np.abs(x[:, :, d] - dx[:, :, d]).max() <= tol * np.abs(dx[:, :, d]).max()
                assert np.abs(w[:, :, d] - dw[:, :, d]).max() <= tol * max(np.abs(dw[:, :, d]).max(), np.abs(x[:, :, d] - mean[:, d]).max())


def test_the_draws_have_covariance_S():
    """A = the model's map applied to the identity (column j: the draw of z = e_j, mean 0); A A^T is R^-1."""
    for wname, mode, T, tight in all_cases():
        win = C.WINDOWS[wname]
        var = one(wname, mode, T, tight)
        fac, _, _ = SM.factor_of(var, win, T, SD)
        ident = np.repeat(np.eye(T)[:, :, None], SD, axis=2)                   # (K = T, T, sd): draw j is e_j
        A = SM.sample_utterance(fac, ident)                                    # A[j, t, d] = (L^-T D^-1/2)[t, j]
        R, S, _ = TM.dense_definition(var, win, T, SD)
        for d in range(SD):
            M = A[:, :, d].T
            tol = 2 * SM.BOUND_C * C.EPS * C.cond2(R[d]) * np.abs(S[d]).max() * T
            assert np.abs(M @ M.T - S[d]).max() <= tol, (wname, mode, T, tight, d)
            assert np.array_equal(M, np.triu(M))                               # L^-T is upper triangular


def test_whiten_inverts_sample_and_gives_the_likelihood():
    for wname, mode, T, tight in all_cases():
        win = C.WINDOWS[wname]
        nw = len(win)
        var = one(wname, mode, T, tight)
        z, mean = inputs(T)
        fac, ld, _ = SM.factor_of(var, win, T, SD)
        R = TM.dense_definition(var, win, T, SD)[0]
        x = SM.sample_utterance(fac, z, mean)
        back = SM.whiten_utterance(fac, x, mean)
        for d in range(SD):
            tol = 2 * SM.BOUND_C * C.EPS * C.cond2(R[d]) * max(1.0, np.abs(z[:, :, d]).max())
            assert np.abs(back[:, :, d] - z[:, :, d]).max() <= tol, (wname, mode, T, tight)
        # 1/2 sum z^2 - 1/2 logdet + T/2 log 2 pi for z = whiten(target) is trajcov_model's likelihood of the target
        target = x[0]
        w = SM.whiten_utterance(fac, target[None], mean)[0]
        nll = 0.5 * (w * w).sum(axis=0) - 0.5 * ld + 0.5 * T * TM.LOG_2PI
        means = np.zeros((T, nw * SD))
        want = TM.nll_utterance(means, var, win, mean, target, None, ld, T, SD, np.float64, want_grad=False)[0]
        for d in range(SD):
            quad = float((w[:, d] ** 2).sum())
            assert abs(nll[d] - want[d]) <= 4 * SM.BOUND_C * C.EPS * C.cond2(R[d]) * max(1.0, quad, abs(want[d])), (wname, mode, T, tight, d)


def test_padded_batch_rules():
    win = C.WINDOWS["std3"]
    B, Tmax, lengths = 3, 9, [9, 0, 5]
    var = C.variances(4, B, Tmax, SD, "std3", TM.VAR_FRAME)
    var[2, 3, 1] = -1e-3                                                        # utterance 2, dim 1: a non-positive pivot
    for b, T in enumerate(lengths):
        var[b, T:] = np.nan
    fac, logdet, status = SM.factor_batch(var, win, lengths, B, Tmax, SD)
    band, klog, kstat = TM.covariance_batch(var, win, lengths, B, Tmax, SD)
    assert np.array_equal(status, kstat) and status[2, 1] == 4 and status.sum() == 4 and C.same_bits(logdet, klog)
    assert (fac[:, 1] == 0).all() and (fac[:, 2, 5:] == 0).all() and np.isnan(fac[:, 2, :5, 1]).all()
    assert np.isfinite(fac[:, 2, :5, 0]).all() and np.isfinite(fac[:, 0]).all()
    rng = np.random.RandomState(0)
    z, mean = rng.randn(K, B, Tmax, SD), rng.randn(B, Tmax, SD)
    for b, T in enumerate(lengths):
        z[:, b, T:] = np.nan
        mean[b, T:] = np.nan
    for dt in (np.float32, np.float64):
        x = SM.sample_batch(fac, status, lengths, z.astype(dt), mean.astype(dt))
        assert x.dtype == dt and (x[:, 1] == 0).all() and (x[:, 2, 5:] == 0).all() and np.isnan(x[:, 2, :5, 1]).all()
        assert np.isfinite(x[:, 0]).all() and np.isfinite(x[:, 2, :5, 0]).all()
        w = SM.whiten_batch(fac, status, lengths, x, mean.astype(dt))
        assert (w[:, 1] == 0).all() and (w[:, 2, 5:] == 0).all() and np.isnan(w[:, 2, :5, 1]).all()
        assert np.abs(w[:, 0] - z[:, 0]).max() < (1e-4 if dt == np.float32 else 1e-12)
        # a draw's bits depend neither on K nor on the mean's presence in another draw
        alone = SM.sample_batch(fac, status, lengths, z[1:].astype(dt), mean.astype(dt))
        assert C.same_bits(alone[0], x[1])


def test_planted_dropped_j2_term_is_caught():
    """The j = 2 term of either recurrence dropped: far outside the bound wherever Q = 2 and T >= 3; unseen where Q < 2."""
    for wname, expect in (("std3", True), ("std2", True), ("asym", False), ("static", False)):
        rs, rw = ratios(wname, TM.VAR_FRAME, 17, False, defect="drop_j2")
        assert (rs > SM.BOUND_C) == expect and (rw > SM.BOUND_C) == expect, (wname, rs, rw)
    rs, rw = ratios("std3", TM.VAR_FRAME, 17, False)
    assert rs <= SM.BOUND_C and rw <= SM.BOUND_C


def test_extended_square_root():
    from fractions import Fraction
    for q in (Fraction(2), Fraction(1, 3), Fraction(10 ** 30 + 7, 3), Fraction(1, 10 ** 30 + 9), Fraction(9, 4)):
        r = SM.sqrt_fraction(q)
        assert 0 <= q - r * r <= q * Fraction(1, 2 ** 150)
    assert SM.sqrt_fraction(Fraction(9, 4)) == Fraction(3, 2) and SM.sqrt_fraction(Fraction(0)) == 0
