"""tools/trajcov_model.py, the executable specification of K19 (-m "not gpu"): the kernel's recurrences against the literal dense
definition and against the truth in extended precision, the measured constant of the error bound, the identity R S = I from the
band alone at T = 1000, the likelihood and both gradients against torch's float64 autograd of the dense expression, the exact
zeros of the variance gradient on the edge frames, the padded-batch rules, and three planted defects that must be seen."""
import numpy as np
import pytest
import torch

import trajcov_cases as C
from trajcov_cases import TM

LENGTHS = [0, 1, 2, 3, 4, 5, 8, 17]
SD = 2


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


def ratios(wname, mode, T, tight, defect=None, edge_rule=True):
    """(worst band error, worst logdet error) of the recurrences in units of 2^-53 cond_2(R) max|S| and 2^-53 cond_2(R)
    max(1, |logdet|), against the truth in extended precision; the dense definition is held to the same bound on the way."""
    win = C.WINDOWS[wname]
    var = one(wname, mode, T, tight)
    band, ld, status = TM.covariance(var, win, T, SD, edge_rule=edge_rule, defect=defect)
    assert not status.any()
    R, S, ld_dense = TM.dense_definition(var, win, T, SD)
    tband, tld = TM.truth(var, win, T, SD)
    rb = rl = 0.0
    for d in range(SD):
        unit = C.EPS * C.cond2(R[d])
        smax = float(np.abs(tband[:, :, d]).max()) if T else 1.0
        if T:
            rb = max(rb, float(np.abs(band[:, :, d] - tband[:, :, d]).max()) / (unit * smax))
            dense_band = np.stack([np.concatenate([np.diagonal(S[d], k), np.zeros(k)])[:T] for k in range(band.shape[0])])
            assert np.abs(dense_band - tband[:, :, d]).max() <= 64 * unit * smax     # numpy's own inverse: LAPACK's error, not ours
        rl = max(rl, float(abs(ld[d] - tld[d])) / (unit * max(1.0, float(abs(tld[d])))))
        assert abs(ld_dense[d] - tld[d]) <= 64 * unit * max(1.0, float(abs(tld[d])))
    return rb, rl


def test_error_bound_is_the_measured_one():
    """The recurrences against the truth on every case; the largest ratios are printed and must not exceed the recorded ones,
    and the bound is 8 x the recorded worst, rounded up to a power of two."""
    worst_b = worst_l = 0.0
    for wname, mode, T, tight in all_cases():
        rb, rl = ratios(wname, mode, T, tight)
        worst_b, worst_l = max(worst_b, rb), max(worst_l, rl)
    print("worst band ratio %.3f (recorded %.2f), worst logdet ratio %.3f (recorded %.2f), bound c = %g"
          % (worst_b, TM.WORST_RATIO_BAND, worst_l, TM.WORST_RATIO_LOGDET, TM.BOUND_C))
    assert worst_b <= TM.WORST_RATIO_BAND and worst_l <= TM.WORST_RATIO_LOGDET
    assert TM.BOUND_C == 2.0 ** np.ceil(np.log2(8 * max(TM.WORST_RATIO_BAND, TM.WORST_RATIO_LOGDET)))


@pytest.mark.parametrize("wname", list(C.WINDOWS))
@pytest.mark.parametrize("mode", C.MODES)
def test_recurrences_against_the_dense_definition(wname, mode):
    win = C.WINDOWS[wname]
    for T in LENGTHS:
        for tight in ((False, True) if wname == "std3" and mode == TM.VAR_FRAME else (False,)):
            for seed in (1, 2):
                var = one(wname, mode, T, tight, seed)
                band, ld, status = TM.covariance(var, win, T, SD)
                R, S, ld_dense = TM.dense_definition(var, win, T, SD)
                assert not status.any() and band.shape == (TM.window_set(win)[1] + 1, T, SD)
                for d in range(SD):
                    unit = TM.BOUND_C * C.EPS * C.cond2(R[d])
                    Sm = TM.band_to_dense(band, T)[d]
                    inside = np.abs(np.subtract.outer(np.arange(T), np.arange(T))) < band.shape[0]
                    assert np.abs((Sm - S[d])[inside]).max(initial=0.0) <= 2 * unit * np.abs(S[d]).max(initial=1.0), (T, d)
                    assert abs(ld[d] - ld_dense[d]) <= 2 * unit * max(1.0, abs(ld_dense[d]))
                    # the band's rectangle: zeros where t + k >= T
                    for k in range(band.shape[0]):
                        assert (band[k, max(T - k, 0):, d] == 0).all()


def test_short_utterances_are_static_only():
    """T <= 2 mw leaves the static window alone: S is diag(variance); T = 3 has one live dynamic row."""
    win = C.WINDOWS["std3"]
    var = one("std3", TM.VAR_FRAME, 2, False)
    band, ld, _ = TM.covariance(var, win, 2, SD)
    assert np.array_equal(band[0], 1.0 / (1.0 / var[:, :SD])) and (band[1:] == 0).all()
    assert np.allclose(ld, -np.log(var[:, :SD]).sum(axis=0), rtol=1e-14)
    tau = TM.precisions(one("std3", TM.VAR_FRAME, 3, False), win, 3, SD)
    assert (tau[1:, [0, 2]] == 0).all() and (tau[1:, 1] > 0).all()


def test_identity_from_the_band_alone_at_1000_frames():
    """sum_k R[t, t +- k] S[t +- k, t] = 1 for every t: every entry needed lies inside the two bands."""
    T, win = 1000, C.WINDOWS["std3"]
    var = one("std3", TM.VAR_FRAME, T, False)
    band, _, status = TM.covariance(var, win, T, SD)
    pk = TM.assemble(TM.precisions(var, win, T, SD), win)          # pk[f, k] = R[f + k, f]
    assert not status.any()
    Q = band.shape[0] - 1
    acc = pk[:, 0] * band[0]
    for k in range(1, Q + 1):
        acc[:T - k] += pk[:T - k, k] * band[k, :T - k]            # R[t, t + k] S[t + k, t]
        acc[k:] += pk[:T - k, k] * band[k, :T - k]                # R[t, t - k] S[t - k, t]
    R = TM.dense_definition(var, win, 64, SD)[0]
    assert np.abs(acc - 1.0).max() <= TM.BOUND_C * C.EPS * max(C.cond2(R[d]) for d in range(SD)) * 4


def dense_autograd(mean, var, win, target, T, sd, mode):
    """nll (sd) and the gradients for the means (T, D) and the variances (like var) by torch float64 autograd of the dense form."""
    nw = len(win)
    ws, _, mw = TM.window_set(win)
    m = torch.tensor(np.asarray(mean[:T], dtype=np.float64), requires_grad=True)
    v = None if var is None else torch.tensor(np.asarray(var, dtype=np.float64), requires_grad=True)
    edge = torch.ones((nw, T), dtype=torch.float64)
    for w in range(1, nw):
        for t in range(T):
            if mw == 0 or t < mw or t >= T - mw:
                edge[w, t] = 0.0
    out = []
    for d in range(sd):
        cols = [w * sd + d for w in range(nw)]
        if v is None:
            tau = edge.clone()
        elif mode == TM.VAR_GLOBAL:
            tau = edge * (1.0 / v[cols])[:, None]
        else:
            tau = edge * (1.0 / v[:T, cols]).T
        out.append(TM.nll_dense(tau, m[:, cols].T, ws, torch.tensor(np.asarray(target[:T, d], dtype=np.float64))))
    nll = torch.stack(out)
    nll.sum().backward()
    return nll.detach().numpy(), m.grad.numpy(), None if v is None else v.grad.numpy()


def nll_case(wname, mode, T, seed=0, tight=False, get=TM.band_get):
    win = C.WINDOWS[wname]
    nw = len(win)
    var = one(wname, mode, T, tight, seed)
    mean = C.features(seed + 1, 1, T, nw * SD)[0]
    target = C.features(seed + 2, 1, T, SD)[0]
    band, ld, _ = TM.covariance(var, win, T, SD)
    cbar = TM.mean_trajectory(mean, var, win, T, SD)
    got = TM.nll_utterance(mean, var, win, cbar, target, band, ld, T, SD, np.float64, want_grad=mode != TM.VAR_UNIT, get=get)
    want = dense_autograd(mean, var, win, target, T, SD, mode)
    R = TM.dense_definition(var, win, T, SD)[0]
    cond = max([C.cond2(R[d]) for d in range(SD)] + [1.0])
    return got, want, cond, var


@pytest.mark.parametrize("wname", list(C.WINDOWS))
@pytest.mark.parametrize("mode", C.MODES)
def test_likelihood_and_gradients_against_float64_autograd(wname, mode):
    for T in (1, 2, 3, 4, 5, 8, 17):
        (nll, gm, gv, gsum), (nll_t, gm_t, gv_t), cond, var = nll_case(wname, mode, T)
        tol = TM.BOUND_C * C.EPS * cond                    # the bound's own form: c 2^-53 cond_2(R) max|.|
        assert np.abs(nll - nll_t).max() <= tol * max(1.0, np.abs(nll_t).max()), T
        assert np.abs(gm - gm_t).max() <= tol * max(1.0, np.abs(gm_t).max()), T
        if mode == TM.VAR_FRAME:
            assert np.abs(gv - gv_t).max() <= tol * max(1.0, np.abs(gv_t).max()), T
        elif mode == TM.VAR_GLOBAL:
            assert np.abs(gsum.reshape(-1) - gv_t).max() <= tol * max(1.0, np.abs(gv_t).max()), T


def test_variance_gradient_is_exactly_zero_on_the_edge_frames():
    for T in (1, 2, 3, 8):
        (_, _, gv, _), (_, _, gv_t), _, _ = nll_case("std3", TM.VAR_FRAME, T)
        edge = [t for t in range(T) if t < 1 or t >= T - 1]
        assert (gv[edge, SD:] == 0).all() and (gv_t[edge, SD:] == 0).all()
        assert T < 3 or (gv[1:-1, SD:] != 0).all()
        assert (gv[:, :SD] != 0).all()


def test_padded_batch_rules():
    win = C.WINDOWS["std3"]
    B, Tmax, lengths = 3, 9, [9, 0, 4]
    var = C.variances(3, B, Tmax, SD, "std3", TM.VAR_FRAME)
    band, ld, status = TM.covariance_batch(var, win, lengths, B, Tmax, SD)
    assert band.shape == (3, B, Tmax, SD) and (band[:, 1] == 0).all() and (band[:, 2, 4:] == 0).all() and (ld[1] == 0).all()
    alone = TM.covariance(var[2], win, 4, SD)
    assert C.same_bits(band[:, 2, :4], alone[0]) and C.same_bits(ld[2], alone[1])
    var[0, 5, 1] = -1e-3                                           # a negative static variance: a non-positive pivot at frame 6
    band, ld, status = TM.covariance_batch(var, win, lengths, B, Tmax, SD)
    assert status[0, 1] == 6 and status.sum() == 6 and np.isnan(band[:, 0, :, 1]).all() and np.isnan(ld[0, 1])
    assert not np.isnan(band[:, 0, :, 0]).any() and not np.isnan(band[:, 2]).any()


# ---- the comparison bites ----------------------------------------------------------------------------------------------------------

def test_planted_dropped_j2_term_is_caught():
    with pytest.raises(AssertionError):
        for T in (5, 8):
            rb, rl = ratios("std3", TM.VAR_FRAME, T, False, defect="drop_j2")
            assert rb <= TM.BOUND_C
    assert ratios("std3", TM.VAR_FRAME, 8, False)[0] <= TM.BOUND_C


def test_planted_missing_edge_rule_is_caught():
    rb, rl = ratios("std3", TM.VAR_FRAME, 8, False, edge_rule=False)
    assert rb > 1e6 * TM.BOUND_C and rl > 1e6 * TM.BOUND_C


def test_planted_transposed_band_read_is_caught():
    (_, _, gv, _), (_, _, gv_t), cond, _ = nll_case("std3", TM.VAR_FRAME, 8, get=TM.band_get_transposed)
    assert np.abs(gv - gv_t).max() > 1e6 * TM.BOUND_C * C.EPS * cond * np.abs(gv_t).max()
