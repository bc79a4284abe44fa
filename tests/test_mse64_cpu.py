"""oracle/mse64.py (the float64 reference of mlpg_hip_unit_mse_step) against the dense definition, no GPU.

The dense definition of the unit-variance step (paramgen/_mlpg.py:297-373 without the float32 cast, around nn.MSELoss):
y = R mu, R = P^-1 [mask W_w]^T, P = sum_w (mask W_w)^T W_w, the edge mask at each utterance's own length; loss =
sum (y - target)^2 / n_elems over live frames; d loss / d mu = R^T 2 (y - target) / n_elems."""
import numpy as np
import pytest

from cases import WINDOW_SETS
from oracle import mlpg as O
from oracle.mse64 import unit_mse_step64

EXTRA_SETS = {
    "fwd2": [(0, 0, np.array([1.0])), (0, 1, np.array([-1.0, 1.0]))],
    "std3-s2": [(0, 0, np.array([2.0]))] + WINDOW_SETS["std3"][1:],
    "dynamic-x4": [(0, 0, np.array([1.0])), (1, 1, 4.0 * np.array([-0.5, 0.0, 0.5])), (1, 1, 4.0 * np.array([1.0, -2.0, 1.0]))],
}
ALL_SETS = dict(WINDOW_SETS, **EXTRA_SETS)


def _dense_R(windows, T):
    """R = P^-1 [mask W_w]^T in float64 for one utterance of T frames: (T, nw T)."""
    nw = len(windows)
    mw = int(max(max(l, u) for l, u, _ in windows))
    mask = O._edge_mask(T, mw)
    Ws = [O.window_matrix(l, u, np.asarray(c, dtype=np.float64), T) for (l, u, c) in windows]
    Wt = [W if w == 0 else mask[:, None] * W for w, W in enumerate(Ws)]
    P = sum(Wt[w].T @ Ws[w] for w in range(nw))
    return np.linalg.solve(P, np.concatenate([Wt[w].T for w in range(nw)], axis=1))


def _dense_step(windows, m, t, n_elems):
    """One utterance m (L, D), t (L, sd): y (L, sd), its loss term sum (y - t)^2 / n_elems, gradient (L, D)."""
    L, D = m.shape
    nw = len(windows)
    sd = D // nw
    R = _dense_R(windows, L)
    mu = m.reshape(L, nw, sd).transpose(1, 0, 2).reshape(nw * L, sd)
    y = R @ mu
    e = y - t
    g = (R.T @ (2.0 * e / n_elems)).reshape(nw, L, sd).transpose(1, 0, 2).reshape(L, D)
    return y, float((e * e).sum() / n_elems), g


def _rel(a, b):
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


@pytest.mark.parametrize("wname", sorted(ALL_SETS))
def test_full_length_batches_match_the_dense_definition(wname):
    windows = ALL_SETS[wname]
    nw = len(windows)
    for T in list(range(1, 41)) + [301]:
        sd = 3 if T <= 40 else 2
        rng = np.random.RandomState(T * 7 + nw)
        m = rng.randn(2, T, nw * sd)
        tg = rng.randn(2, T, sd)
        y, loss, grad, st = unit_mse_step64(m, tg, windows)
        assert y.dtype == np.float64 and not st.any()
        n = 2.0 * T * sd
        dl = 0.0
        for b in range(2):
            yd, ld, gd = _dense_step(windows, m[b], tg[b], n)
            dl += ld
            assert _rel(y[b], yd) <= 1e-12, (wname, T, b)
            assert _rel(grad[b], gd) <= 1e-12, (wname, T, b)
        assert abs(loss - dl) <= 1e-12 * dl, (wname, T)


@pytest.mark.parametrize("wname", sorted(ALL_SETS))
def test_ragged_batches_match_the_dense_definition_per_utterance(wname):
    windows = ALL_SETS[wname]
    nw = len(windows)
    mw = int(max(max(l, u) for l, u, _ in windows))
    Tmax, sd = 37, 2
    lengths = np.array([Tmax, 0, 1, 2, 2 * mw, 2 * mw + 1, 20], dtype=np.int32)
    B = len(lengths)
    rng = np.random.RandomState(nw + 11)
    m = rng.randn(B, Tmax, nw * sd)
    tg = rng.randn(B, Tmax, sd)
    pad = np.arange(Tmax)[None, :] >= lengths[:, None]
    m[pad] = 0.0
    tg[pad] = 0.0
    n = float(lengths.sum() * sd) + 5.0          # any divisor: the batch's, not the utterance's
    y, loss, grad, st = unit_mse_step64(m, tg, windows, lengths, n_elems=n)
    assert not st.any()
    dl = 0.0
    for b, L in enumerate(lengths):
        assert not y[b, L:].any() and not grad[b, L:].any(), (wname, b)
        if L == 0:
            continue
        yd, ld, gd = _dense_step(windows, m[b, :L], tg[b, :L], n)
        dl += ld
        assert _rel(y[b, :L], yd) <= 1e-12, (wname, b)
        assert _rel(grad[b, :L], gd) <= 1e-12, (wname, b)
    assert abs(loss - dl) <= 1e-12 * dl
    # padding holds no information: NaN there changes nothing
    m2, tg2 = m.copy(), tg.copy()
    m2[pad] = np.nan
    tg2[pad] = np.nan
    y2, loss2, grad2, _ = unit_mse_step64(m2, tg2, windows, lengths, n_elems=n)
    assert np.array_equal(y2, y) and loss2 == loss and np.array_equal(grad2, grad)


@pytest.mark.parametrize("wname", ["std3", "wide3", "asym2", "fwd2", "zero2"])
def test_gradient_is_the_central_difference_of_the_loss(wname):
    windows = ALL_SETS[wname]
    nw = len(windows)
    Tmax, sd = 12, 2
    lengths = np.array([12, 7], dtype=np.int32)
    rng = np.random.RandomState(5 + nw)
    m = rng.randn(2, Tmax, nw * sd)
    tg = rng.randn(2, Tmax, sd)
    m[1, 7:] = 0.0
    tg[1, 7:] = 0.0
    _, _, grad, _ = unit_mse_step64(m, tg, windows, lengths)
    h = 1e-3
    # edge frames of both utterances (the second one ragged), interior frames, every window
    for b, t, col in [(0, 0, 0), (0, 11, nw * sd - 1), (0, 5, sd), (1, 0, 1), (1, 6, nw * sd - 1), (1, 3, (nw - 1) * sd),
                      (0, 1, (nw - 1) * sd), (1, 5, sd if nw > 1 else 0)]:
        mp, mm = m.copy(), m.copy()
        mp[b, t, col] += h
        mm[b, t, col] -= h
        fd = (unit_mse_step64(mp, tg, windows, lengths)[1] - unit_mse_step64(mm, tg, windows, lengths)[1]) / (2 * h)
        assert abs(fd - grad[b, t, col]) <= 1e-6 * max(abs(grad[b, t, col]), np.abs(grad).max()), (wname, b, t, col, fd)


@pytest.mark.parametrize("wname", ["std3", "std2", "asym2", "wide3"])
def test_float32_loss_is_taken_from_the_rounded_trajectory(wname):
    """The kernels form the error from y rounded to the input dtype: with the reference's own float32 y as the target the
    loss and the gradient are exactly 0 (a loss from the unrounded float64 y would not be)."""
    windows = ALL_SETS[wname]
    nw = len(windows)
    rng = np.random.RandomState(17)
    lengths = np.array([50, 31, 0], dtype=np.int32)
    m = rng.randn(3, 50, nw * 4).astype(np.float32)
    m[1, 31:] = 0
    m[2] = 0
    y, _, _, _ = unit_mse_step64(m, np.zeros((3, 50, 4), np.float32), windows, lengths)
    assert y.dtype == np.float32
    y2, loss, grad, st = unit_mse_step64(m, y, windows, lengths)
    assert np.array_equal(y2, y) and loss == 0.0 and not grad.any() and not st.any()
    # a target one ulp away does give a loss
    _, loss1, _, _ = unit_mse_step64(m, np.nextafter(y, np.float32(np.inf)), windows, lengths)
    assert loss1 > 0.0


@pytest.mark.parametrize("windows,lengths,want", [
    ([(0, 0, [0.0]), (1, 1, [-0.5, 0.0, 0.5])], [0, 1, 2], [0, 1, 1]),
    ([(0, 0, [0.0])], [0, 1, 5], [0, 1, 1]),
])
def test_failing_pivots_zero_the_system_and_leave_it_out_of_the_loss(windows, lengths, want):
    """A static coefficient of 0 makes the first pivot exactly 0 where every dynamic row is masked (and always for a lone
    static window): status k = 1, y and grad columns 0, no loss term."""
    nw = len(windows)
    lengths = np.asarray(lengths, dtype=np.int32)
    B, Tmax, sd = len(lengths), int(lengths.max()), 3
    rng = np.random.RandomState(3)
    m = rng.randn(B, Tmax, nw * sd)
    tg = rng.randn(B, Tmax, sd)
    pad = np.arange(Tmax)[None, :] >= lengths[:, None]
    m[pad] = 0
    tg[pad] = 0
    y, loss, grad, st = unit_mse_step64(m, tg, windows, lengths)
    assert (st == np.asarray(want)[:, None]).all(), st
    assert not y.any() and loss == 0.0 and not grad.any()
    assert np.isfinite(grad).all()


def test_defaults_and_shapes():
    windows = ALL_SETS["std3"]
    rng = np.random.RandomState(1)
    m = rng.randn(2, 9, 6)
    tg = rng.randn(2, 9, 2)
    y, loss, grad, st = unit_mse_step64(m, tg, windows)
    y2, loss2, grad2, _ = unit_mse_step64(m, tg, windows, np.array([9, 9]), n_elems=2 * 9 * 2)
    assert y.shape == (2, 9, 2) and grad.shape == (2, 9, 6) and st.shape == (2, 2) and st.dtype == np.int32
    assert np.array_equal(y, y2) and loss == loss2 and np.array_equal(grad, grad2)
    _, loss3, grad3, _ = unit_mse_step64(m, tg, windows, n_elems=7.0)
    assert abs(loss3 * 7.0 - loss * 36.0) <= 1e-12 * loss3 and np.allclose(grad3 * 7.0, grad * 36.0, rtol=1e-12, atol=0)
