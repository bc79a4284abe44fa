"""CPU tests (no GPU): tests/vargrad64.py, the float64 anchor of the variance gradient, against a dense restatement.

Float64 inputs: complex-step derivatives of a dense float64 MLPG (P and b from oracle.mlpg.window_matrix truncated at each
length, solved in complex arithmetic): Im L(var + i h V) / h with h = 1e-30 and L = <grad_out, y> is <grad_var, V> to machine
precision, with no cancellation.  Float32 inputs: the same dense restatement in real arithmetic with tau rounded to float32
first (a complex step cannot model that rounding).  Then grad_mean against oracle.grad64, the scale invariant, global = the sum
of frame mode, exact zeros, and two deliberately wrong variants of the helper that these checks catch."""
import numpy as np
import pytest

import vargrad64
from cases import WINDOW_SETS
from oracle.grad64 import mlpg_grad64
from oracle.mlpg import window_matrix

WNAMES = ["static", "std2", "std3", "wide3", "zero2", "asym2"]


def _masks(windows, L):
    """Edge mask per window for an utterance of L frames (w >= 1: 0 where t < mw or t >= L - mw; the whole column if mw == 0)."""
    mw = max(max(l, u) for l, u, _ in windows)
    out = []
    for w in range(len(windows)):
        m = np.ones(L)
        if w >= 1:
            if mw == 0:
                m[:] = 0
            else:
                m[:mw] = 0
                m[max(L - mw, 0):] = 0
        out.append(m)
    return out


def _dense_loss(means, tau_fn, grad_out, windows, lengths):
    """L = sum_{b,d} <grad_out[b, :L, d], y_{b,d}> with y from the dense system; tau_fn(b, w, d, L) gives tau_w (unmasked)."""
    B, T, D = means.shape
    nw = len(windows)
    sd = D // nw
    total = 0.0
    for b in range(B):
        L = int(lengths[b])
        if L == 0:
            continue
        Ws = [window_matrix(l, u, np.asarray(c, dtype=np.float64), L) for l, u, c in windows]
        masks = _masks(windows, L)
        for d in range(sd):
            taus = [tau_fn(b, w, d, L) * masks[w] for w in range(nw)]
            P = sum(W.T @ (t[:, None] * W) for W, t in zip(Ws, taus))
            rhs = sum(W.T @ (t * means[b, :L, w * sd + d]) for w, (W, t) in enumerate(zip(Ws, taus)))
            y = np.linalg.solve(P, rhs)
            total = total + grad_out[b, :L, d] @ y
    return total


def _dense_var_grad_real(means, var, grad_out, windows, lengths, tau_dtype):
    """grad_var by the dense formula in real arithmetic, tau = 1/var evaluated in tau_dtype: (B, T, D) or (D,)."""
    B, T, D = means.shape
    nw = len(windows)
    sd = D // nw
    glob = var.ndim == 1
    out = np.zeros((B, T, D))
    one = np.dtype(tau_dtype).type(1)
    for b in range(B):
        L = int(lengths[b])
        if L == 0:
            continue
        Ws = [window_matrix(l, u, np.asarray(c, dtype=np.float64), L) for l, u, c in windows]
        masks = _masks(windows, L)
        for d in range(sd):
            taus = []
            for w in range(nw):
                v = var[w * sd + d] if glob else var[b, :L, w * sd + d]
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = np.broadcast_to((one / np.asarray(v, dtype=tau_dtype)).astype(np.float64), (L,))
                taus.append(np.where(masks[w] != 0, t, 0.0))
            P = sum(W.T @ (t[:, None] * W) for W, t in zip(Ws, taus))
            mu = [np.asarray(means[b, :L, w * sd + d], dtype=np.float64) for w in range(nw)]
            y = np.linalg.solve(P, sum(W.T @ (t * m) for W, t, m in zip(Ws, taus, mu)))
            z = np.linalg.solve(P, np.asarray(grad_out[b, :L, d], dtype=np.float64))
            for w, (W, t) in enumerate(zip(Ws, taus)):
                out[b, :L, w * sd + d] = np.where(t != 0, -t * t * (W @ z) * (mu[w] - W @ y), 0.0)
    return out.sum(axis=(0, 1)) if glob else out


def _case(wname, T, B, sd, seed, dt=np.float64):
    windows = WINDOW_SETS[wname]
    D = len(windows) * sd
    rng = np.random.RandomState(seed)
    means = rng.randn(B, T, D).astype(dt)
    var = (rng.rand(B, T, D) + 0.2).astype(dt)
    vg = (rng.rand(D) + 0.2).astype(dt)
    go = rng.randn(B, T, sd).astype(dt)
    lengths = np.array([T, max(T - 1, 0), T // 2, 0][:B], dtype=np.int64)
    return windows, means, var, vg, go, lengths


def _complex_step(means, var, go, windows, lengths, V, h=1e-30):
    """<grad_var, V> by a complex step of the dense float64 MLPG."""
    sd = go.shape[2]
    vc = var.astype(np.complex128) + 1j * h * V
    if var.ndim == 1:
        tau_fn = lambda b, w, d, L: np.full(L, 1.0 / vc[w * sd + d])  # noqa: E731
    else:
        tau_fn = lambda b, w, d, L: 1.0 / vc[b, :L, w * sd + d]  # noqa: E731
    return float(np.imag(_dense_loss(means, tau_fn, go, windows, lengths)) / h)


def _live_unmasked(windows, lengths, T, sd):
    """Boolean (B, T, D): the entries whose precision survives the mask."""
    B = len(lengths)
    nw = len(windows)
    ok = np.zeros((B, T, nw * sd), dtype=bool)
    for b, L in enumerate(lengths):
        for w, m in enumerate(_masks(windows, int(L))):
            ok[b, :int(L), w * sd:(w + 1) * sd] = (m != 0)[:, None]
    return ok


@pytest.mark.parametrize("wname", WNAMES)
def test_complex_step_float64(wname):
    """<grad_var, V> against complex-step derivatives for T = 1..40, ragged batches down to length 0, frame and global
    modes, a random and a coordinate direction, to 1e-12 relative."""
    for T in range(1, 41):
        windows, means, var, vg, go, lengths = _case(wname, T, 4, 2, seed=T)
        B, _, D = means.shape
        rng = np.random.RandomState(100 + T)
        ok = _live_unmasked(windows, lengths, T, 2)
        for v in (var, vg):
            _, _, gv = vargrad64.mlpg_var_grad64(means, v, go, windows, lengths)
            dirs = [rng.randn(*v.shape)]
            if v.ndim == 1:
                dirs.append(np.eye(D)[rng.randint(D)])
            else:
                idx = np.argwhere(ok)
                if len(idx):
                    e = np.zeros(v.shape)
                    e[tuple(idx[rng.randint(len(idx))])] = 1.0
                    dirs.append(e)
            for V in dirs:
                ref = _complex_step(means, v, go, windows, lengths, V)
                got = float(np.sum(gv * V))
                # relative to the terms of the derivative; where they cancel exactly (a static-only window set: y = mu,
                # grad_var = 0) the complex step's own rounding, ~ eps |grad_out| |mu| |V| / var, is the floor
                floor = 1e-14 * np.abs(go).sum() * np.abs(means).max() * np.abs(V).max() / v.min()
                assert abs(got - ref) <= 1e-12 * float(np.sum(np.abs(gv * V))) + floor, (wname, T, v.ndim, got, ref)


@pytest.mark.parametrize("wname", WNAMES)
def test_float32_inputs_against_dense_real(wname):
    """Float32 inputs: tau rounded to float32 before everything else, as the forward forms it -- to 1e-12 of the largest entry."""
    for T in (1, 2, 3, 7, 16, 33):
        windows, means, var, vg, go, lengths = _case(wname, T, 4, 3, seed=7 * T, dt=np.float32)
        for v in (var, vg):
            _, _, gv = vargrad64.mlpg_var_grad64(means, v, go, windows, lengths)
            ref = _dense_var_grad_real(means, v, go, windows, lengths, np.float32)
            assert np.abs(gv - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), (wname, T, v.ndim)


@pytest.mark.parametrize("wname", WNAMES)
def test_grad_mean_matches_grad64(wname):
    for T in (1, 5, 40, 129):
        windows, means, var, vg, go, lengths = _case(wname, T, 4, 3, seed=T + 5)
        for v in (var, vg):
            _, gm, _ = vargrad64.mlpg_var_grad64(means, v, go, windows, lengths)
            ref = mlpg_grad64(v, go, windows, lengths)
            assert np.abs(gm - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1e-300), (wname, T, v.ndim)


@pytest.mark.parametrize("wname", WNAMES)
def test_scale_invariant_per_system(wname):
    """y does not change when every variance of a system is scaled alike: sum_{w,t} var grad_var = 0 per (b, d)."""
    T, sd = 60, 3
    windows, means, var, vg, go, lengths = _case(wname, T, 4, sd, seed=11)
    nw = len(windows)
    _, _, gv = vargrad64.mlpg_var_grad64(means, var, go, windows, lengths)
    s = (var * gv).reshape(4, T, nw, sd).sum(axis=(1, 2))
    mag = np.abs(var * gv).reshape(4, T, nw, sd).sum(axis=(1, 2))
    # (static-only / fully masked sets: y = mu and grad_var is rounding noise; the floor is eps |grad_out| |mu| per system)
    floor = 1e-14 * np.abs(go).sum(axis=1) * np.abs(means).max()
    assert (np.abs(s) <= 1e-12 * mag + floor).all(), (wname, s)


@pytest.mark.parametrize("wname", WNAMES)
def test_global_is_sum_of_frame_mode(wname):
    T, sd = 37, 4
    windows, means, var, vg, go, lengths = _case(wname, T, 4, sd, seed=3)
    _, gm_g, gv_g = vargrad64.mlpg_var_grad64(means, vg, go, windows, lengths)
    _, gm_f, gv_f = vargrad64.mlpg_var_grad64(means, np.broadcast_to(vg, means.shape).copy(), go, windows, lengths)
    assert gv_g.shape == (means.shape[2],)
    assert np.array_equal(gm_g, gm_f)
    assert np.abs(gv_g - gv_f.sum(axis=(0, 1))).max() <= 1e-13 * np.abs(gv_f).sum(axis=(0, 1)).max()


@pytest.mark.parametrize("wname", WNAMES)
def test_exact_zeros_and_junk_is_not_read(wname):
    """Masked entries and padding rows are exactly 0; NaN in the padding (means, var, grad_out) and in masked var entries
    changes nothing."""
    T, sd = 30, 3
    windows, means, var, vg, go, lengths = _case(wname, T, 4, sd, seed=5)
    ok = _live_unmasked(windows, lengths, T, sd)
    y0, gm0, gv0 = vargrad64.mlpg_var_grad64(means, var, go, windows, lengths)
    assert not gv0[~ok].any() and not gm0[~ok].any()
    pad = np.arange(T)[None, :] >= lengths[:, None]
    assert not y0[pad].any()
    m1, v1, g1 = means.copy(), var.copy(), go.copy()
    m1[pad] = np.nan
    g1[pad] = np.nan
    v1[~ok] = np.nan
    y1, gm1, gv1 = vargrad64.mlpg_var_grad64(m1, v1, g1, windows, lengths)
    assert np.array_equal(y0, y1) and np.array_equal(gm0, gm1) and np.array_equal(gv0, gv1)


_PRECISIONS = vargrad64.precisions


def _wrong_mask_at_tmax(var, windows, lengths, B, T, sd, dtype=np.float64):
    """A deliberately wrong precisions(): the edge mask taken at Tmax instead of each length."""
    tau = _PRECISIONS(var, windows, np.full(B, T), B, T, sd, dtype)
    live = np.arange(T)[:, None] < np.repeat(np.asarray(lengths), sd)[None, :]
    return np.where(live[None], tau, 0)


def _wrong_f64_reciprocal(var, windows, lengths, B, T, sd, dtype=np.float64):
    """A deliberately wrong precisions(): float64 reciprocals for float32 inputs."""
    return _PRECISIONS(np.asarray(var, dtype=np.float64), windows, lengths, B, T, sd, dtype)


@pytest.mark.parametrize("wrong", [_wrong_mask_at_tmax, _wrong_f64_reciprocal])
def test_wrong_variants_fail(monkeypatch, wrong):
    """The checks above catch a helper with the edge mask at Tmax, and one with float64 reciprocals of float32 inputs."""
    monkeypatch.setattr(vargrad64, "precisions", wrong)
    windows, means, var, vg, go, lengths = _case("std3", 20, 4, 2, seed=20, dt=np.float32)
    _, _, gv = vargrad64.mlpg_var_grad64(means, var, go, windows, lengths)
    ref = _dense_var_grad_real(means, var, go, windows, lengths, np.float32)
    caught = np.abs(gv - ref).max() > 1e-12 * np.abs(ref).max()
    assert caught, wrong.__name__
