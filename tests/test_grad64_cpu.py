"""oracle/grad64.py (the float64 MLPG gradient every backward route is judged by: tests/test_backward_routes_gpu.py)
against three things it does not share code with: the oracle's dense restatement of the reference's mlpg_grad, the
transposed Jacobian of the C oracle's forward pass, and the reference's own float32 gradients.  No GPU needed."""
import os
import time

import numpy as np
import pytest

from cases import WINDOW_SETS, rand_case
from oracle import mlpg as O
from oracle.grad64 import _band, banded_solve, mlpg_grad64, precisions

HERE = os.path.dirname(os.path.abspath(__file__))
F32_ULP = 2.0 ** -24          # unit roundoff of float32: O.mlpg_grad returns float32, as the reference


def _var_arg(mode, v):
    """(B, T, D) per-frame variances -> what mlpg_grad64 takes for `mode`."""
    return {"frame": v, "global": v[0, 0].copy(), "unit": None}[mode]


def _dense_var(mode, v, T):
    """What the reference's mlpg_grad is handed for `mode` on one utterance: (T, D)."""
    D = v.shape[-1]
    if mode == "frame":
        return v[0]
    if mode == "global":
        return np.ascontiguousarray(np.broadcast_to(v[0, 0], (T, D)))
    return np.ones((T, D), dtype=v.dtype)


@pytest.mark.parametrize("wname", sorted(WINDOW_SETS))
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_equals_dense_mlpg_grad(wname, dt):
    """Every window set (static and the [-0:] quirk set included), T = 1..40, per-frame / global / unit variances: equal to the
    dense restatement within the float32 rounding of its result."""
    windows = WINDOW_SETS[wname]
    nw, sd = len(windows), 3
    for T in range(1, 41):
        rng = np.random.RandomState(1000 * T + nw)
        v = (rng.rand(1, T, nw * sd) + 0.1).astype(dt)
        go = rng.randn(1, T, sd).astype(dt)
        for mode in ("frame", "global", "unit"):
            g = mlpg_grad64(_var_arg(mode, v), go, windows)[0]
            r = O.mlpg_grad(np.zeros((T, nw * sd)), _dense_var(mode, v, T), windows, go[0])
            assert g.dtype == np.float64 and g.shape == r.shape
            scale = np.abs(g).max()
            assert (np.abs(g - r) <= F32_ULP * np.abs(g) + 1e-12 * scale).all(), (wname, T, mode, np.abs(g - r).max() / scale)


def _jacobian_T(V, windows, lengths, go):
    """J^T go for the C oracle's batched forward pass, one one-hot mean per (t, k): (B, T, D) float64."""
    B, T, sd = go.shape
    D = len(windows) * sd
    out = np.zeros((B, T, D))
    eye = np.eye(T * D).reshape(T * D, T, D)
    for b in range(B):
        varb = V if V.ndim == 1 else np.ascontiguousarray(np.broadcast_to(V[b], (T * D, T, D)))
        y, status, rc = O.mlpg_batch(eye, varb, windows, np.full(T * D, lengths[b], dtype=np.int32))
        assert rc == 0
        out[b] = np.einsum("ntd,td->n", y, go[b]).reshape(T, D)
    return out


@pytest.mark.parametrize("wname", ["wide3", "std3", "asym2", "std2", "zero2", "static"])
@pytest.mark.parametrize("mode", ["frame", "global", "unit"])
def test_equals_transposed_jacobian_of_the_forward_pass_ragged(wname, mode):
    """Ragged lengths including 1 and 0: the per-utterance edge mask and the truncation at each length, to 1e-13."""
    windows = WINDOW_SETS[wname]
    nw, sd, T = len(windows), 2, 23
    D = nw * sd
    rng = np.random.RandomState(7 + nw)
    V = rng.rand(5, T, D) + 0.1
    go = rng.randn(5, T, sd)
    lengths = np.array([23, 22, 11, 1, 0])
    var = _var_arg(mode, V)
    J = _jacobian_T(np.ones(D) if var is None else var, windows, lengths, go)
    g = mlpg_grad64(var, go, windows, lengths)
    scale = np.abs(J).max()
    assert np.abs(g - J).max() <= 1e-13 * scale, (wname, mode, np.abs(g - J).max() / scale)
    for b, L in enumerate(lengths):
        assert (g[b, L:] == 0).all()
    # float32 inputs: the reciprocal is taken in float32 and widened (the float64 forward pass is handed the exact
    # float64 reciprocal of that float32 precision, so the two must agree to float64 rounding, not to float32's)
    if mode != "unit":
        v32 = var.astype(np.float32)
        v64 = 1.0 / (np.float32(1) / v32).astype(np.float64)
        g32 = mlpg_grad64(v32, go.astype(np.float32), windows, lengths)
        J32 = _jacobian_T(v64, windows, lengths, go.astype(np.float32).astype(np.float64))
        assert np.abs(g32 - J32).max() <= 1e-13 * np.abs(J32).max(), (wname, mode)


@pytest.mark.parametrize("key", ["std3-f32-T300", "std3-f64-T300", "std3-f32-T1000", "std3-f64-T1000",
                                 "std3-f32-T2000", "std3-f64-T2000", "std2-f64-T700", "asym2-f64-T700"])
def test_equals_reference_goldens(key):
    """The reference's own (float32) mlpg_grad outputs at T = 300 / 700 / 1000 / 2000 (tests/golden/make_golden2.py)."""
    g2 = np.load(os.path.join(HERE, "golden", "mlpg_golden2.npz"))
    wname, dt, T = key.split("-")
    T = int(T[1:])
    sd = 2 if wname == "std3" else 3
    _, v, _ = rand_case(wname, dt, T, sd, salt=11)
    go = np.random.RandomState(500 + T).randn(T, sd).astype(v.dtype)
    ref = g2["grad2/%s/g" % key]
    g = mlpg_grad64(v[None], go[None], WINDOW_SETS[wname])[0]
    assert np.abs(g - ref).max() <= 3e-6 * np.abs(ref).max(), key


def test_padding_is_never_read():
    """NaN / 0 / -1 in the variances' padding and NaN in grad_out's: live rows bit-identical, padding rows exactly 0."""
    windows = WINDOW_SETS["std3"]
    rng = np.random.RandomState(3)
    B, T, sd = 4, 30, 3
    V = rng.rand(B, T, 3 * sd) + 0.1
    go = rng.randn(B, T, sd)
    lengths = np.array([30, 17, 1, 0])
    clean = mlpg_grad64(V, go, windows, lengths)
    Vd, god = V.copy(), go.copy()
    for b, L in enumerate(lengths):
        Vd[b, L:] = np.array([np.nan, 0.0, -1.0])[np.arange(T - L) % 3][:, None]
        god[b, L:] = np.nan
    dirty = mlpg_grad64(Vd, god, windows, lengths)
    assert np.array_equal(clean, dirty)
    for b, L in enumerate(lengths):
        assert (dirty[b, L:] == 0).all()


def _dense_P(Pb):
    q, T = Pb.shape[0] - 1, Pb.shape[1]
    P = np.zeros((Pb.shape[2], T, T), dtype=Pb.dtype)
    for m in range(q + 1):
        i = np.arange(T - m)
        P[:, i, i + m] = Pb[m, :T - m].T
        P[:, i + m, i] = Pb[m, :T - m].T
    return P


@pytest.mark.parametrize("wname", ["std3", "wide3", "asym2", "static"])
def test_banded_solve_equals_dense_solve(wname):
    windows = WINDOW_SETS[wname]
    q = max(l + u for l, u, _ in windows)
    rng = np.random.RandomState(11)
    for T in (1, 2, 5, 37, 200):
        B, sd = 3, 4
        V = rng.rand(B, T, len(windows) * sd) + 0.1
        lengths = np.array([T, max(T // 2, 1), 1])
        Ls = np.repeat(lengths, sd)[None, :]
        tau = precisions(V, windows, lengths, B, T, sd)
        Pb = _band(tau, [(l, u, np.asarray(c, dtype=np.float64)) for l, u, c in windows], Ls, T, q, np.float64)
        rhs = rng.randn(T, B * sd)
        z = banded_solve(Pb, rhs)
        zd = np.linalg.solve(_dense_P(Pb), rhs.T[:, :, None])[:, :, 0].T
        assert np.abs(z - zd).max() <= 1e-13 * np.abs(zd).max(), (wname, T)
        # the extended-precision variant agrees with the float64 one
        zl = banded_solve(Pb.astype(np.longdouble), rhs.astype(np.longdouble))
        assert np.abs(z - zl).max() <= 1e-13 * np.abs(zd).max(), (wname, T)


def test_long_utterances_are_cheap():
    """O(T): T = 4100 with 60 systems well under a second."""
    rng = np.random.RandomState(5)
    V = rng.rand(3, 4100, 60) + 0.1
    go = rng.randn(3, 4100, 20)
    t0 = time.perf_counter()
    g = mlpg_grad64(V, go, WINDOW_SETS["std3"])
    assert time.perf_counter() - t0 < 1.0
    assert np.isfinite(g).all()
