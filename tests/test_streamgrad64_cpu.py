"""CPU checks (-m "not gpu") of tests/streamgrad64.py, the float64 anchor of the multi-stream backward tests: its value is the
oracle's, its gradients are the central differences of the oracle's forward pass through a scalar loss, and its pass-through,
padding and unused-column rules hold exactly.

The bar of the difference quotients: with h = 1e-5 the truncation error of a central difference is h^2 f''' / 6 ~ 1e-10 for these
O(1) problems and its rounding error eps |f| / h ~ 1e-10 (|f| = |sum y g| of tens); 1e-6 of the largest gradient entry leaves
three decades of room and is far below any error of the formula itself (a wrong sign, mask or stencil tap is O(1))."""
import numpy as np
import pytest

import streamgrad64 as SG
from cases import WINDOW_SETS

STD3, ASYM2, WIDE3 = WINDOW_SETS["std3"], WINDOW_SETS["asym2"], WINDOW_SETS["wide3"]


def _layout():
    """Four streams with gaps in the input and output rows and permuted output columns; ld_in 24, ld_out 12."""
    streams = [dict(in_col=1, out_col=7, static_dim=2, windows=STD3),         # columns 1..6
               dict(in_col=8, out_col=1, static_dim=1, windows=None),         # column 8
               dict(in_col=10, out_col=3, static_dim=3, windows=ASYM2),       # columns 10..15
               dict(in_col=17, out_col=10, static_dim=2, windows=WIDE3)]      # columns 17..22
    return streams, 24, 12


def _data(seed=0, B=3, T=9):
    streams, ld_in, ld_out = _layout()
    rng = np.random.RandomState(seed)
    M = rng.randn(B, T, ld_in)
    V = rng.rand(B, T, ld_in) + 0.5
    G = rng.randn(B, T, ld_out)
    lens = np.array([T, 5, 0], dtype=np.int32)[:B]
    return streams, M, V, G, lens


def _forward_oracle(M, V, streams, lens, ld_out):
    from oracle import mlpg as O
    B, T, _ = M.shape
    y = np.zeros((B, T, ld_out))
    live = (np.arange(T)[None, :] < lens[:, None])[:, :, None]
    for s in streams:
        sd, ic, oc = s["static_dim"], s["in_col"], s["out_col"]
        if not s["windows"]:
            y[:, :, oc:oc + sd] = np.where(live, M[:, :, ic:ic + sd], 0.0)
            continue
        cols = SG.stream_cols(s)
        v = V[cols] if V.ndim == 1 else np.ascontiguousarray(V[:, :, cols])
        ys, st, rc = O.mlpg_batch(np.ascontiguousarray(M[:, :, cols]), v, s["windows"], lens)
        assert rc == 0 and not st.any()
        y[:, :, oc:oc + sd] = ys
    return y


@pytest.mark.parametrize("mode", ["frame", "global"])
def test_value_and_gradients_against_the_oracle(mode):
    streams, M, V, G, lens = _data()
    ld_out = G.shape[2]
    var = V if mode == "frame" else V[0, 0].copy()
    y, gm, gv = SG.multi_stream_grad64(M, var, G, streams, lens)
    y_ref = _forward_oracle(M, var, streams, lens, ld_out)
    assert np.abs(y - y_ref).max() <= 1e-12 * np.abs(y_ref).max()
    if mode == "global":
        gv = gv.sum(axis=(0, 1))
    loss = lambda m, v: float((_forward_oracle(m, v, streams, lens, ld_out) * G).sum())  # noqa: E731
    h = 1e-5
    oi, _ = SG.owned(streams, M.shape[2], ld_out)
    rng = np.random.RandomState(1)
    for name, arr, grad in (("mean", M, gm), ("var", var, gv)):
        num = np.zeros_like(grad)
        idx = [i for i in np.ndindex(*arr.shape) if oi[i[-1]]]
        if len(idx) > 160:                                            # a sample; every owned column is in it
            pick = rng.permutation(len(idx))[:160]
            idx = [idx[k] for k in pick]
        for i in idx:
            ap, am = arr.copy(), arr.copy()
            ap[i] += h
            am[i] -= h
            num[i] = ((loss(ap, var) - loss(am, var)) if name == "mean" else (loss(M, ap) - loss(M, am))) / (2 * h)
        sel = np.zeros(grad.shape, dtype=bool)
        for i in idx:
            sel[i] = True
        err = np.abs(num - grad)[sel].max()
        assert err <= 1e-6 * np.abs(grad).max(), (mode, name, err, np.abs(grad).max())
        assert np.abs(grad[sel]).max() > 0


def test_pass_through_padding_and_unused_columns():
    streams, M, V, G, lens = _data(seed=2)
    B, T, ld_in = M.shape
    ld_out = G.shape[2]
    oi, oo = SG.owned(streams, ld_in, ld_out)
    pad = np.arange(T)[None, :] >= lens[:, None]
    # whatever the padding rows, the unused columns and a pass-through stream's variances hold is never read
    Mx, Vx, Gx = M.copy(), V.copy(), G.copy()
    Mx[pad] = np.nan
    Vx[pad] = np.nan
    Gx[pad] = np.nan
    Mx[:, :, ~oi] = np.nan
    Vx[:, :, ~oi] = np.nan
    Gx[:, :, ~oo] = np.nan
    Vx[:, :, 8] = -1.0
    a = SG.multi_stream_grad64(M, V, G, streams, lens)
    b = SG.multi_stream_grad64(Mx, Vx, Gx, streams, lens)
    for x, z in zip(a, b):
        assert np.array_equal(x, z)
    y, gm, gv = a
    assert not y[pad].any() and not gm[pad].any() and not gv[pad].any()
    assert not y[:, :, ~oo].any() and not gm[:, :, ~oi].any() and not gv[:, :, ~oi].any()
    live = ~pad
    assert np.array_equal(y[:, :, 1][live], M[:, :, 8][live]) and np.array_equal(gm[:, :, 8][live], G[:, :, 1][live])
    assert not gv[:, :, 8].any()
    # unit variances: no variance gradient, the means' one as with variances of 1
    y1, gm1, gv1 = SG.multi_stream_grad64(M, None, G, streams, lens)
    y2, gm2, _ = SG.multi_stream_grad64(M, np.ones_like(V), G, streams, lens)
    assert gv1 is None and np.array_equal(y1, y2) and np.array_equal(gm1, gm2)


def test_scale_invariant_on_a_merlin_layout():
    """180 | 3 | 1 | 15 with ragged lengths down to 0: sum var * grad_var = 0 per dynamic system."""
    rng = np.random.RandomState(3)
    sizes, dyn = [180, 3, 1, 15], [True, True, False, True]
    streams, col, oc = [], 0, 0
    for size, d in zip(sizes, dyn):
        sd = size // 3 if d else size
        streams.append(dict(in_col=col, out_col=oc, static_dim=sd, windows=STD3 if d else None))
        col += size
        oc += sd
    B, T = 4, 40
    M, V, G = rng.randn(B, T, col), rng.rand(B, T, col) + 0.1, rng.randn(B, T, oc)
    lens = np.array([T, 23, 1, 0])
    _, gm, gv = SG.multi_stream_grad64(M, V, G, streams, lens)
    for s in streams:
        if not s["windows"]:
            continue
        cols = SG.stream_cols(s)
        sd = s["static_dim"]
        prod = (V[:, :, cols] * gv[:, :, cols]).reshape(B, T, 3, sd)
        assert (np.abs(prod.sum(axis=(1, 2))) <= 1e-12 * np.maximum(np.abs(prod).sum(axis=(1, 2)), 1e-300) + 1e-14).all()
