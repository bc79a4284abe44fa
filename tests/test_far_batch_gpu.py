"""GPU tests (-m gpu): the dense entries that take `lengths`, on batches of thousands of mostly empty utterances (tests/far.py), so
that the few live utterances lie on both sides of 2^31 bytes and 2^32 bytes from the array's first element.  float64, D = 180
(three windows, 60 static dims), Tmax = 1000: an utterance of the input is 1 440 000 bytes, utterance 1491 straddles 2^31 bytes
(1491 * 1.44e6 = 2 147 040 000) and utterance 2982 straddles 2^32 bytes (4 294 080 000).  lengths is 0 everywhere except the
first and the last utterance, the three around each boundary and one in the middle of each stretch; the live lengths are mixed
(Tmax, 1, 63, 64, 65, ...), the padding of a live utterance holds NaN and the dead utterances keep the fill byte 0xA5.  An array
of 60 columns crosses the boundaries three times later: where an entry has one, further cases are sized for it -- more
utterances, or the one-window set, whose input and output have the same width -- as far as 12 GiB of device memory go.

Inputs must keep their bits (FarParent.untouched()).  Every output is written whole: exact zeros in every dead utterance and in
the padding of the live ones, checked on the device over the whole array (untouched(rest=0)), guards included.  The live utterances
are compared with the reference and the bound of the entry's own GPU test, computed for those utterances alone.  The last
test prints which boundaries each array argument crossed and fails unless every one crossed 2^31 bytes and 2^32 bytes; the
arguments that 12 GiB hold to 2^31 bytes alone are named there, with the sizes that rule 2^32 out."""
import collections
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

import far
import modspec_batch64 as R64
from cases import WINDOW_SETS
from far import FarParent

pytestmark = pytest.mark.gpu

F64 = np.float64
T, D, SD = 1000, 180, 60
WINDOWS, ONE_WINDOW = WINDOW_SETS["std3"], WINDOW_SETS["static"]
BYTES = ("2^31 bytes", "2^32 bytes")
COVER = collections.defaultdict(set)
LIVE_LENGTHS = [T, 1, 63, 64, 65, T - 1, 129, 2, T, 257, 3]


def far_test(fn):
    """Peak device memory of the test stays under far.MEM_CAP; whatever it allocated is handed back at its end."""
    @functools.wraps(fn)
    def run(*a, **kw):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        try:
            fn(*a, **kw)
            peak = torch.cuda.max_memory_allocated()
        finally:
            gc.collect()
            torch.cuda.empty_cache()
        assert peak <= far.MEM_CAP, "peak device memory %.2f GiB" % (peak / 2.0 ** 30)
    return run


def live_utterances(B, *utt_bytes):
    """(indices, lengths) of the live utterances of a batch whose arrays have utterances of utt_bytes bytes: the first, the
    last, for each array the one that holds each boundary with its two neighbours, and one in the middle of each stretch
    between them."""
    marks = sorted({0, B - 1} | {b + k for ub in utt_bytes for at in (1 << 31, 1 << 32) for b in [at // ub] for k in (-1, 0, 1)
                                 if 0 <= b + k < B})
    mids = {(a + b) // 2 for a, b in zip(marks[:-1], marks[1:]) if b - a > 4}
    idx = np.array(sorted(set(marks) | mids), dtype=np.int64)
    lens = np.array((LIVE_LENGTHS * 4)[:len(idx)], dtype=np.int32)
    return idx, lens


def batch_for(*row_bytes):
    """The smallest B (plus two) whose last utterance lies beyond the boundary named for each array: (bytes per utterance, boundary)."""
    return max(at // ub for ub, at in row_bytes) + 2


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def lengths_on_device(B, idx, lens):
    L = torch.zeros(B, dtype=torch.int32, device="cuda")
    L[torch.from_numpy(idx).cuda()] = torch.from_numpy(lens).cuda()
    return L


def parent(B, rows, cols, dtype=F64, other_bytes=0, fill_byte=0xA5):
    nbytes = B * rows * cols * np.dtype(dtype).itemsize
    return FarParent((B, rows, cols), dtype, low_guard_bytes=far.low_guard_for(nbytes, other_bytes), fill_byte=fill_byte)


def put_live(p, idx, X):
    """Utterance idx[i] of the parent holds X[i] whole (its padding rows too: NaN)."""
    for i, b in enumerate(idx):
        p.place(int(b), p.Tmax, 0, X[i])


def expect_live(p, idx):
    for b in idx:
        p.expect_written(int(b), p.Tmax, 0, p.ld)


def get_live(p, idx):
    return np.stack([p.read(int(b), p.Tmax, 0, p.ld) for b in idx])


def note(entry, arg, p):
    COVER[(entry, arg)] |= p.crossed()


def nan_pad(X, lens):
    X = X.copy()
    for i, n in enumerate(lens):
        X[i, n:] = np.nan
    return X


def lib_call():
    from nnmnkwii_amd import _hip
    d = torch.device("cuda", torch.cuda.current_device())
    return _hip.lib(), d.index, _hip._stream(d)


def win_args(windows=WINDOWS):
    """(the packed arrays, to be kept alive; the four window arguments of a C entry)."""
    from nnmnkwii_amd import _hip
    wl, wu, wc = _hip.pack_windows(windows)
    return (wl, wu, wc), (len(wl), wl.ctypes.data, wu.ctypes.data, wc.ctypes.data)


def counts(n=44):
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return [L.mlpg_hip_launch_count(k) for k in range(n)]


def moved(c0):
    return {k: b - a for k, (a, b) in enumerate(zip(c0, counts())) if a != b}


def all_clean(*checks):
    for name, fails in checks:
        assert fails == [], (name, fails)


# ---------------------------------------------------------------------------------------------------- forward and backward

FAMILIES = {"auto": (0, None), "generic": (1, 0), "wave": (2, 1), "strip": (3, 2), "const": (5, 4), "chunk": (6, 6)}
UTT_IN, UTT_OUT = T * D * 8, T * SD * 8
B_IN = batch_for((UTT_IN, 1 << 32))                 # 2984: a (B, T, 180) array crosses 2^32 bytes, a (B, T, 60) one nothing
B_IN_HALF = batch_for((UTT_IN, 1 << 31))            # 1493: a (B, T, 180) array crosses 2^31 bytes
B_OUT = batch_for((UTT_OUT, 1 << 31))               # 4475: a (B, T, 60) array crosses 2^31 bytes
B_OUT_FULL = batch_for((UTT_OUT, 1 << 32))          # 8949: a (B, T, 60) array crosses 2^32 bytes
# case -> (windows, columns in, B): the families the shape admits are those of FAMILIES that take the window set
SHAPES = {"wide_past_4GiB": (WINDOWS, D, B_IN), "narrow_past_2GiB": (WINDOWS, D, B_OUT), "one_window_past_4GiB": (ONE_WINDOW, SD, B_OUT_FULL)}


def admitted(case):
    return [f for f in FAMILIES if SHAPES[case][0] is WINDOWS or f not in ("const", "chunk")]   # (these two need a dynamic window)


SOLVE_CASES = [(case, fam) for case in SHAPES for fam in admitted(case)]


def test_the_geometry_is_the_one_worked_out_by_hand():
    assert (B_IN, B_IN_HALF, B_OUT, B_OUT_FULL) == (2984, 1493, 4475, 8949)
    assert 1491 * UTT_IN < 2 ** 31 < 1492 * UTT_IN and 2982 * UTT_IN < 2 ** 32 < 2983 * UTT_IN
    idx, lens = live_utterances(B_IN, UTT_IN)
    assert idx.tolist() == [0, 745, 1490, 1491, 1492, 2236, 2981, 2982, 2983] and lens.tolist() == [1000, 1, 63, 64, 65, 999, 129, 2, 1000]


@pytest.mark.parametrize("case,fam", SOLVE_CASES, ids=["%s-%s" % c for c in SOLVE_CASES])
@far_test
def test_forward(case, fam):
    """Global variances; every family the shape admits (60 static dims, windows of extent <= 1, 1000 frames) and AUTO."""
    from oracle import mlpg as O
    import test_stream_routes_gpu as R
    windows, din, B = SHAPES[case]
    L, di, stream = lib_call()
    keep, win = win_args(windows)
    algo, kind = FAMILIES[fam]
    idx, lens = live_utterances(B, T * din * 8, UTT_OUT)
    rng = np.random.RandomState(B % 1000 + algo)
    M = rng.randn(len(idx), T, din)
    V = rng.rand(din) + 0.1
    mean = parent(B, T, din, other_bytes=B * UTT_OUT)
    out = parent(B, T, SD, other_bytes=mean.nbytes + mean.lo)
    put_live(mean, idx, nan_pad(M, lens))
    expect_live(out, idx)
    Ld, Vd = lengths_on_device(B, idx, lens), dev(V)
    status = torch.full((B * SD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0 = counts()
    rc = L.mlpg_hip_forward(di, stream, 1, algo, mean.ptr(), Vd.data_ptr(), 1, Ld.data_ptr(), B, T, din, *win, out.ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    m = moved(c0)
    assert sum(m.values()) == 1 and (kind is None or m == {kind: 1}), (fam, m)
    assert not bool(status.any()), "a status cell is not zero"
    got = get_live(out, idx)
    ref, st, orc = O.mlpg_batch(M, V, windows, lens)
    assert orc == 0
    e, scale = np.abs(got - ref).max(axis=(1, 2)), np.abs(ref).max(axis=(1, 2))
    assert (e <= R.TOL[F64] * scale).all(), (fam, (e / scale).tolist())
    assert all(not got[i, n:].any() for i, n in enumerate(lens))
    note("forward", "mean", mean)
    note("forward", "out", out)
    all_clean(("mean", mean.untouched()), ("out", out.untouched(rest=0)))
    mean.free()
    out.free()


@pytest.mark.parametrize("case,fam", [c for c in SOLVE_CASES if c[0] != "wide_past_4GiB"],
                         ids=["%s-%s" % c for c in SOLVE_CASES if c[0] != "wide_past_4GiB"])
@far_test
def test_backward(case, fam):
    """Unit variances.  grad_out (B, T, 60) past 2^31 bytes with grad_mean (B, T, 180) past 2^32; with one window both are
    (B, T, 60) and past 2^32."""
    from oracle.grad64 import mlpg_grad64
    from test_backward_routes_gpu import _check_grad
    windows, dg, B = SHAPES[case]
    L, di, stream = lib_call()
    keep, win = win_args(windows)
    algo, kind = FAMILIES[fam]
    idx, lens = live_utterances(B, UTT_OUT, T * dg * 8)
    rng = np.random.RandomState(algo)
    GO = rng.randn(len(idx), T, SD)
    go = parent(B, T, SD, other_bytes=B * T * dg * 8)
    gm = parent(B, T, dg, other_bytes=go.nbytes + go.lo)
    put_live(go, idx, nan_pad(GO, lens))
    expect_live(gm, idx)
    Ld = lengths_on_device(B, idx, lens)
    status = torch.full((B * SD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0 = counts()
    rc = L.mlpg_hip_backward(di, stream, 1, 1, algo, None, 2, go.ptr(), Ld.data_ptr(), B, T, dg, *win, gm.ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    m = moved(c0)
    assert sum(m.values()) == 1 and (kind is None or m == {kind: 1}), (fam, m)
    assert not bool(status.any())
    _check_grad(get_live(gm, idx), mlpg_grad64(None, GO, windows, lens), lens, 1e-10, fam)
    note("backward", "grad_out", go)
    note("backward", "grad_mean", gm)
    assert set(BYTES) <= gm.crossed() and "2^31 bytes" in go.crossed()
    all_clean(("grad_out", go.untouched()), ("grad_mean", gm.untouched(rest=0)))
    go.free()
    gm.free()


@pytest.mark.parametrize("mode", ["frame", "global", "one_window_global"])
@far_test
def test_backward_var(mode):
    """Six arrays of the batch's size: 1493 utterances put the four (B, T, 180) ones past 2^31 bytes in 10 GB.  With one window and
    global variances the five arrays are (B, T, 60): 4475 utterances put y and grad_out past 2^31 bytes too."""
    import vargrad64
    from oracle import mlpg as O
    from test_backward_routes_gpu import _check_grad
    from test_var_grad_gpu import _check_var_grad, _masked, _terms
    L, di, stream = lib_call()
    windows, d, B = (ONE_WINDOW, SD, B_OUT) if mode == "one_window_global" else (WINDOWS, D, B_IN_HALF)
    keep, win = win_args(windows)
    idx, lens = live_utterances(B, T * d * 8)
    n = len(idx)
    rng = np.random.RandomState(len(mode))
    M, GO = rng.randn(n, T, d), rng.randn(n, T, SD)
    V = rng.rand(n, T, d) + 0.1 if mode == "frame" else rng.rand(d) + 0.1
    Y, st, orc = O.mlpg_batch(M, V, windows, lens)
    assert orc == 0 and not st.any()
    names = ["mean", "y", "grad_out", "grad_mean", "grad_var"] + (["var"] if mode == "frame" else [])
    cols = dict(mean=d, var=d, y=SD, grad_out=SD, grad_mean=d, grad_var=d)
    assert sum(B * T * cols[k] * 8 for k in names) + (1 << 30) <= far.MEM_CAP
    P = {k: FarParent((B, T, cols[k]), F64) for k in names}                       # 4096-byte guards: six arrays under the cap
    put_live(P["mean"], idx, nan_pad(M, lens))
    put_live(P["y"], idx, nan_pad(Y, lens))
    put_live(P["grad_out"], idx, nan_pad(GO, lens))
    if mode == "frame":
        put_live(P["var"], idx, nan_pad(V, lens))
    expect_live(P["grad_mean"], idx)
    expect_live(P["grad_var"], idx)
    Vd = None if mode == "frame" else dev(V)
    Ld = lengths_on_device(B, idx, lens)
    status = torch.full((B * SD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0 = counts()
    rc = L.mlpg_hip_backward_var(di, stream, 1, 0, P["mean"].ptr(), P["var"].ptr() if mode == "frame" else Vd.data_ptr(),
                                 0 if mode == "frame" else 1, P["y"].ptr(), P["grad_out"].ptr(), Ld.data_ptr(), B, T, d, *win,
                                 P["grad_mean"].ptr(), P["grad_var"].ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    m = moved(c0)
    assert m.pop(13, 0) == 1 and sum(m.values()) == 1, m
    assert not bool(status.any()), "the status of a dead utterance (or of a live one) is not zero"
    gm, gv = get_live(P["grad_mean"], idx), get_live(P["grad_var"], idx)
    live = np.arange(T)[None, :, None] < lens[:, None, None]
    Mz = np.where(live, M, 0.0)
    # (global variances: entry (b, t, c) of grad_var is frame t's share of the vector's gradient -- what per-frame variances
    # that repeat the vector give)
    Vs = np.where(live, V, 1.0) if mode == "frame" else np.broadcast_to(V, M.shape).copy()
    _, ref_m, ref_v = vargrad64.mlpg_var_grad64(Mz, Vs, np.where(live, GO, 0.0), windows, lens)
    _check_grad(gm, ref_m, lens, 1e-10, mode)
    _check_var_grad(gv, ref_v, lens, _masked(windows, lens, T, SD), 1e-10, mode, _terms(Mz, Vs, Y, ref_m, windows))
    for k in names:
        note("backward_var", k, P[k])
        fails = P[k].untouched(rest=0 if k in ("grad_mean", "grad_var") else None)
        assert fails == [], (k, fails)
        P[k].free()


@pytest.mark.parametrize("case", ["out_past_4GiB", "one_window_past_4GiB"])
@far_test
def test_delta_features(case):
    """x (B, T, 60) -> out (B, T, 180) with the three standard windows: out past 2^32 bytes; x (B, T, 180) -> out (B, T, 180)
    with the delta window alone: both past 2^32 bytes."""
    from oracle import mlpg as O
    L, di, stream = lib_call()
    windows = WINDOWS if case == "out_past_4GiB" else WINDOWS[1:2]
    dx = SD if case == "out_past_4GiB" else D
    B = B_IN
    keep, win = win_args(windows)
    idx, lens = live_utterances(B, UTT_IN)
    rng = np.random.RandomState(7)
    X = rng.randn(len(idx), T, dx)
    x = parent(B, T, dx, other_bytes=B * UTT_IN)
    out = parent(B, T, dx * len(windows), other_bytes=x.nbytes + x.lo)
    put_live(x, idx, nan_pad(X, lens))
    expect_live(out, idx)
    Ld = lengths_on_device(B, idx, lens)
    rc = L.mlpg_hip_delta_features(di, stream, 1, x.ptr(), Ld.data_ptr(), B, T, dx, *win, out.ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    got = get_live(out, idx)
    for i, n in enumerate(lens):
        assert not got[i, n:].any()
        # (x = 0 outside [0, len): two rows of zeros behind the utterance, so that the oracle's "same" correlation also takes
        # the utterances shorter than the window)
        ref = O.delta_features(np.vstack([X[i, :n], np.zeros((2, dx))]), windows)[:n]
        np.testing.assert_allclose(got[i, :n], ref, rtol=1e-12, atol=1e-14)                                   # tests/test_util_gpu.py
    note("delta_features", "x", x)
    note("delta_features", "out", out)
    all_clean(("x", x.untouched()), ("out", out.untouched(rest=0)))
    x.free()
    out.free()


# ---------------------------------------------------------------------------------------------------- gv ascent, the fused step

GV_SD, GV_D = 4, 12
# case -> (B, y_out is y_in, window set)
GV_CASES = {"mean_past_4GiB": (batch_for((T * GV_D * 8, 1 << 32)), False, "std3"),
            "y_past_2GiB": (batch_for((T * GV_SD * 8, 1 << 31)), True, "std3"),
            "one_window_y_past_4GiB": (batch_for((T * GV_SD * 8, 1 << 32)), True, "static")}


@pytest.mark.parametrize("case", list(GV_CASES))
@far_test
def test_gv_ascent(case):
    """Four static dims, so that tens of thousands of utterances fit: mean (B, T, 12) past 2^32 bytes with y_in and y_out apart,
    y (B, T, 4) past 2^31 bytes in place, and with the one-window set mean and y, both (B, T, 4), past 2^32 bytes in place (134219
    utterances, 8.6 GB).  Five iterations; the report and the status of a dead utterance are zero."""
    import gvmlpg_cases as GC
    import test_gvmlpg_gpu as TG
    L, di, stream = lib_call()
    B, in_place, wname = GV_CASES[case]
    gv_d = GV_SD * len(GC.WINDOWS[wname])
    idx, lens = live_utterances(B, T * gv_d * 8, T * GV_SD * 8)
    n = len(idx)
    c = GC.make_case(5, n, T, GV_SD, wname, GC.GV.VAR_GLOBAL, F64, lengths=lens)
    keep, win = win_args(c["windows"])
    mean = parent(B, T, gv_d, other_bytes=2 * B * T * GV_SD * 8)
    y_in = parent(B, T, GV_SD, other_bytes=mean.nbytes + mean.lo + B * T * GV_SD * 8)
    y_out = y_in if in_place else parent(B, T, GV_SD, other_bytes=mean.nbytes + mean.lo + y_in.nbytes + y_in.lo)
    put_live(mean, idx, nan_pad(c["mean"], lens))
    put_live(y_in, idx, nan_pad(c["y_in"], lens))
    expect_live(y_out, idx)
    Ld, Vd, gm, gp = lengths_on_device(B, idx, lens), dev(c["var"]), dev(c["gv_mean"]), dev(c["gv_prec"])
    rep = torch.full((B, GV_SD, 4), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((B, GV_SD), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    c0 = counts()
    rc = L.mlpg_hip_gv_ascent(di, stream, 1, mean.ptr(), Vd.data_ptr(), 1, Ld.data_ptr(), B, T, gv_d, *win, y_in.ptr(), y_out.ptr(),
                              gm.data_ptr(), gp.data_ptr(), 1.0, 5, -1.0, 1, rep.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {35: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    sel = torch.from_numpy(idx).cuda()
    TG.check_against_model(c, get_live(y_out, idx), rep[sel].cpu().numpy(), st[sel].cpu().numpy(), n_iter=5)
    rep[sel], st[sel] = 0.0, 0
    assert not bool(rep.any()) and not bool(st.any()), "the report or the status of a dead utterance is not zero"
    note("gv_ascent", "mean", mean)
    note("gv_ascent", "y_in", y_in)
    note("gv_ascent", "y_out", y_out)
    all_clean(("mean", mean.untouched()), ("y_out", y_out.untouched(rest=0)))
    if not in_place:
        assert y_in.untouched() == []
    for p in (mean, y_in, y_out):
        p.free()


@pytest.mark.parametrize("case", ["wide_past_4GiB", "one_window_past_2GiB"])
@far_test
def test_unit_mse_step(case):
    """mean and grad_mean (B, T, 180) past 2^32 bytes, y_out NULL; with one window mean, target, y_out and grad_mean are all
    (B, T, 60) and past 2^31 bytes (four such arrays past 2^32 would be 17 GB)."""
    from oracle.mse64 import unit_mse_step64
    from test_mse_routes_gpu import TOL, _check_rows
    L, di, stream = lib_call()
    windows, dm, B, with_y = (WINDOWS, D, B_IN, False) if case == "wide_past_4GiB" else (ONE_WINDOW, SD, B_OUT, True)
    keep, win = win_args(windows)
    idx, lens = live_utterances(B, T * dm * 8, UTT_OUT)
    n = len(idx)
    rng = np.random.RandomState(13)
    M, Tg = rng.randn(n, T, dm), rng.randn(n, T, SD)
    mean = FarParent((B, T, dm), F64)
    target = FarParent((B, T, SD), F64)
    grad = FarParent((B, T, dm), F64)
    y = FarParent((B, T, SD), F64) if with_y else None
    put_live(mean, idx, nan_pad(M, lens))
    put_live(target, idx, nan_pad(Tg, lens))
    expect_live(grad, idx)
    if with_y:
        expect_live(y, idx)
    Ld = lengths_on_device(B, idx, lens)
    ws_bytes = int(L.mlpg_hip_unit_mse_workspace_bytes(B, dm, len(windows)))
    ws = torch.zeros(ws_bytes + 128, dtype=torch.uint8, device="cuda")
    ws_ptr = -(-ws.data_ptr() // 128) * 128
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((B * SD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    n_elems = float(n * T * SD)
    c0 = counts()
    rc = L.mlpg_hip_unit_mse_step(di, stream, 1, mean.ptr(), target.ptr(), Ld.data_ptr(), B, T, dm, *win, n_elems,
                                  y.ptr() if with_y else None, grad.ptr(), loss.data_ptr(), status.data_ptr(), ws_ptr, ws_bytes)
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {5: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    assert not bool(status.any())
    y_ref, loss_ref, grad_ref, st_ref = unit_mse_step64(M, Tg, windows, lens, n_elems)
    tol_y, tol_g, tol_l = TOL[(1, 1)]
    ok = st_ref == 0
    _check_rows(get_live(grad, idx), grad_ref, lens, ok, tol_g, case + " grad")
    if with_y:
        _check_rows(get_live(y, idx), y_ref, lens, ok, tol_y, case + " y")
    assert abs(float(loss[0]) - loss_ref) <= tol_l * loss_ref, (float(loss[0]), loss_ref)
    for name, p, rest in (("mean", mean, None), ("target", target, None), ("grad_mean", grad, 0), ("y_out", y, 0)):
        if p is not None:
            note("unit_mse_step", name, p)
            fails = p.untouched(rest=rest)
            assert fails == [], (name, fails)
            p.free()


# ---------------------------------------------------------------------------------------------------- modulation spectrum

N_FFT = 1024
NB = N_FFT // 2 + 1
UTT_MS = NB * D * 8
MS_SHAPES = {"x_past_4GiB": (B_IN, T), "ms_past_4GiB": (batch_for((UTT_MS, 1 << 32)), 256)}


def _close(a, b, rel, what):
    err = np.abs(np.asarray(a, dtype=F64) - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= rel, (what, err)


@pytest.mark.parametrize("case", list(MS_SHAPES))
@pytest.mark.parametrize("ortho,norm", [(0, None), (1, "ortho")])
@far_test
def test_modspec_batch_backward_and_loss_step(ortho, norm, case):
    """x and grad_x (B, 1000, 180) past 2^32 bytes with ms, grad_ms and target_ms (B, 513, 180) past 2^31; then 256 frames per
    utterance and more utterances, so that the spectra are the arrays past 2^32.  The spectrum, its gradient and the fused loss
    step, one after the other on the same input."""
    from test_modspec_batch_gpu import TOL
    tol = TOL[torch.float64]
    L, di, stream = lib_call()
    B, Tm = MS_SHAPES[case]
    idx, lens = live_utterances(B, UTT_MS, Tm * D * 8)
    lens = np.minimum(lens, Tm).astype(np.int32)
    n = len(idx)
    rng = np.random.RandomState(11 + ortho)
    X = R64.make_batch(rng, n, Tm, D, lens)                                         # NaN from each length on
    Gm = rng.rand(n, NB, D)
    Tg = R64.modspec(R64.make_batch(rng, n, Tm, D, lens, pad=0.0), N_FFT, None, lens) + 0.01
    Ld = lengths_on_device(B, idx, lens)
    sizes = B * Tm * D * 8, B * UTT_MS
    x = parent(B, Tm, D, other_bytes=sizes[0] + sizes[1])
    put_live(x, idx, X)
    # the spectrum; a dead utterance's is that of no frames: zeros
    ms = parent(B, NB, D, other_bytes=2 * sizes[0] + x.lo)
    expect_live(ms, idx)
    c0 = counts()
    rc = L.mlpg_hip_modspec_batch(di, stream, 1, x.ptr(), Ld.data_ptr(), B, Tm, D, N_FFT, ortho, ms.ptr())
    torch.cuda.synchronize()
    assert rc == 0 and moved(c0) == {17: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
    _close(get_live(ms, idx), R64.modspec(X, N_FFT, norm, lens), tol["ms"], "ms")
    note("modspec_batch", "x", x)
    note("modspec_batch", "ms", ms)
    assert ms.untouched(rest=0) == []
    ms.forget()
    # the gradient: grad_ms where ms was (zeros in the dead utterances)
    for i, b in enumerate(idx):
        ms.place(int(b), NB, 0, Gm[i])
    gx = parent(B, Tm, D, other_bytes=sizes[0] + x.lo + sizes[1] + ms.lo)
    expect_live(gx, idx)
    rc = L.mlpg_hip_modspec_batch_backward(di, stream, 1, x.ptr(), ms.ptr(), Ld.data_ptr(), B, Tm, D, N_FFT, ortho, gx.ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    got = get_live(gx, idx)
    live = R64.live_frames(lens, n, Tm, N_FFT)
    assert all(not got[i, live[i]:].any() for i in range(n))
    _close(got, R64.modspec_grad(X, Gm, N_FFT, norm, lens), tol["grad"], "grad")
    note("modspec_batch_backward", "x", x)
    note("modspec_batch_backward", "grad_ms", ms)
    note("modspec_batch_backward", "grad_x", gx)
    all_clean(("grad_ms", ms.untouched(rest=0)), ("grad_x", gx.untouched(rest=0)))
    ms.forget()
    # the fused loss step: target_ms where grad_ms was.  A dead utterance has the spectrum 0 and the target 0: f(0) - f(0) adds
    # nothing to the loss in either domain, so the reference over the live utterances is the whole loss.
    assert L.mlpg_hip_modspec_loss_form(N_FFT) == 1
    ws_bytes = int(L.mlpg_hip_modspec_loss_workspace_bytes(B, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    n_elems = float(n * NB * D)
    for log_domain in (1, 0):
        for i, b in enumerate(idx):
            ms.place(int(b), NB, 0, Tg[i])
        expect_live(gx, idx)
        loss = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        c0 = counts()
        rc = L.mlpg_hip_modspec_loss_step(di, stream, 1, x.ptr(), ms.ptr(), Ld.data_ptr(), B, Tm, D, N_FFT, ortho, log_domain, 1e-10,
                                          n_elems, gx.ptr(), loss.data_ptr(), ws.data_ptr(), ws_bytes)
        torch.cuda.synchronize()
        assert rc == 0 and moved(c0) == {19: 1}, (rc, L.mlpg_hip_last_error(), moved(c0))
        want, wgrad = R64.loss_and_grad(X, Tg, N_FFT, norm, lens, bool(log_domain), 1e-10, n_elems)
        _close(loss.cpu().numpy(), np.array([want]), tol["loss"], "loss")
        _close(get_live(gx, idx), wgrad, tol["grad"], "loss grad")
        note("modspec_loss_step", "x", x)
        note("modspec_loss_step", "target_ms", ms)
        note("modspec_loss_step", "grad_x", gx)
        all_clean(("target_ms", ms.untouched(rest=0)), ("grad_x", gx.untouched(rest=0)))
        ms.forget()
    assert x.untouched() == []
    for p in (x, ms, gx):
        p.free()


# ---------------------------------------------------------------------------------------------------- entries without lengths

@far_test
def test_trim_lengths():
    """An (N, T, D) batch of zeros in which only the utterances around the boundaries hold anything: the lengths are exact."""
    L, di, stream = lib_call()
    N = B_IN
    idx, lens = live_utterances(N, UTT_IN)
    rng = np.random.RandomState(5)
    X = np.zeros((len(idx), T, D))
    for i, n in enumerate(lens):
        X[i, :n] = rng.rand(n, D) + 0.1
        if n > 70:
            X[i, 40:60] = 0.0                                                       # zeros inside stay
    x = parent(N, T, D, fill_byte=0)
    put_live(x, idx, X)
    out = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = L.mlpg_hip_trim_lengths(di, stream, 1, x.ptr(), N, T, D, 1e-7, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    assert torch.equal(out, lengths_on_device(N, idx, lens))
    note("trim_lengths", "X", x)
    assert x.untouched() == []
    x.free()


@pytest.mark.parametrize("case", ["src_past_4GiB", "out_past_4GiB"])
@far_test
def test_gather_path(case):
    """path_len is 0 except around the boundaries of src (Tsrc = 1000, Tout = 300) or of out (Tsrc = 300, Tout = 1000); the
    gathered rows are exact copies and everything else of out is zero."""
    L, di, stream = lib_call()
    Tsrc, Tout = (T, 300) if case == "src_past_4GiB" else (300, T)
    N, Pmax = B_IN, 1000
    idx, plen = live_utterances(N, UTT_IN)
    plen = np.minimum(plen, Tout).astype(np.int32)
    rng = np.random.RandomState(9)
    S = rng.randn(len(idx), Tsrc, D)
    path = np.zeros((len(idx), Pmax), dtype=np.int32)
    for i, n in enumerate(plen):
        path[i, :n] = np.sort(rng.randint(0, Tsrc, size=n))
    src = parent(N, Tsrc, D, other_bytes=N * Tout * D * 8)
    out = parent(N, Tout, D, other_bytes=src.nbytes + src.lo)
    put_live(src, idx, S)
    expect_live(out, idx)
    pathd = torch.zeros((N, Pmax), dtype=torch.int32, device="cuda")
    pathd[torch.from_numpy(idx).cuda()] = torch.from_numpy(path).cuda()
    Pl = lengths_on_device(N, idx, plen)
    rc = L.mlpg_hip_gather_path(di, stream, 1, src.ptr(), pathd.data_ptr(), Pl.data_ptr(), N, Tsrc, Pmax, D, Tout, out.ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    got = get_live(out, idx)
    for i, n in enumerate(plen):
        assert np.array_equal(got[i, :n], S[i, path[i, :n]]) and not got[i, n:].any()
    note("gather_path", "src", src)
    note("gather_path", "out", out)
    assert set(BYTES) <= (src if case == "src_past_4GiB" else out).crossed()
    all_clean(("src", src.untouched()), ("out", out.untouched(rest=0)))
    src.free()
    out.free()


@far_test
def test_gmm_convert_mixture_form():
    """x (N, 64) float64 of 2^23 + 1024 rows -- 4 GiB and a block -- built on the device by tiling a block of 1024 rows; out
    (N, 64) the same size.  The result is compared on the device with the tiled float64 result of that block (the project's
    1e-10 float64 bound of tests/test_embed_entries_gpu.py against numpy, then the same bits in every tile)."""
    L, di, stream = lib_call()
    Dx, M, blk = 64, 4, 1024
    tiles = (1 << 23) // blk + 1
    N = tiles * blk
    assert N * Dx * 8 > 2 ** 32
    rng = np.random.RandomState(70)
    xb, mu_x, mu_y, A = rng.randn(blk, Dx), rng.randn(M, Dx), rng.randn(M, Dx), rng.randn(M, Dx, Dx) / 8.0
    mixb = rng.randint(M, size=blk).astype(np.int32)
    per = mu_y[None] + np.einsum("myd,nmd->nmy", A, xb[:, None, :] - mu_x[None])
    want = per[np.arange(blk), mixb]
    x = dev(xb).repeat(tiles, 1)
    mix = dev(mixb).repeat(tiles)
    out = torch.full((N, Dx), float("nan"), dtype=torch.float64, device="cuda")
    tabs = [dev(a) for a in (mu_x, mu_y, A)]
    rc = L.mlpg_hip_gmm_convert(di, stream, x.data_ptr(), None, mix.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(),
                                N, Dx, Dx, M, out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, L.mlpg_hip_last_error()
    first = out[:blk].cpu().numpy()
    assert np.abs(first - want).max() / np.abs(want).max() <= 1e-10
    same = (out.view(tiles, blk, Dx) == out[:blk][None]).all(dim=2).all(dim=1)
    assert bool(same.all()), "a tile differs from the first: rows from %s on" % (torch.nonzero(~same).flatten()[:4] * blk).tolist()
    COVER[("gmm_convert", "x")] |= set(BYTES)
    COVER[("gmm_convert", "out")] |= set(BYTES)
    del x, out, mix


# ---------------------------------------------------------------------------------------------------- coverage

def test_every_array_argument_crossed_every_boundary():
    """The table (entry, array argument) -> boundaries crossed, built from FarParent.crossed() as the tests above ran."""
    args = {"forward": ("mean", "out"), "backward": ("grad_out", "grad_mean"),
            "backward_var": ("mean", "var", "y", "grad_out", "grad_mean", "grad_var"), "delta_features": ("x", "out"),
            "gv_ascent": ("mean", "y_in", "y_out"), "unit_mse_step": ("mean", "target", "y_out", "grad_mean"),
            "modspec_batch": ("x", "ms"), "modspec_batch_backward": ("x", "grad_ms", "grad_x"),
            "modspec_loss_step": ("x", "target_ms", "grad_x"), "trim_lengths": ("X",), "gather_path": ("src", "out"),
            "gmm_convert": ("x", "out")}
    # What 12 GiB hold to 2^31 bytes alone.  mlpg_hip_backward_var: mean, grad_mean and grad_var have one shape, three of them
    # past 2^32 bytes are 12.9 GB before y and grad_out (which reach 2^31 bytes with the one-window set, where all five arrays
    # have 60 columns).  mlpg_hip_unit_mse_step: target and y_out are a third of mean and grad_mean with three windows, and with
    # one window the four arrays have one shape (17 GB past 2^32).
    only_2gib = {("backward_var", k) for k in ("mean", "var", "y", "grad_out", "grad_mean", "grad_var")} | {("unit_mse_step", "target"),
                                                                                                          ("unit_mse_step", "y_out")}
    nothing = set()
    print()
    missing = {}
    for entry, names in args.items():
        for arg in names:
            got = COVER.get((entry, arg), set())
            print("%-24s %-10s %s" % (entry, arg, ", ".join(sorted(got)) or "-"))
            want = set() if (entry, arg) in nothing else ({"2^31 bytes"} if (entry, arg) in only_2gib else set(BYTES))
            if want - got:
                missing[(entry, arg)] = sorted(want - got)
    assert not missing, missing
