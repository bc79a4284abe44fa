"""The case list of the joint-rows kernels, shared by the host run of the kernel text (tests/test_joint_host_cpu.py), the model's
own tests (tests/test_joint_model.py) and the device (tests/test_joint_gpu.py, tests/test_embed_joint_gpu.py): the smallest shapes
at which the three stages can go wrong.  A case is a dict: name, X (B, Tmax, Dx) and Y (B, Tmax, Dy) or None in float64, len_x /
len_y (None: NULL), wins (a list of (l, u, coef)), keep, eps, dtypes (x, y, out), cap (None: exactly N), pad (ld_out - W).

Two properties of the data are checked here, on the CPU, when the module is imported (check_margins): the threshold rows are
single-element rows (no summation order can decide them), and every other live row of every NONZERO case has s == 0, a NaN s, or
s >= 1e-3 and >= 4 eps."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import joint_model as JM  # noqa: E402

TILE = JM.TILE
F32, F64 = np.float32, np.float64
W0 = []
W2 = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
W3 = W2 + [(1, 1, np.array([1.0, -2.0, 1.0]))]
WIDE = [(0, 0, np.array([1.0])), (8, 3, np.array([0.5, -1.0, 0.25, 2.0, -0.75, 1.5, 0.125, -2.0, 1.0, 0.5, -0.25, 3.0]))]


def frames(rng, B, T, D):
    """Values of magnitude 1 + (t mod 7) + [0, 0.25) with random signs: every element, and every difference or sum of two
    frames one or two apart, is at least 0.75 in magnitude."""
    t = np.arange(T)[None, :, None]
    return ((1 + t % 7) + 0.25 * rng.rand(B, T, D)) * np.where(rng.rand(B, T, D) < 0.5, -1.0, 1.0)


def case(name, rng, B, Tmax, Dx, Dy, wins, len_x="full", len_y="full", zeros=(), keep=JM.NONZERO, eps=1e-7, dtypes=(F64, F64, F64), cap=None,
         pad=0, threshold=False):
    X = frames(rng, B, Tmax, Dx)
    Y = frames(rng, B, Tmax, Dy) if Dy else None
    for b, t in zeros:
        X[b, t] = 0.0
        if Y is not None:
            Y[b, t] = 0.0
    full = np.full(B, Tmax, dtype=np.int32)
    lx = None if len_x is None else (full if isinstance(len_x, str) else np.array(len_x, dtype=np.int32))
    ly = None if len_y is None else (full if isinstance(len_y, str) else np.array(len_y, dtype=np.int32))
    return dict(name=name, X=X, Y=Y, len_x=lx, len_y=ly, wins=wins, keep=keep, eps=eps, dtypes=dtypes, cap=cap, pad=pad, threshold=threshold)


def _build():
    rng = np.random.RandomState(1717)
    T = TILE
    cs = [case("t1-b1-d1", rng, 1, 1, 1, 0, W0, None, None)]
    cs.append(case("t63-b3-d5-5-w3", rng, 3, T - 1, 5, 5, W3, [T - 1, 2, 0], [T - 1, 1, 0], zeros=[(0, 0), (0, T - 2), (0, 30), (1, 1)]))
    cs.append(case("t64-b3-d63-64-w2", rng, 3, T, 63, 64, W2, [T, 1, 40], [T, 2, 33], zeros=[(0, 0), (0, T - 1), (2, 32), (2, 39)], pad=3))
    cs.append(case("t65-b3-d64-65-w0", rng, 3, T + 1, 64, 65, W0, [T + 1, T, 2], [T + 1, T + 1, 2], zeros=[(0, T - 1), (0, T), (1, T)]))
    cs.append(case("t131-b3-d65-130-w3-f32", rng, 3, 2 * T + 3, 65, 130, W3, [2 * T + 3, 2 * T + 3, 70], [2 * T + 3, 2 * T + 3, 2 * T],
                   zeros=[(0, t) for t in (T - 1, T, T + 1, 2 * T - 1, 2 * T)] + [(1, t) for t in range(T - 1, 2 * T + 1)], dtypes=(F32, F32, F64)))
    lens70 = [(0, 1, 2, 2 * T + 3, T, T + 1, 99)[b % 7] for b in range(70)]
    cs.append(case("t131-b70-d1-w2", rng, 70, 2 * T + 3, 1, 0, W2, lens70, None, zeros=[(b, t) for b in range(3, 70, 7) for t in (0, 5, T, 2 * T + 2)]))
    cs.append(case("t131-b70-d130-w0-f32", rng, 70, 2 * T + 3, 130, 0, W0, lens70[::-1], None, zeros=[(b, T - 1) for b in range(70)],
                   dtypes=(F32, F32, F32)))
    c = case("all-dropped", rng, 3, T + 1, 5, 1, W3, "full", [3, 0, T])
    c["X"][:] = 0.0
    c["Y"][:] = 0.0
    cs.append(c)
    cs.append(case("all-kept-null-lengths", rng, 3, T + 1, 5, 1, W3, None, None))
    c = case("static-zero-delta-not", rng, 1, 10, 1, 0, W2, None, None)
    c["X"][0, :3, 0] = 0.0                                   # frame 2: static 0, delta 0.5 * x[3]: kept; frames 0, 1 dropped
    cs.append(c)
    for name, wins in (("negzero-nan-w0", W0), ("negzero-nan-w3", W3)):
        c = case(name, rng, 1, T + 6, 5, 5, wins, "full", "full", zeros=[(0, 3), (0, T), (0, 20), (0, 21), (0, 22)])
        c["X"][0, 3] = -0.0                                  # a row of -0.0 and 0.0: dropped
        c["X"][0, 21] = -0.0
        c["X"][0, 8, 2] = -0.0                               # -0.0 in a kept row keeps its sign where nothing is computed
        c["Y"][0, T + 1, 4] = np.nan                         # a NaN row: dropped (with windows its neighbours too)
        cs.append(c)
    zs = [(0, 1), (0, T - 1), (0, T), (1, 0), (2, 2)]
    for dts in ((F32, F64, F32), (F64, F32, F64), (F64, F64, F32), (F32, F32, F32)):
        cs.append(case("mix-%s" % "-".join(np.dtype(d).name for d in dts), rng, 3, T + 1, 5, 5, W3, [T + 1, 40, 3], [T, 44, 3], zeros=zs, dtypes=dts))
    cs.append(case("live-w3", rng, 3, T + 1, 5, 5, W3, [T + 1, 40, 0], [T, 44, 0], zeros=zs, keep=JM.LIVE))
    cs.append(case("live-null-lengths-w0", rng, 3, T + 1, 5, 0, W0, None, None, zeros=zs, keep=JM.LIVE, dtypes=(F32, F32, F64)))
    for name, cap in (("cap-below", -3), ("cap-above", 5), ("cap-zero", None)):
        c = case(name, rng, 3, T + 1, 5, 5, W2, [T + 1, 40, 3], [T, 44, 3], zeros=zs, pad=3)
        n = int(JM.literal(c["X"], c["Y"], c["len_x"], c["len_y"], c["wins"])[1][-1])
        c["cap"] = 0 if cap is None else n + cap
        cs.append(c)
    cs.append(case("wide-window-short-utterances", rng, 3, T + 1, 5, 1, WIDE, [T + 1, 2, 5], [T + 1, 1, 5], zeros=[(0, 40)]))
    cs.append(case("eps-zero", rng, 2, 7, 1, 1, W0, "full", "full", zeros=[(0, 2), (1, 6)], eps=0.0))
    # threshold rows: ONE element per row, so no summation order can decide
    c = case("threshold-1e-7", rng, 1, 6, 1, 0, W0, None, None, threshold=True)
    c["X"][0, :, 0] = [1e-7, np.nextafter(1e-7, 1.0), 0.5e-7, 1.0, 0.0, -2.0]          # dropped, kept, dropped, kept, dropped, kept
    cs.append(c)
    c = case("threshold-quarter-f32", rng, 1, 6, 1, 0, W0, None, None, eps=0.25, dtypes=(F32, F32, F32), threshold=True)
    c["X"][0, :, 0] = [0.25, np.nextafter(F32(0.25), F32(1.0)), 0.125, -1.0, -0.25, 0.0]
    cs.append(c)
    return cs


_CASES = _build()
_EXPECTED = {}


def cases():
    return _CASES


def typed(c):
    """The sources in their dtypes: (X, Y or None)."""
    dx, dy, _ = c["dtypes"]
    return c["X"].astype(dx), None if c["Y"] is None else c["Y"].astype(dy)


def expected(c):
    """(all N kept rows (N, W) in the output's dtype, offsets (B + 1)), from the model's literal form; computed once per case."""
    if c["name"] not in _EXPECTED:
        X, Y = typed(c)
        _EXPECTED[c["name"]] = JM.literal(X, Y, c["len_x"], c["len_y"], c["wins"], c["keep"], c["eps"], c["dtypes"][2])
    return _EXPECTED[c["name"]]


def width(c):
    return (c["X"].shape[2] + (0 if c["Y"] is None else c["Y"].shape[2])) * max(len(c["wins"]), 1)


def capacity(c):
    return len(expected(c)[0]) if c["cap"] is None else c["cap"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def verdict(c, out, offsets, sentinel=-7.0, off=0):
    """What fails ([]: nothing).  out: (cap, ld_out) as the call left it, pre-filled with `sentinel`; the rows start at column off."""
    rows, offs = expected(c)
    W, cap = width(c), capacity(c)
    n = min(len(rows), cap)
    fails = []
    if not same_bits(np.asarray(offsets, dtype=np.int64), offs):
        fails.append("offsets")
    if not same_bits(out[:n, off:off + W], rows[:n]):
        fails.append("rows")
    rest = out.copy()
    rest[:n, off:off + W] = sentinel
    if not (rest == sentinel).all():
        fails.append("stray write")
    return fails


def wide_source(A, lengths, extra, off):
    """A as columns off .. of rows `extra` wider; NaN in the other columns and in the rows at or past the lengths."""
    B, Tmax, D = A.shape
    wide = np.full((B, Tmax, D + extra), np.nan, dtype=A.dtype)
    wide[:, :, off:off + D] = A
    if lengths is not None:
        for b, n in enumerate(np.clip(lengths, 0, Tmax)):
            wide[b, n:] = np.nan
    return wide


def check_margins():
    for c in _CASES:
        if c["keep"] != JM.NONZERO:
            continue
        X, Y = typed(c)
        B = X.shape[0]
        lx = JM.clamp(c["len_x"], B, X.shape[1])
        ly = JM.clamp(c["len_y"], B, X.shape[1]) if Y is not None else np.zeros(B, dtype=np.int64)
        if c["threshold"]:
            assert width(c) == 1, c["name"]
            continue
        for b in range(B):
            rows, _ = JM.utterance(X[b], None if Y is None else Y[b], int(lx[b]), int(ly[b]), c["wins"], JM.LIVE, 0.0, c["dtypes"][2])
            s = JM.abs_sums(rows[:max(lx[b], ly[b])])
            ok = (s == 0) | np.isnan(s) | ((s >= 1e-3) & (s >= 4 * c["eps"]))
            assert ok.all(), (c["name"], b, s[~ok])


check_margins()
