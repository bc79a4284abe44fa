"""The case list that tests/test_f0_host_cpu.py (the kernel text on the CPU) and tests/test_f0_gpu.py (the kernel on the device)
share: padded batches of F0-like tracks chosen for where a walk in tiles of 256 frames can break, and what tools/f0_model.py
gives on them.  A case is a dict: name, X (B, Tmax, C) float64 with NaN in the rows at or past each length, lengths (int32 (B)
or None), kind, dtypes (x, y, vuv), mode ("both", "y", "vuv", "inplace", "inplace_y")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f0_model as F0  # noqa: E402

TILE = F0.TILE
F32, F64 = np.float32, np.float64
SENTINEL = -7
MODES = ("both", "y", "vuv", "inplace", "inplace_y")
LENGTHS = (0, 1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5)


def runs(rng, L, share=0.5, unvoiced=(0.0, -0.0, -1e10)):
    """L frames in voiced runs (values in 4.5 .. 5.5) and unvoiced runs, each unvoiced run written as one of `unvoiced`."""
    x = np.empty(L)
    t, on = 0, rng.rand() < share
    while t < L:
        n = 1 + rng.geometric(1.0 / (1 + 12 * (share if on else 1 - share)))
        x[t:t + n] = (4.5 + rng.rand(min(n, L - t))) if on else unvoiced[rng.randint(len(unvoiced))]
        t += n
        on = not on
    return x


def voiced_only(rng, L, spans):
    """L unvoiced frames (0) with voiced values in the half-open spans."""
    x = np.zeros(L)
    for s, e in spans:
        x[s:e] = 4.5 + rng.rand(e - s)
    return x


def structural(rng):
    """(name, track): one track per place where the tile logic can break."""
    T = TILE
    L = 3 * T + 5
    out = [("gap over one whole tile", voiced_only(rng, L, [(0, 200), (2 * T + 8, L)])),
           ("gap over two whole tiles", voiced_only(rng, 4 * T + 76, [(0, 100), (3 * T + 32, 4 * T + 76)])),
           ("gap from a tile's last frame to the next tile's first", voiced_only(rng, L, [(0, T - 1), (2 * T, L)])),
           ("gap that is a tile's last frame alone", voiced_only(rng, L, [(0, T - 1), (T, L)])),
           ("gap that ends on a tile's first frame", voiced_only(rng, L, [(0, T - 40), (T + 1, L)])),
           ("first voiced frame in the last tile", voiced_only(rng, L, [(3 * T + 1, 3 * T + 3)])),
           ("last voiced frame in the first tile", voiced_only(rng, L, [(10, 20)])),
           ("one voiced frame at 0", voiced_only(rng, L, [(0, 1)])),
           ("one voiced frame at the end", voiced_only(rng, L, [(L - 1, L)])),
           ("one voiced frame in the middle", voiced_only(rng, L, [(T + 77, T + 78)])),
           ("one voiced frame on a tile's last frame", voiced_only(rng, L, [(2 * T - 1, 2 * T)])),
           ("one voiced frame on a tile's first frame", voiced_only(rng, L, [(2 * T, 2 * T + 1)])),
           ("all voiced", 4.5 + rng.rand(L)),
           ("none voiced", rng.choice([0.0, -0.0, -1e10], size=L)),
           ("none voiced with NaN", np.where(rng.rand(L) < 0.1, np.nan, -1e10)),
           ("two frames, the second voiced", np.array([0.0, 5.0])),
           ("two frames, the first voiced", np.array([5.0, -1e10])),
           ("three frames, the middle voiced", np.array([np.nan, 5.0, 0.0]))]
    x = runs(rng, L)
    x[0] = x[-1] = np.nan
    x[5], x[L - 9] = 5.25, 4.75
    out.append(("NaN at 0 and at the end", x))
    x = voiced_only(rng, L, [(3, T - 10), (T + 30, 2 * T + 3), (2 * T + 100, L - 30)])
    x[T] = x[T + 1] = x[L - 10] = np.nan                      # inside a gap (on a tile's first frame) and in the trailing silence
    x[50] = x[2 * T - 1] = np.nan                             # inside voiced runs (one on a tile's last frame)
    out.append(("NaN inside gaps and runs", x))
    return out


def pack(tracks, C=1, rng=None):
    """(X (B, Tmax, C), lengths): the tracks as column 0 of a padded batch (further columns: random tracks of the same lengths);
    NaN in the rows at or past each length."""
    B, Tmax = len(tracks), max(max(len(t) for t in tracks), 1)
    X = np.full((B, Tmax, C), np.nan)
    for b, t in enumerate(tracks):
        X[b, :len(t), 0] = t
        for c in range(1, C):
            X[b, :len(t), c] = runs(rng, len(t), (0.1, 0.8)[c % 2])
    return X, np.array([len(t) for t in tracks], dtype=np.int32)


def _case(name, X, lengths, kind="slinear", dtypes=(F64, F64, F64), mode="both"):
    return dict(name=name, X=X, lengths=lengths, kind=kind, dtypes=dtypes, mode=mode)


def cases():
    rng = np.random.RandomState(15)
    out = []
    # every length around the tile, three columns, every kind
    tracks = [runs(rng, L) for L in LENGTHS]
    X, lengths = pack(tracks, 3, rng)
    for i, kind in enumerate(F0.KINDS):
        out.append(_case("lengths-%s" % kind, X, lengths, kind, ((F64, F64, F64), (F32, F32, F32))[i % 2]))
    # the structural tracks, one batch, the kinds and modes taking turns
    names, tracks = zip(*structural(rng))
    X, lengths = pack(tracks)
    for kind, dtypes, mode in (("slinear", (F64, F64, F64), "both"), ("linear", (F32, F32, F32), "inplace"), ("nearest", (F64, F64, F32), "y"),
                               ("nearest-up", (F32, F64, F64), "both"), ("previous", (F64, F32, F64), "both"), ("next", (F32, F32, F64), "inplace_y"),
                               ("zero", (F64, F64, F32), "vuv")):
        out.append(_case("structural-%s-%s" % (kind, mode), X, lengths, kind, dtypes, mode))
    # lengths above Tmax and negative; no lengths at all (Tmax not a multiple of the tile; one utterance)
    tracks = [runs(rng, 300, 0.3) for _ in range(5)]
    X, _ = pack(tracks, 3, rng)
    out.append(_case("clamped-lengths", X, np.array([300, 301, 1 << 30, -5, 300], dtype=np.int32), "slinear", (F32, F32, F32), "inplace"))
    out.append(_case("no-lengths", X, None, "linear", (F64, F32, F32)))
    out.append(_case("one-utterance", X[:1, :, :1], None, "nearest", (F32, F64, F32)))
    out.append(_case("empty-utterances", X[:2], np.zeros(2, dtype=np.int32), "slinear", (F32, F32, F32)))
    return out


def expected(case):
    """(y, vuv) of the model for a case, in its output dtypes (B, Tmax, C)."""
    dx, dy, dv = case["dtypes"]
    if case["mode"] in ("inplace", "inplace_y"):
        dy = dx
    return F0.batch(case["X"].astype(dx), case["lengths"], case["kind"], dtype=dy, vuv_dtype=dv)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def verdict(case, got):
    """The checks that fail, as texts.  got: (x after the call, y, vuv, x before it, (off_x, off_y, off_v)), the arrays
    (B, Tmax, ld) with the batch in columns off .. off + C - 1, the outputs pre-filled with SENTINEL."""
    xa, ya, va, wide, (off_x, off_y, off_v) = got
    C = case["X"].shape[2]
    want_y, want_v = expected(case)
    mode = case["mode"]
    fails = []

    def foreign(a, off, what):
        mask = np.ones(a.shape[2], dtype=bool)
        mask[off:off + C] = False
        if not (a[:, :, mask] == SENTINEL).all():
            fails.append("foreign columns of %s" % what)
    if mode in ("inplace", "inplace_y"):
        back = wide.copy()
        back[:, :, off_x:off_x + C] = want_y
        if not same_bits(xa, back):
            fails.append("y in place (or x's foreign columns)")
        if not (ya == SENTINEL).all():
            fails.append("the unused y was written")
    else:
        if not same_bits(xa, wide):
            fails.append("x changed")
        if mode == "vuv":
            if not (ya == SENTINEL).all():
                fails.append("the unused y was written")
        else:
            foreign(ya, off_y, "y")
            if not same_bits(np.ascontiguousarray(ya[:, :, off_y:off_y + C]), want_y):
                fails.append("y")
    if mode in ("y", "inplace_y"):
        if not (va == SENTINEL).all():
            fails.append("the unused vuv was written")
    else:
        foreign(va, off_v, "vuv")
        if not same_bits(np.ascontiguousarray(va[:, :, off_v:off_v + C]), want_v):
            fails.append("vuv")
    return fails
