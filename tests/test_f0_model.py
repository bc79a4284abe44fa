"""tools/f0_model.py, the executable specification of continuous F0, on the CPU: ``literal`` against what the
reference gave (tests/golden/f0_ref.npz, written by tests/golden/make_golden_f0.py) -- the step kinds and every untouched frame
bit for bit with NaNs in the same places, the linear kinds within 8 ulp of max(|a|, |b|) in float64 and 1 ulp of float32 in
float32; ``literal`` against the exact ``truth`` within 4 ulp; ``tiled`` (the kernel's partition) equal to ``literal`` bit for
bit at every tile size; ``batch`` against per-utterance ``literal``.

The 8: for positive finite knots a, b and the weight w = (t - p) / (q - p) in (0, 1), with u = 2^-53: the division, the
subtraction and the product each add a relative error u to a term of size at most |b - a|, the final sum a relative error u to
y, so the model's form is within (3 |b - a| + |y|) u <= 4 u max(|a|, |b|) <= 4 ulp(max(|a|, |b|)) of the exact value; SciPy's
two-weight form a (1 - w) + b w is within the same 4; 4 + 4 = 8.  The largest distance seen is printed (and kept in DESIGN.md)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f0_model as F0  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "f0_ref.npz"))
N = int(G["n"])
TRACKS = [(G["x%d" % i], G["y%d" % i], str(G["kinds"][i])) for i in range(N)]
LINEAR = ("slinear", "linear")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def knot_scale(x):
    """max(|a|, |b|) of every filled frame of a column (0 elsewhere)."""
    m = np.zeros(len(x))
    for t, _, s in F0.truth(x, "previous"):
        m[t] = s
    return m


def test_the_golden_file_holds_what_the_generator_says():
    assert 180 <= N <= 260 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "f0_ref.npz")) < 300 * 1024
    seen = dict(kinds=set(), dtypes=set(), ndim=set(), T=set(), unvoiced=set())
    flags = dict(none=0, all=0, one=0, nan0=0, nanend=0, nangap=0, nanrun=0, lead=0, trail=0)
    for x, y, kind in TRACKS:
        assert y.shape == x.shape and y.dtype == x.dtype
        seen["kinds"].add(kind), seen["dtypes"].add(x.dtype), seen["ndim"].add(x.ndim), seen["T"].add(len(x))
        f = x.ravel()
        v = f > 0
        flags["none"] += not v.any()
        flags["all"] += v.all()
        flags["one"] += v.sum() == 1
        flags["nan0"] += np.isnan(f[0])
        flags["nanend"] += np.isnan(f[-1])
        inner = np.flatnonzero(np.isnan(f[1:-1])) + 1
        flags["nangap"] += any(not v[t - 1] for t in inner)
        flags["nanrun"] += any(v[t + 1] and v[t - 1] for t in inner)
        flags["lead"] += not v[0] and v.any()
        flags["trail"] += not v[-1] and v.any()
        for z in f[~v & ~np.isnan(f)]:
            seen["unvoiced"].add((float(z), bool(np.signbit(z))))
    assert seen["kinds"] == set(F0.KINDS) and seen["dtypes"] == {np.dtype(np.float32), np.dtype(np.float64)} and seen["ndim"] == {1, 2}
    assert min(seen["T"]) == 2 and max(seen["T"]) == 700 and {255, 256, 257} <= seen["T"]
    assert seen["unvoiced"] == {(0.0, False), (0.0, True), (-1e10, True)}
    assert all(n > 0 for n in flags.values()), flags
    shares = [np.mean(x > 0) for x, _, _ in TRACKS if len(x) >= 255 and not np.isnan(x).any()]
    assert min(shares) < 0.15 and max(shares) > 0.85


def test_literal_against_the_reference():
    worst = {np.dtype(np.float32): 0.0, np.dtype(np.float64): 0.0}
    for i, (x, want, kind) in enumerate(TRACKS):
        got = F0.literal(x.ravel(), kind).reshape(x.shape)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), i
        f = x.ravel()
        if kind not in LINEAR:
            assert same_bits(got, want), (i, kind)
            continue
        scale = knot_scale(f)
        filled = scale > 0
        g, w = got.ravel(), want.ravel()
        assert np.array_equal(bits(g[~filled]), bits(w[~filled])), (i, kind)          # untouched frames, knots, edge holds
        if not filled.any():
            continue
        if x.dtype == np.float64:
            d = np.abs(g[filled] - w[filled]) / np.spacing(scale[filled])
            bound = 8.0
        else:
            d = np.abs(g[filled].astype(np.float64) - w[filled].astype(np.float64)) / np.spacing(np.abs(w[filled])).astype(np.float64)
            bound = 1.0
        worst[x.dtype] = max(worst[x.dtype], float(d.max()))
        assert d.max() <= bound, (i, kind, d.max())
    print("literal against the reference, linear kinds: worst %.3g ulp of max(|a|, |b|) in float64 (bound 8), %.3g ulp in float32 (bound 1)"
          % (worst[np.dtype(np.float64)], worst[np.dtype(np.float32)]))


def test_literal_against_the_exact_value():
    worst = 0.0
    for x, _, kind in TRACKS:
        f = x.ravel()
        if kind not in LINEAR or x.dtype != np.float64:
            continue
        y = F0.literal(f, kind)
        for t, exact, scale in F0.truth(f, kind):
            from fractions import Fraction
            d = abs(Fraction(float(y[t])) - exact) / Fraction(float(np.spacing(scale)))
            worst = max(worst, float(d))
            assert d <= 4, (t, float(d))
    print("literal against the exact value: worst %.3g ulp of max(|a|, |b|) (bound 4)" % worst)
    assert worst > 0


def test_equal_knots_give_exactly_the_knot():
    x = np.array([0.0, 5.1, 0, 0, 0, 5.1, -1e10, -0.0, 5.1, 0])
    for kind in F0.KINDS:
        assert np.array_equal(F0.literal(x, kind), np.full(10, 5.1))
        assert np.array_equal(F0.vuv(x), [0, 1, 0, 0, 0, 1, 0, 0, 1, 0])


@pytest.mark.parametrize("tile", [1, 2, 3, 64, 256, None])
def test_tiled_equals_literal_bit_for_bit(tile):
    for x, _, kind in TRACKS:
        f = x.ravel()
        stats = {}
        assert same_bits(F0.tiled(f, kind, tile or len(f) + 5, stats=stats), F0.literal(f, kind))
        assert stats["walk"] == len(f) and stats["ahead"] <= len(f)                  # every frame is read at most twice
    rng = np.random.RandomState(7)
    for L in (0, 1, 2, 3, 5, 40):
        for _ in range(20):
            f = np.where(rng.rand(L) < 0.3, 4 + rng.rand(L), rng.choice([0.0, -0.0, -1e10, np.nan, np.inf], size=L))
            for kind in F0.KINDS:
                for out in (np.float32, np.float64):
                    assert same_bits(F0.tiled(f, kind, tile or L + 5, dtype=out), F0.literal(f, kind, dtype=out)), (f, kind)


def test_one_frame_and_unknown_kinds():
    assert np.array_equal(F0.literal(np.array([5.0])), [5.0]) and np.array_equal(F0.literal(np.array([-1e10])), [-1e10])
    assert len(F0.literal(np.zeros(0))) == 0
    for kind in ("quadratic", "cubic", 1, None, "Linear"):
        with pytest.raises(ValueError, match="kind must be one of"):
            F0.literal(np.ones(3), kind)


def test_batch_against_per_utterance_literal():
    rng = np.random.RandomState(11)
    B, Tmax, C = 6, 50, 3
    X = np.where(rng.rand(B, Tmax, C) < 0.4, 4 + rng.rand(B, Tmax, C), 0.0).astype(np.float32)
    lengths = np.array([0, 50, 73, 1, -4, 20])
    for kind in ("slinear", "nearest"):
        Y, V = F0.batch(X, lengths, kind, vuv_dtype=np.float64)
        assert Y.dtype == np.float32 and V.dtype == np.float64 and Y.shape == V.shape == X.shape
        for b, Lb in enumerate([0, 50, 50, 1, 0, 20]):
            assert not Y[b, Lb:].any() and not V[b, Lb:].any()
            for c in range(C):
                assert same_bits(Y[b, :Lb, c], F0.literal(X[b, :Lb, c], kind))
                assert np.array_equal(V[b, :Lb, c], X[b, :Lb, c] > 0)
        Yt, Vt = F0.batch(X, lengths, kind, vuv_dtype=np.float64, fn=F0.tiled)
        assert same_bits(Yt, Y) and same_bits(Vt, V)
    Y2, V2 = F0.batch(X[:, :, 0], None, "linear")
    Y3, _ = F0.batch(X[:, :, :1], None, "linear")
    assert Y2.shape == (B, Tmax) and same_bits(Y2, Y3[:, :, 0]) and V2.dtype == np.float32
