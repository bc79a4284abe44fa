"""The case list that tests/test_wave_host_cpu.py (the kernel text on the CPU) and tests/test_wave_gpu.py (the kernels on the device)
share: padded batches of waveforms chosen for where 4 samples per thread, tiles of 1024 samples and segments with a warm-up can
break, and what tools/wave_model.py gives on them.  A case is a dict: name, op ("encode" / "decode"), X (B, Lmax) in the input's
dtype with NaN (classes: far outside [0, mu]) at or past each length, lengths (int32 (B) or None), coef (None: no emphasis),
stage, mu, segment (decode: the C entry's value), dtypes (x, y), layout ("wide": utterance stride Lmax + 3 starting one element
in, so nothing is aligned; "dense": stride Lmax from an aligned start), mode ("out", "inplace", or "refused": the call must
return -1 and write nothing)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wave_model as WM  # noqa: E402

TILE = WM.TILE
F32, F64, U8, I16, I32, I64 = np.float32, np.float64, np.uint8, np.int16, np.int32, np.int64
LENGTHS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, 3077, 7000)
TILE_ENDS = (TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE, 4 * TILE - 3, 4 * TILE)        # lengths that end on a tile's first and last sample
SENTINEL = -7                                                                          # (249 as uint8)
# a class may differ from the model's only where the float64 value v lies this close to an integer: the host's or the device's
# float64 log1p against numpy's moves v by a few ulp of 256, about 1e-12 bins
CLASS_BAND = 2.0 ** -30


def wave(rng, L, scale=0.3):
    """A speech-like waveform of L samples in (-1, 1): a slow random walk under an envelope, some exact zeros and a -0.0."""
    x = np.cumsum(rng.randn(L)) * 0.02 + rng.randn(L) * scale * 0.2
    x = np.clip(x * np.abs(np.sin(np.arange(L) / 211.0)) * scale / max(np.abs(x).max(initial=0.0), 1e-3) * 3, -0.999, 0.999)
    if L > 8:
        x[3] = 0.0
        x[7] = -0.0
    return x


def pack(tracks, fill):
    B, Lmax = len(tracks), max(max(len(t) for t in tracks), 1)
    X = np.full((B, Lmax), fill, dtype=np.asarray(tracks[0]).dtype if len(tracks[0]) else np.float64)
    for b, t in enumerate(tracks):
        X[b, :len(t)] = t
    return X, np.array([len(t) for t in tracks], dtype=np.int32)


def _case(name, op, X, lengths, coef=None, stage=WM.PLAIN, mu=256, segment=0, dtypes=(F32, F32), layout="wide", mode="out"):
    return dict(name=name, op=op, X=X, lengths=lengths, coef=coef, stage=stage, mu=mu, segment=segment, dtypes=dtypes, layout=layout,
                mode=mode)


def cases():
    rng = np.random.RandomState(16)
    out = []
    X, lengths = pack([wave(rng, L) for L in LENGTHS], np.nan)                 # (12, 7000)
    NONE = 1 << 40                                                             # segment >= Lmax: no split
    # ---- decode, de-emphasis: every length, the three segment settings, both layouts, dtype mixes
    for name, coef, seg, dts, layout in (("deemph-none-f64", 0.97, NONE, (F64, F64), "wide"), ("deemph-none-f32", 0.97, NONE, (F32, F32), "dense"),
                                         ("deemph-seg2048-f64", 0.5, 2048, (F64, F64), "dense"), ("deemph-seg2048-f32-f64", 0.5, 2048, (F32, F64), "wide"),
                                         ("deemph-auto-f64-f32", 0.97, 0, (F64, F32), "wide"), ("deemph-negative-coef", -0.97, 4096, (F32, F32), "dense"),
                                         ("deemph-0.999-none", 0.999, NONE, (F64, F64), "dense")):
        out.append(_case(name, "decode", X, lengths, coef, WM.PLAIN, 256, seg, dts, layout))
    # the automatic split needs Lmax > 16384: two utterances, one of them short
    Xl, ll = pack([wave(rng, 2 * 16384 + 1029), wave(rng, 16384 + 1)], np.nan)
    out.append(_case("deemph-auto-split", "decode", Xl, ll, 0.97, WM.PLAIN, 256, 0, (F32, F32), "dense"))
    Xe, le = pack([wave(rng, L) for L in TILE_ENDS], np.nan)
    out.append(_case("deemph-tile-ends", "decode", Xe, le, 0.85, WM.PLAIN, 256, 2048, (F64, F64), "wide"))
    out.append(_case("deemph-no-lengths", "decode", np.nan_to_num(Xe), None, 0.85, WM.PLAIN, 256, 1024, (F32, F32), "dense"))
    out.append(_case("deemph-clamped-lengths", "decode", np.nan_to_num(Xe[:3, :2051]), np.array([1 << 30, -5, 2051], dtype=np.int32), 0.5, WM.PLAIN, 256, 1024,
                     (F64, F64), "wide"))
    # ---- decode, the table: all four class dtypes (classes outside [0, mu] in two live places: clamped), with and without de-emphasis
    classes = {}
    for i, (dt, mu) in enumerate(((U8, 255), (I16, 256), (I32, 256), (I64, 1023))):
        C = classes[dt] = rng.randint(0, mu + 1, size=X.shape).astype(dt)
        C[np.arange(X.shape[1])[None, :] >= lengths[:, None]] = 200 if dt == U8 else 9999
        if dt != U8:
            C[11, 5], C[11, 6] = -3, mu + 7
        out.append(_case("table-%s" % np.dtype(dt).name, "decode", C, lengths, None, WM.QUANTIZE, mu, 0, (dt, (F32, F64)[i % 2]), ("dense", "wide")[i % 2]))
        out.append(_case("table-deemph-%s" % np.dtype(dt).name, "decode", C, lengths, float(np.float32(0.97)), WM.QUANTIZE, mu, (NONE, 4096)[i % 2],
                         (dt, (F32, F64)[(i + 1) % 2]), ("wide", "dense")[i % 2]))
    C = rng.randint(0, 5000, size=(2, 1500)).astype(I32)
    out.append(_case("table-longer-than-lds", "decode", C, None, None, WM.QUANTIZE, 4999, 0, (I32, F32), "dense"))
    out.append(_case("inv-mulaw-float", "decode", (X * 3).astype(F32), lengths, None, WM.MULAW, 256, 0, (F32, F32), "dense"))
    out.append(_case("inv-mulaw-float-f64", "decode", X * 3, lengths, None, WM.MULAW, 255, 0, (F64, F64), "wide"))
    out.append(_case("decode-plain-convert", "decode", X, lengths, None, WM.PLAIN, 256, 0, (F64, F32), "wide"))
    # ---- encode
    for name, coef, stage, mu, dts, layout in (("preemph-f32", 0.97, WM.PLAIN, 256, (F32, F32), "dense"), ("preemph-f64", 0.97, WM.PLAIN, 256, (F64, F64), "wide"),
                                               ("preemph-f32-to-f64", -0.85, WM.PLAIN, 256, (F32, F64), "wide"), ("mulaw-f32", None, WM.MULAW, 256, (F32, F32), "wide"),
                                               ("mulaw-f64-255", None, WM.MULAW, 255, (F64, F64), "dense"), ("preemph-mulaw-f64-to-f32", 0.97, WM.MULAW, 256, (F64, F32), "dense"),
                                               ("quantize-u8", None, WM.QUANTIZE, 255, (F32, U8), "dense"), ("quantize-i16", None, WM.QUANTIZE, 256, (F64, I16), "wide"),
                                               ("preemph-quantize-i32", 0.97, WM.QUANTIZE, 256, (F32, I32), "wide"),
                                               ("preemph-quantize-i64", 0.97, WM.QUANTIZE, 1023, (F64, I64), "dense"),
                                               ("preemph-quantize-u8-wide", 0.5, WM.QUANTIZE, 255, (F32, U8), "wide")):
        out.append(_case(name, "encode", X, lengths, coef, stage, mu, 0, dts, layout))
    out.append(_case("encode-no-lengths-over-one", "encode", np.nan_to_num(Xe) * 4, None, 0.97, WM.QUANTIZE, 256, 0, (F32, I16), "dense"))
    out.append(_case("encode-nonfinite", "encode", np.array([[0.1, np.inf, 0.2, 0.3, np.nan, 0.1, -np.inf, 0.5, 0.25]]), None, 0.97, WM.MULAW, 256, 0,
                     (F64, F64), "dense"))
    # ---- in place: allowed without emphasis when the element sizes match, refused with it (and with unequal sizes)
    out.append(_case("inplace-mulaw-f32", "encode", X, lengths, None, WM.MULAW, 256, 0, (F32, F32), "wide", "inplace"))
    out.append(_case("inplace-quantize-f32-i32", "encode", X, lengths, None, WM.QUANTIZE, 256, 0, (F32, I32), "dense", "inplace"))
    out.append(_case("inplace-table-i32-f32", "decode", classes[I32], lengths, None, WM.QUANTIZE, 256, 0, (I32, F32), "dense", "inplace"))
    out.append(_case("inplace-inv-mulaw-f64", "decode", X, lengths, None, WM.MULAW, 256, 0, (F64, F64), "wide", "inplace"))
    out.append(_case("refused-inplace-preemph", "encode", X[:2, :9], None, 0.97, WM.PLAIN, 256, 0, (F32, F32), "dense", "refused"))
    out.append(_case("refused-inplace-deemph", "decode", X[:2, :9], None, 0.97, WM.PLAIN, 256, 0, (F64, F64), "dense", "refused"))
    out.append(_case("refused-inplace-sizes", "encode", X[:2, :9], None, None, WM.QUANTIZE, 256, 0, (F64, I32), "dense", "refused"))
    assert len(set(c["name"] for c in out)) == len(out)
    return out


def layout_of(case):
    """(ld_x, off_x, ld_y, off_y) in elements."""
    Lmax = case["X"].shape[1]
    return (Lmax + 3, 1, Lmax + 5, 2) if case["layout"] == "wide" else (Lmax, 0, Lmax, 0)


def x_fill(case):
    """What the foreign elements of x hold."""
    return np.nan if np.dtype(case["dtypes"][0]).kind == "f" else 77


def buffers(case):
    """(x, y) as the call gets them: (B, ld) arrays, the batch at columns off .. off + Lmax - 1, y pre-filled with SENTINEL."""
    dx, dy = (np.dtype(t) for t in case["dtypes"])
    X = case["X"].astype(dx)
    B, Lmax = X.shape
    ld_x, off_x, ld_y, off_y = layout_of(case)
    x = np.full((B, ld_x), x_fill(case), dtype=dx)
    x[:, off_x:off_x + Lmax] = X
    y = np.full((B, ld_y), SENTINEL, dtype=dy) if dy.kind != "u" else np.full((B, ld_y), 256 + SENTINEL, dtype=dy)
    return x, y


_EXPECTED = {}


def expected(case):
    """The model's (B, Lmax) result in the output dtype (in place: the output dtype is still dtypes[1]); computed once per case."""
    if case["name"] not in _EXPECTED:
        _EXPECTED[case["name"]] = _expected(case)
    return _EXPECTED[case["name"]]


def _expected(case):
    dx, dy = case["dtypes"]
    X = case["X"].astype(dx)
    if case["op"] == "encode":
        return WM.encode_batch(X, case["lengths"], case["coef"], case["stage"], case["mu"], dy)
    seg = case["segment"]
    return WM.decode_batch(X, case["lengths"], case["stage"], case["mu"], case["coef"], None if seg >= X.shape[1] else seg, dy)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64, 2: np.int16, 1: np.uint8}[a.dtype.itemsize])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def compare(case, got, want):
    """The texts of what differs between a (B, Lmax) result and the model's.  Bit equality, except where a transcendental of the
    host or the device stands against numpy's: the float mu-law within WM.MULAW_ULPS u |y|, the float inv_mulaw within
    WM.INV_MULAW_ULPS u (1 + mu)^|x| / mu, a class equal unless v lies within CLASS_BAND of an integer (and then one off)."""
    fails = []
    live = np.arange(want.shape[1])[None, :] < np.asarray(WM._live(case["lengths"], *want.shape))[:, None]
    dx, dy = case["dtypes"]
    X = case["X"].astype(dx)
    if got.dtype != want.dtype or got.shape != want.shape:
        return ["dtype or shape"]
    if not same_bits(got[~live], want[~live]):
        fails.append("padding")
    g, w = got[live], want[live]
    if case["op"] == "encode" and case["stage"] == WM.MULAW:
        u = WM.U[np.dtype(np.float64)]
        exact = WM.encode_batch(X, case["lengths"], case["coef"], WM.MULAW, case["mu"], np.float64)[live]
        tol = WM.MULAW_ULPS * u * np.abs(exact) + (np.abs(exact) * WM.U[np.dtype(dy)] if np.dtype(dy) == np.float32 else 0)
        with np.errstate(invalid="ignore"):
            ok = (np.abs(g.astype(np.float64) - exact) <= tol) | (np.isnan(g) & np.isnan(exact)) | (g == exact)
        if not ok.all():
            fails.append("mulaw outside its bound at %d samples" % (~ok).sum())
    elif case["op"] == "encode" and case["stage"] == WM.QUANTIZE:
        P = np.stack([WM.preemphasis(x, case["coef"]) if case["coef"] is not None else x for x in X])
        v = WM.mulaw_v(P, case["mu"])[live]
        near = np.abs(v - np.rint(v)) <= CLASS_BAND
        bad = (g != w) & ~(near & (np.abs(g.astype(np.int64) - w.astype(np.int64)) == 1))
        if bad.any():
            fails.append("classes differ at %d samples" % bad.sum())
    elif case["op"] == "decode" and case["stage"] == WM.MULAW and case["coef"] is None:
        d = X[live].astype(np.float64)
        exact = WM._inv_mulaw64(d, case["mu"])
        tol = WM.INV_MULAW_ULPS * WM.U[np.dtype(np.float64)] * (1.0 + case["mu"]) ** np.abs(d) / case["mu"]
        tol = tol + (np.abs(exact) * WM.U[np.dtype(dy)] if np.dtype(dy) == np.float32 else 0)
        ok = (np.abs(g.astype(np.float64) - exact) <= tol) | (np.isnan(g) & np.isnan(exact))
        if not ok.all():
            fails.append("inv_mulaw outside its bound at %d samples" % (~ok).sum())
    elif not same_bits(g, w):
        fails.append("result: %d samples differ" % (bits(g) != bits(w)).sum())
    return fails


def verdict(case, got):
    """The checks that fail, as texts.  got: (rc, x after the call (B, ld_x), y after it (B, ld_y))."""
    rc, xa, ya = got
    x0, y0 = buffers(case)
    Lmax = case["X"].shape[1]
    ld_x, off_x, ld_y, off_y = layout_of(case)
    if case["mode"] == "refused":
        fails = [] if rc == -1 else ["rc %d, not -1" % rc]
        if not (same_bits(xa, x0) and same_bits(ya, y0)):
            fails.append("a refused call wrote")
        return fails
    if rc != 0:
        return ["rc %d" % rc]
    want = expected(case)
    fails = []
    if case["mode"] == "inplace":
        res = np.ascontiguousarray(xa[:, off_x:off_x + Lmax]).view(want.dtype)
        mask = np.ones(ld_x, dtype=bool)
        mask[off_x:off_x + Lmax] = False
        if not same_bits(np.ascontiguousarray(xa[:, mask]), np.ascontiguousarray(x0[:, mask])):
            fails.append("foreign elements of x")
        if not same_bits(ya, y0):
            fails.append("the unused y was written")
    else:
        res = np.ascontiguousarray(ya[:, off_y:off_y + Lmax])
        if not same_bits(xa, x0):
            fails.append("x changed")
        mask = np.ones(ld_y, dtype=bool)
        mask[off_y:off_y + Lmax] = False
        if not same_bits(np.ascontiguousarray(ya[:, mask]), np.ascontiguousarray(y0[:, mask])):
            fails.append("foreign elements of y")
    return fails + compare(case, res, want)
