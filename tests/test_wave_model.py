"""tools/wave_model.py, the executable specification of csrc/wave_codec.hip, against the reference's recorded results
(tests/golden/wave_ref.npz, wave_ref_mulaw.npz; tools/make_golden_wave.py) and against exact arithmetic (-m "not gpu").

  literal   pre-emphasis, the sequential de-emphasis, the decode tables: the reference's bits.  The classes of the whole 16-bit
            grid: the reference's at every point, for both of its dtypes and mu = 255, 256; the three landmarks.  The float
            mu-law within the documented errors of two numpy evaluations.
  tiled     the kernel's de-emphasis (float64 scan, one rounding) against the reference's recorded values within
            E_ref + E_kernel + half an ulp of the output, and against `truth` (exact rational arithmetic) within E_kernel alone
            at tiles of 4, 8, 1024 and L + 5 samples, and with segments, where E_kernel holds the truncation of the zero start.
Every test prints the largest ratio error / bound it saw (pytest -s)."""
import os

import numpy as np
import pytest

import wave_cases as WC
from wave_cases import WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "wave_ref.npz"))


@pytest.fixture(scope="module")
def GM():
    return np.load(os.path.join(ROOT, "tests", "golden", "wave_ref_mulaw.npz"))


def tracks(G):
    for i in range(int(G["n"])):
        yield i, int(G["L"][i]), float(G["coef"][i]), G["x%d" % i], G["pre%d" % i], G["inv%d" % i]


def test_preemphasis_and_the_sequential_recurrence_are_the_reference_bit_for_bit(G):
    n = 0
    for i, L, c, x, pre, inv in tracks(G):
        assert x.dtype == pre.dtype == inv.dtype and len(x) == L
        assert WC.same_bits(WM.preemphasis(x, c), pre), (i, L, c, x.dtype)
        assert WC.same_bits(WM.inv_preemphasis(x, c), inv), (i, L, c, x.dtype)
        assert WC.same_bits(WM.encode(x, c, WM.PLAIN), pre)
        n += 1
    assert n == int(G["n"]) >= 60 and set(G["dt"]) == {"float32", "float64"} and max(G["L"]) == 7000
    assert set(np.round(G["coef"], 3)) == {0.97, 0.85, -0.97, 0.5, 0.999}
    with pytest.raises(TypeError):
        WM.preemphasis(np.arange(5), 0.97)


def test_decode_tables_are_the_reference_bit_for_bit(G):
    for mu in (255, 256, 1023, 4999):
        t = WM.inv_mulaw_table(mu)
        assert t.dtype == np.float32 and WC.same_bits(t, G["table_%d" % mu]), mu
        assert t[0] == -1.0 and t[mu] == 1.0
    assert WC.same_bits(WM.inv_mulaw_quantize(np.array([-4, 0, 128, 256, 300]), 256), G["table_256"][[0, 0, 128, 256, 256]])
    assert WC.same_bits(WM.front(np.arange(257, dtype=np.int16), WM.QUANTIZE, 256), G["table_256"].astype(np.float64))


def test_classes_on_the_whole_16_bit_grid(G):
    k = np.arange(-32768, 32768)
    closest = {}
    for mu in (256, 255):
        assert np.array_equal(G["q_%d_f32" % mu], G["q_%d_f64" % mu])            # the reference's two paths agree on the grid
        for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
            grid = (k / 32768.0).astype(dt)
            got = WM.mulaw_quantize(grid, mu)
            assert got.dtype == np.int64 and np.array_equal(got, G["q_%d_%s" % (mu, tag)]), (mu, tag)
            assert WC.same_bits(WM.encode(grid, None, WM.QUANTIZE, mu, np.int16), G["q_%d_%s" % (mu, tag)])
            for x, want in ((-1.0, 0), (1.0, mu), (0.0, mu // 2), (-0.0, mu // 2)):
                assert WM.mulaw_quantize(np.array([x], dtype=dt), mu)[0] == want == (WM.silence(mu) if x == 0 else want)
        v = WM.mulaw_v(k / 32768.0, mu)
        d = np.abs(v - np.rint(v))
        closest[mu] = d[d > 0].min()
    print("smallest nonzero distance of v from an integer on the grid: %.2e bins (mu 256), %.2e (mu 255); a float64 evaluation "
          "moves v by about 1e-13" % (closest[256], closest[255]))
    assert closest[256] > 1e-6 and closest[255] > 1e-6                           # (so a few ulp of float64 cannot move a class)


def test_float_mulaw_against_the_recorded_values(GM):
    half = np.arange(32769) / 32768.0
    u = 2.0 ** -53
    worst = {}
    for mu in (256, 255):
        want = GM["m_%d_f64" % mu]
        got = WM.mulaw(half, mu)
        bound = (2 * WM.E_NUMPY + 2 * WM.E_NUMPY + 5) * u * np.abs(want)           # two numpy evaluations of the same definition
        assert got.dtype == np.float64 and (np.abs(got - want) <= bound).all()
        assert np.array_equal(WM.mulaw(-half, mu), -got)                          # odd (sign(-0.0) is +0)
        worst["f64 mu %d" % mu] = (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
        # float32 in: the reference evaluates log1p in float32 (its argument rounded: 1 u, log1p: 2 ulp = 4 u, stored rounded: 1 u;
        # ours: float64, rounded once: 1 u, and the float64 terms) -- 8 u of float32
        want32 = GM["m_%d_f32" % mu]
        got32 = WM.mulaw(half.astype(np.float32), mu)
        bound32 = 8 * 2.0 ** -24 * np.abs(want32.astype(np.float64))
        assert got32.dtype == np.float32 and (np.abs(got32.astype(np.float64) - want32) <= bound32).all()
        worst["f32 mu %d" % mu] = (np.abs(got32.astype(np.float64) - want32) / np.maximum(bound32, 1e-300)).max()
    want = GM["im_256_f64"]
    got = WM.inv_mulaw(half, 256)
    bound = (2 * WM.E_NUMPY + 4) * u * (1.0 + 256) ** half / 256
    assert (np.abs(got - want) <= bound).all()
    worst["inv_mulaw"] = (np.abs(got - want) / bound).max()
    rt = WM.inv_mulaw(WM.mulaw(half, 256), 256)
    assert np.abs(rt - half).max() < 1e-12
    print("float mu-law, largest error / bound: " + ", ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    print("kernel bounds: mulaw %d u |y|, inv_mulaw %d u (1 + mu)^|y| / mu" % (WM.MULAW_ULPS, WM.INV_MULAW_ULPS))
    assert WM.MULAW_ULPS == 11 and WM.INV_MULAW_ULPS == 21


def test_tiled_deemphasis_within_the_two_bounds_of_the_reference(G):
    worst = {"float32": 0.0, "float64": 0.0}
    share = {"float32": 0.0, "float64": 0.0}
    for i, L, c, x, pre, inv in tracks(G):
        u = WM.U[x.dtype]
        cd = float(x.dtype.type(c))                                              # the coefficient the reference filters with
        y64, e_kernel = WM.scan(x.astype(np.float64), cd)
        got = WM.decode(x, WM.PLAIN, coef=cd, dtype=x.dtype)
        assert got.dtype == x.dtype and WC.same_bits(got, y64.astype(x.dtype))
        e_ref = WM.ref_bound(inv, c)
        bound = e_ref + e_kernel + u * np.abs(y64)
        err = np.abs(got.astype(np.float64) - inv.astype(np.float64))
        assert (err <= bound).all(), (i, L, c, x.dtype)
        worst[x.dtype.name] = max(worst[x.dtype.name], (err / np.maximum(bound, 1e-300)).max())
        share[x.dtype.name] = max(share[x.dtype.name], (e_kernel / np.maximum(bound, 1e-300)).max())
    print("tiled de-emphasis against the reference, largest error / (E_ref + E_kernel + u |y|): float32 %.3f, float64 %.3f; "
          "largest share of E_kernel in that bound: float32 %.2e, float64 %.3f" % (worst["float32"], worst["float64"], share["float32"], share["float64"]))


@pytest.mark.parametrize("coef", [0.97, 0.85, -0.97, 0.5, 0.999])
def test_tiled_against_truth_at_four_tile_sizes(G, coef):
    worst, worst_u = 0.0, 0.0
    seen = set()
    for i, L, c, x, pre, inv in tracks(G):
        if c != coef or L > 3077 or (L, x.dtype.name) in seen or (L > 1025 and coef not in (0.97, 0.999)):
            continue
        seen.add((L, x.dtype.name))
        v = x.astype(np.float64)
        T = WM.truth(v, coef)
        for tile in (4, 8, 1024, 4 * -(-(L + 5) // 4)):                          # (L + 5 rounded up to whole threads of 4 samples)
            y, E = WM.scan(v, coef, tile=tile)
            d = T.distance(y)
            assert (d <= E).all(), (L, coef, tile, (d / np.maximum(E, 1e-300)).max())
            worst = max(worst, (d / np.maximum(E, 1e-300)).max())
            if tile == 1024:
                worst_u = max(worst_u, d.max() / 2.0 ** -53 / max(np.abs(y).max(), 1e-300))
    assert len(seen) >= 6
    print("coef %g: tiled against truth, largest error / E_kernel %.3f; at the real tile the largest error is %.1f u of max |y|"
          % (coef, worst, worst_u))


def test_segments_against_truth_and_the_plan(G):
    x = next(x for i, L, c, x, pre, inv in tracks(G) if L == 7000).astype(np.float64)
    worst = {}
    for coef, segment, auto in ((0.5, 2048, WM.AUTO_SEGMENT), (0.85, 1024, WM.AUTO_SEGMENT), (0.85, 0, 4096), (-0.97, 2048, WM.AUTO_SEGMENT)):
        S, W, nseg = WM.plan(7000, coef, segment, auto=auto)
        assert nseg == -(-7000 // S) > 1 and W <= S
        y, E = WM.scan(x, coef, 7000, segment, auto=auto)
        d = WM.truth(x, coef).distance(y)
        assert (d <= E).all(), (coef, segment)
        y1, E1 = WM.scan(x, coef)
        assert np.array_equal(y[:S], y1[:S])                                     # segment 0 is the unsplit walk
        if S > W:                                                                # the truncation of the zero start is carried
            assert E[S] >= abs(coef) ** (W + 1) * abs(y[S - W - 1]) > 0
        worst[(coef, S)] = (d / np.maximum(E, 1e-300)).max()
    print("segments against truth, largest error / E_kernel: " + ", ".join("coef %g S %d: %.3f" % (k[0], k[1], v) for k, v in worst.items()))
    assert WM.plan(160000, 0.97, 0) == (16384, 2048, 10) and WM.plan(16384, 0.97, 0) == (16384, 2048, 1)
    assert WM.plan(7000, 0.5, 2048) == (2048, 1024, 4) and WM.plan(7000, 0.97, 7000) == (7000, 2048, 1)
    assert WM.plan(1 << 20, 0.999, 0)[1:] == (56320, 1) and WM.warm_up(1.0) == -1 and WM.warm_up(float("nan")) == -1
    assert WM.warm_up(0.0) == 1024 and WM.warm_up(-0.97) == 2048
    for bad in (dict(coef=0.97, segment=1024), dict(coef=1.0, segment=2048), dict(coef=0.5, segment=1000), dict(coef=0.5, segment=-1)):
        with pytest.raises(ValueError):
            WM.plan(7000, **bad)


def test_fused_chains_against_the_reference(G):
    X, classes, wave = G["chain_x"], G["chain_classes"], G["chain_wave"]
    got = WM.encode_batch(X, None, 0.97, WM.QUANTIZE, 256, np.int16)
    P = np.stack([WM.preemphasis(x, 0.97) for x in X])
    v = WM.mulaw_v(P, 256)
    band = np.abs(v - np.rint(v)) <= 2.0 ** -15
    differ = got != classes
    print("pre-emphasis -> quantise, float32: %d of %d classes differ from the reference's float32 path, all within 2^-15 bins of an "
          "edge: %s; share of samples in that band %.2e (allowed 2e-4)" % (differ.sum(), differ.size, bool((band | ~differ).all()), band.mean()))
    assert (band | ~differ).all() and band.mean() <= 2e-4
    assert (np.abs(got.astype(int) - classes)[differ] == 1).all()
    # decode: the table is exact, the filter within the two bounds
    c32 = float(np.float32(0.97))
    dec = WM.decode_batch(classes, None, WM.QUANTIZE, 256, c32, None, np.float32)
    worst = 0.0
    for b in range(len(classes)):
        y64, e_kernel = WM.scan(WM.front(classes[b], WM.QUANTIZE, 256), c32)
        bound = WM.ref_bound(wave[b], 0.97) + e_kernel + 2.0 ** -24 * np.abs(y64)
        err = np.abs(dec[b].astype(np.float64) - wave[b])
        assert (err <= bound).all()
        worst = max(worst, (err / np.maximum(bound, 1e-300)).max())
    print("classes -> table -> de-emphasis, float32: largest error / bound %.3f" % worst)


def test_batch_padding_rules():
    rng = np.random.RandomState(3)
    X = rng.randn(3, 10).astype(np.float32) * 0.2
    X[0, 4:] = np.nan
    lengths = [4, 100, -2]
    Y = WM.encode_batch(X, lengths, 0.97, WM.QUANTIZE, 255, np.uint8)
    assert Y.dtype == np.uint8 and (Y[0, 4:] == 127).all() and (Y[2] == 127).all() and WM.silence(255) == 127 and WM.silence(256) == 128
    assert np.array_equal(Y[1], WM.mulaw_quantize(WM.preemphasis(X[1], 0.97), 255))
    Z = WM.decode_batch(Y, lengths, WM.QUANTIZE, 255, 0.5, None, np.float64)
    assert (Z[0, 4:] == 0).all() and (Z[2] == 0).all() and Z.dtype == np.float64
    F = WM.encode_batch(X, lengths, None, WM.MULAW, 256)
    assert F.dtype == np.float32 and (F[0, 4:] == 0).all() and WC.same_bits(F[1], WM.mulaw(X[1], 256))
