"""Writes tests/golden/wave_ref.npz and tests/golden/wave_ref_mulaw.npz: what the reference's mulaw, inv_mulaw, mulaw_quantize,
inv_mulaw_quantize, preemphasis and inv_preemphasis (numpy and SciPy underneath) give.  Run on the CPU where the reference's
source tree, SciPy and scikit-learn are at hand (its preprocessing/generic.py is loaded from its file and run unchanged):

    python tools/make_golden_wave.py /path/to/reference

Both files hold data only.  wave_ref.npz:
  q_<mu>_<f32|f64>      int16 (65536): mulaw_quantize of the 16-bit grid k / 32768, k = -32768 .. 32767, in that dtype
  table_<mu>            float32 (mu + 1): inv_mulaw_quantize(arange(mu + 1)), mu = 255, 256, 1023, 4999
  n, L, coef, dt        the emphasis tracks: per track i its length, coefficient and dtype name, and
  x<i>, pre<i>, inv<i>  the seeded input and preemphasis / inv_preemphasis of it (lengths 1 .. 7000; coef 0.97, 0.85, -0.97, 0.5,
                        0.999; float32 and float64 -- the longest tracks in float32 only, for the file's size)
  chain_x               float32 (2, 8192): a seeded waveform;  chain_classes int16: mulaw_quantize(preemphasis(row, 0.97), 256),
                        the reference's float32 path;  chain_wave float32: inv_preemphasis(inv_mulaw_quantize(classes, 256), 0.97)
wave_ref_mulaw.npz (the reference is odd in x bit for bit -- asserted here -- so the non-negative half of the grid is kept):
  m_<mu>_f64            float64 (32769): mulaw of k / 32768, k = 0 .. 32768, float64 in
  m_<mu>_f32            float32 (32769): the same for float32 in, the reference's float64 result rounded to float32 (its float32
                        logarithm carries no more)
  im_256_f64            float64 (32769): inv_mulaw of k / 32768 at mu = 256, float64 in"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
COEFS = (0.97, 0.85, -0.97, 0.5, 0.999)
SHORT = (1, 2, 3, 5, 1023, 1025)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_generic", os.path.join(root, "nnmnkwii", "preprocessing", "generic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def waveform(rng, L):
    """A speech-like waveform in (-1, 1): a random walk and noise under a slow envelope."""
    x = np.cumsum(rng.randn(L)) * 0.02 + rng.randn(L) * 0.06
    return np.clip(x * np.abs(np.sin(np.arange(L) / 211.0)) * 0.9 / max(np.abs(x).max(), 1e-3), -0.999, 0.999)


def tracks():
    """(L, coef, dtype) of every emphasis track."""
    for dt in (np.float32, np.float64):
        for L in SHORT:
            for c in COEFS:
                yield L, c, dt
        for c in (0.999, -0.97):
            yield (3077 if dt == np.float32 else 2049), c, dt
    yield 7000, 0.97, np.float32
    yield 3077, 0.97, np.float64


def main():
    G = load_reference(sys.argv[1])
    out, mul = {}, {}
    k = np.arange(-32768, 32768)
    for mu in (256, 255):
        for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
            grid = (k / 32768.0).astype(dt)
            assert np.array_equal(grid.astype(np.float64) * 32768.0, k)
            q = G.mulaw_quantize(grid, mu)
            assert q.min() >= 0 and q.max() <= mu
            out["q_%d_%s" % (mu, tag)] = q.astype(np.int16)
            half = (np.arange(32769) / 32768.0).astype(dt)
            m = np.asarray(G.mulaw(half, mu), dtype=np.float64)
            assert np.array_equal(np.asarray(G.mulaw(-half, mu), dtype=np.float64), -m)          # odd, bit for bit
            mul["m_%d_%s" % (mu, tag)] = m.astype(dt)
    half = np.arange(32769) / 32768.0
    im = G.inv_mulaw(half, 256)
    assert np.array_equal(G.inv_mulaw(-half, 256), -im)
    mul["im_256_f64"] = im
    for mu in (255, 256, 1023, 4999):
        t = G.inv_mulaw_quantize(np.arange(mu + 1), mu)
        assert t.dtype == np.float32, t.dtype
        out["table_%d" % mu] = t
    rng = np.random.RandomState(2016)
    inputs = {}
    Ls, cs, dts = [], [], []
    for i, (L, c, dt) in enumerate(tracks()):
        if (L, dt) not in inputs:
            inputs[(L, dt)] = waveform(rng, L).astype(dt)
        x = inputs[(L, dt)]
        pre, inv = G.preemphasis(x.copy(), c), G.inv_preemphasis(x.copy(), c)
        assert pre.dtype == dt and inv.dtype == dt and pre.shape == x.shape == inv.shape
        out["x%d" % i], out["pre%d" % i], out["inv%d" % i] = x, pre, inv
        Ls.append(L)
        cs.append(c)
        dts.append(np.dtype(dt).name)
    out["n"], out["L"], out["coef"], out["dt"] = np.array(len(Ls)), np.array(Ls), np.array(cs), np.array(dts)
    X = np.stack([waveform(rng, 8192), waveform(rng, 8192) * 0.3]).astype(np.float32)
    classes = np.stack([G.mulaw_quantize(G.preemphasis(x, 0.97), 256) for x in X])
    assert classes.min() >= 0 and classes.max() <= 256
    wave = np.stack([G.inv_preemphasis(G.inv_mulaw_quantize(c, 256), 0.97) for c in classes])
    assert wave.dtype == np.float32
    out["chain_x"], out["chain_classes"], out["chain_wave"] = X, classes.astype(np.int16), wave
    for name, d in (("wave_ref.npz", out), ("wave_ref_mulaw.npz", mul)):
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **d)
        print("%s: %d arrays, %d bytes" % (name, len(d), os.path.getsize(path)))
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
