"""Writes tests/golden/joint_ref.npz: what the reference's ``remove_zeros_frames`` gives on single matrices, and what its
voice-conversion recipe gives on padded batches of pairs:

    Xa, Ya = Xa[:, :, start:], Ya[:, :, start:]
    Xa = apply_each2d_trim(delta_features, Xa, windows); Ya = apply_each2d_trim(delta_features, Ya, windows)
    XY = remove_zeros_frames(np.concatenate((Xa, Ya), axis=-1).reshape(-1, W))

Run on the CPU where the reference's source tree is at hand (its preprocessing/generic.py is loaded from its file and run
unchanged; apply_each2d_trim / apply_each2d_padded of its util package are restated below -- collecting into np.zeros, float64 --
with one guard: an utterance without a live frame is skipped, where np.correlate would raise on the empty array):

    python tests/golden/make_golden_joint.py /path/to/reference

The file holds data only.  ``m`` matrices ``mx<i>`` with their results ``my<i>``; ``n`` compositions with ``X<i>``, ``Y<i>``
(the padded pairs, (B, Tmax, D)), ``start<i>``, ``win<i>`` (0: no windows, 2: static + delta, 3: + delta-delta), ``lx<i>`` /
``ly<i>`` (the trimmed lengths the reference found) and ``XY<i>`` (its joint rows, float64).  np.correlate(..., "same") raises
for a sequence shorter than the window, so utterances have 0 or at least 3 live frames."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOWS = {0: None,
           2: [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))],
           3: [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]}


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_generic", os.path.join(root, "nnmnkwii", "preprocessing", "generic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def apply_each2d_padded(func2d, X, lengths, *args):
    """util/__init__.py:44-66, with the guard for an utterance without a live frame."""
    N, T, D = X.shape
    Y = None
    for idx in range(N):
        if lengths[idx] == 0:
            continue
        y = func2d(X[idx][: lengths[idx]], *args)
        if Y is None:
            Y = np.zeros((N, T, y.shape[1]))
        Y[idx][: len(y)] = y
    return Y if Y is not None else np.zeros((N, T, D * len(args[0])))


def apply_each2d_trim(ref, func2d, X, *args):
    """util/__init__.py:19-41: the lengths are what trim_zeros_frames leaves.  Returns the lengths too."""
    lengths = [len(ref.trim_zeros_frames(X[idx])) for idx in range(len(X))]
    return apply_each2d_padded(func2d, X, lengths, *args), np.array(lengths, dtype=np.int32)


def pairs(rng, dtype):
    """A padded batch of aligned pairs: live lengths 40, 25, 0, 3 and 33 of Tmax = 40, silent (all-zero) frames inside, at the
    start and -- in Y alone -- at the end of one utterance, so that the two trimmed lengths differ."""
    B, Tmax, D = 5, 40, 5
    X, Y = rng.randn(B, Tmax, D), rng.randn(B, Tmax, D)
    for b, n in enumerate((40, 25, 0, 3, 33)):
        X[b, n:] = 0.0
        Y[b, n:] = 0.0
    for b, t in ((0, 0), (0, 1), (0, 17), (0, 39), (1, 10), (1, 11), (1, 12), (1, 13), (4, 5)):
        X[b, t] = 0.0
        Y[b, t] = 0.0
    Y[4, 30:] = 0.0
    return X.astype(dtype), Y.astype(dtype)


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.RandomState(1717)
    out = {}
    m = 0
    for dtype in (np.float64, np.float32):
        for T, D in ((1, 1), (7, 3), (64, 5), (130, 70)):
            x = rng.randn(T, D).astype(dtype)
            x[rng.rand(T) < 0.3] = 0.0
            if T > 4:
                x[2] = 1e-9                          # below eps: a zero frame
                x[3, 0] = -0.0
            out["mx%d" % m], out["my%d" % m] = x, ref.remove_zeros_frames(x.copy())
            m += 1
    out["m"] = np.array(m)
    n = 0
    for dtype in (np.float64, np.float32):
        X, Y = pairs(rng, dtype)
        for win in (0, 2, 3):
            for start in (0, 1):
                Xa, Ya = X[:, :, start:], Y[:, :, start:]
                if win:
                    Xa, lx = apply_each2d_trim(ref, ref.delta_features, Xa, WINDOWS[win])
                    Ya, ly = apply_each2d_trim(ref, ref.delta_features, Ya, WINDOWS[win])
                else:
                    lx = np.array([len(ref.trim_zeros_frames(x)) for x in Xa], dtype=np.int32)
                    ly = np.array([len(ref.trim_zeros_frames(y)) for y in Ya], dtype=np.int32)
                XY = np.concatenate((Xa, Ya), axis=-1)
                XY = ref.remove_zeros_frames(XY.reshape(-1, XY.shape[-1]))
                for k, v in (("X", X), ("Y", Y), ("start", np.array(start)), ("win", np.array(win)), ("lx", lx), ("ly", ly), ("XY", XY)):
                    out["%s%d" % (k, n)] = v
                n += 1
    out["n"] = np.array(n)
    path = os.path.join(HERE, "joint_ref.npz")
    np.savez_compressed(path, **out)
    print("%d matrices, %d compositions, %d bytes" % (m, n, os.path.getsize(path)))


if __name__ == "__main__":
    main()
