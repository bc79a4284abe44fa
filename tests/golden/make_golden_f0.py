"""Writes tests/golden/f0_ref.npz: what the reference's ``preprocessing.interp1d`` (SciPy underneath) gives on about 200 F0
tracks.  Run on the CPU where the reference's source tree and SciPy are at hand (its preprocessing/f0.py is loaded from its file
and run unchanged):

    python tests/golden/make_golden_f0.py /path/to/reference

The file holds data only: ``n`` tracks, ``kinds`` (the kind of each), and per track i ``x<i>`` (the input, float32 or float64,
(T,) or (T, 1)) and ``y<i>`` (the reference's output).  The tracks: T from 2 to 700; both dtypes; all seven kinds; voiced shares
of 5 %, 50 % and 90 % in runs; unvoiced frames written as 0, -0.0 and -1e10; leading and trailing silences; one voiced frame
only, none voiced, all voiced; NaN at frame 0, at the end, inside a gap and inside a voiced run."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("slinear", "linear", "previous", "zero", "next", "nearest", "nearest-up")
LENGTHS = (2, 3, 5, 17, 64, 255, 256, 257, 300, 700)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_f0", os.path.join(root, "nnmnkwii", "preprocessing", "f0.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.interp1d


def track(rng, T, share, unvoiced, lead, trail):
    """A log-F0-like track of T frames: voiced runs (values around 5, positive) and unvoiced runs written as `unvoiced`."""
    x = np.empty(T)
    t, on = 0, rng.rand() < share
    while t < T:
        mean_run = 1 + 12 * (share if on else 1 - share)
        n = 1 + rng.geometric(1.0 / mean_run)
        x[t:t + n] = 4.5 + rng.rand(min(n, T - t)) if on else unvoiced
        t += n
        on = not on
    if lead:
        x[:min(lead, T)] = unvoiced
    if trail:
        x[T - min(trail, T):] = unvoiced
    return x


def cases():
    rng = np.random.RandomState(2015)
    i = 0
    for T in LENGTHS:
        for share in (0.05, 0.5, 0.9):
            for rep in range(5):
                unvoiced = (0.0, -0.0, -1e10)[i % 3]
                lead, trail = ((0, 0), (T // 3, 0), (0, T // 4), (1, 1), (T // 5, T // 5))[rep]
                x = track(rng, T, share, unvoiced, lead, trail)
                if not (x > 0).any() and rep:
                    x[rng.randint(T)] = 5.0                       # (the all-unvoiced tracks come below)
                yield x, KINDS[i % 7], (np.float64, np.float32)[(i // 7) % 2], i % 4 == 3
                i += 1
    for T in (2, 7, 300, 600):
        for j, kind in enumerate(KINDS):
            dt = (np.float32, np.float64)[j % 2]
            one = np.zeros(T)
            one[(0, T - 1, T // 2)[j % 3]] = 5.25                 # one voiced frame only: at 0, at the end, in the middle
            yield one, kind, dt, False
            if j < 3:
                yield np.full(T, (0.0, -0.0, -1e10)[j]), kind, dt, j == 1          # none voiced
                yield 4.5 + rng.rand(T), kind, dt, j == 2                          # all voiced
    for T in (9, 300):
        for j, kind in enumerate(KINDS):
            dt = (np.float64, np.float32)[j % 2]
            x = track(rng, T, 0.5, 0.0, 0, 0)
            x[T // 2 - 2:T // 2 + 2] = 0.0
            x[1], x[T - 2] = 5.5, 4.75
            for where in ("first", "last", "gap", "run"):
                z = x.copy()
                if where == "first":
                    z[0] = np.nan
                elif where == "last":
                    z[-1] = np.nan
                elif where == "gap":
                    z[T // 2] = np.nan
                else:
                    z[1] = np.nan
                    z[2] = 5.0
                if (j + len(where)) % 2 == 0 or T == 9:
                    yield z, kind, dt, False


def main():
    interp1d = load_reference(sys.argv[1])
    out = {}
    kinds = []
    for i, (x, kind, dt, two_d) in enumerate(cases()):
        x = x.astype(dt)
        if two_d:
            x = x[:, None]
        y = interp1d(x.copy(), kind=kind)
        assert y.shape == x.shape and y.dtype == x.dtype, (i, y.shape, y.dtype)
        out["x%d" % i], out["y%d" % i] = x, y
        kinds.append(kind)
    out["n"] = np.array(len(kinds))
    out["kinds"] = np.array(kinds)
    path = os.path.join(HERE, "f0_ref.npz")
    np.savez_compressed(path, **out)
    print("%d tracks, %d frames, %d bytes" % (len(kinds), sum(out["x%d" % i].shape[0] for i in range(len(kinds))), os.path.getsize(path)))


if __name__ == "__main__":
    main()
