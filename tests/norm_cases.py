"""Inputs and bounds shared by the tests of corpus normalisation (tests/test_norm_*.py) and by tests/golden/make_golden_norm.py:
the probe's columns, ragged corpora, the shapes that cross every boundary of the kernel, and the recorded error ratios."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import norm_model as NM  # noqa: E402

EPS = NM.EPS
CHUNK, BLOCK = NM.CHUNK_ROWS, NM.BLOCK_ROWS
# The kernel text built for the host (tests/test_norm_host_cpu.py) against the exact truth on HOST_SHAPES, in units of the error
# scales S_mean = eps mean|x| and S_var = eps (var + |mean| sigma): the worst ratios measured there were 0.860 (mean) and 1.964
# (variance); recorded rounded up.  The device's bound is 8 times this (the margin of the gv kernel's bound: another, equally
# valid rounding of the divisions).  A dropped chunk, a wrong count or a wrong merge weight sits at 1e10 and more.
WORST_RATIO = 1.97
BOUND_RATIO = 8 * WORST_RATIO

# (offset, scale) of the probe's columns; None: the 0/1 vuv column; a float alone: a constant column
COLUMNS = [(5.0, 1.0), (-3.0, 0.3), (100.0, 1e-3), (1e4, 1e-6), (1e-3, 1.0), None, 0.1, 1e4 + 0.3, (1e4, 1.0), (5.0, 1e-6),
           (0.0, 1.0), (-3.0, 1e-3)]
CONSTANT = {k: c for k, c in enumerate(COLUMNS) if isinstance(c, float)}


def corpus(seed, lengths, D, dtype=np.float64):
    """A list of (T_i, D) arrays of `dtype`: column d follows COLUMNS[d % 12]."""
    rng = np.random.RandomState(seed)
    out = []
    for T in lengths:
        u = np.empty((T, D))
        for d in range(D):
            c = COLUMNS[d % len(COLUMNS)]
            if c is None:
                u[:, d] = (rng.rand(T) < 0.6).astype(np.float64)
            elif isinstance(c, float):
                u[:, d] = c
            else:
                u[:, d] = c[0] + c[1] * rng.randn(T)
        out.append(u.astype(dtype))
    return out


def padded(seed, lengths, D, dtype=np.float64, Tmax=None, pad_value=np.nan):
    """(X, lengths int32): the corpus as a padded batch whose pad frames hold `pad_value` (NaN: a kernel that reads one shows it)."""
    utts = corpus(seed, [max(int(n), 0) for n in lengths], D, dtype)
    Tmax = max(1, max(lengths)) if Tmax is None else Tmax
    X = np.full((len(utts), Tmax, D), pad_value, dtype=dtype)
    for b, u in enumerate(utts):
        X[b, :len(u)] = u[:Tmax]
    return X, np.asarray(lengths, dtype=np.int32)


# lengths that cover {0, 1, 2} and each of (chunk rows, block rows) +- 1, per B in {1, 2, 3, 5, 17}; Tmax <= ~600
LENGTHS = {
    1: [BLOCK + 1],
    2: [CHUNK - 1, BLOCK],
    3: [0, CHUNK + 1, BLOCK - 1],
    5: [1, 2, CHUNK, 4 * CHUNK + 1, BLOCK + CHUNK + 1],
    17: [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK, 4 * CHUNK, 4 * CHUNK + 1, 100, 255, BLOCK - 1, BLOCK, BLOCK + 1, 530, 7, 64],
}
DIMS = [1, 5, 63, 64, 65, 187]
# the host build runs 256 threads per workgroup: fewer, smaller shapes, the same boundaries
HOST_SHAPES = [(1, 1), (2, 5), (3, 65), (5, 12), (17, 12), (1, 64), (3, 187)]     # (B, D) with LENGTHS[B]


def stats_ok(state, truth, bound=BOUND_RATIO):
    count, mean, var = NM.stats_of(state)[:3]
    return count == truth["count"] and max(NM.ratios(mean, var, truth)) <= bound


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "norm_golden.npz"))
