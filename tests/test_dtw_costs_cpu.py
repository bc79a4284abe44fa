"""CPU test: the summation order csrc/dtw_fast.hip assumes for the MLPG_HIP_DIST_SCALED_{L2,L1,SQL2}_NP local costs IS numpy's,
at every feature width the kernel accepts.

``np_cost`` below restates the kernel's ``np_cost<F>`` branch for branch in plain Python floats (IEEE double, one rounding per
operation, no contraction): sequential below 8 elements, otherwise eight partial sums combined as
((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus a sequential tail.  numpy sums a contiguous float64 vector of up to 128 elements in exactly
that order; above 128 it splits the vector recursively, which is why the kernel refuses wider frames for these kinds.  A numpy
whose reduction order differs fails HERE, with the width named, instead of as unexplained path mismatches on the GPU.

tests/test_dtw_costs_gpu.py imports ``np_cost``, ``NP_DISTS`` and ``NP_MAX_DIMS`` from this module (no torch, no GPU here)."""
import math

import numpy as np

NP_MAX_DIMS = 128                         # launch_fastdtw refuses the _NP kinds above this many feature dims
L2, L1, SQL2 = 0, 1, 2                    # F of np_cost<F>: MLPG_HIP_DIST_SCALED_L2_NP - 1, ..._L1_NP - 1, ..._SQL2_NP - 1


def _term(form, diff):
    return abs(diff) if form == L1 else diff * diff


def np_cost(form, a, b, scale):
    """csrc/dtw_fast.hip np_cost<form>(a, b, D, scale) in Python floats."""
    a = [float(v) for v in a]
    b = [float(v) for v in b]
    D = len(a)
    if D < 8:
        res = 0.0
        for k in range(D):
            res = res + _term(form, a[k] - b[k])
    else:
        r = [_term(form, a[q] - b[q]) for q in range(8)]
        k = 8
        while k < D - (D % 8):
            for q in range(8):
                r[q] = r[q] + _term(form, a[k + q] - b[k + q])
            k += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while k < D:
            res = res + _term(form, a[k] - b[k])
            k += 1
    return float(scale) * (math.sqrt(res) if form == L2 else res)


def np_dist(form, c):
    """The numpy expression of each form as a ``dist`` callable: what DTWAligner recognises and what the kernel must reproduce."""
    c = float(c)
    if form == L2:
        return lambda x, y: c * math.sqrt(((x - y) * (x - y)).sum(-1))
    if form == L1:
        return lambda x, y: c * np.abs(x - y).sum()
    return lambda x, y: c * ((x - y) ** 2).sum()


# form -> the scale every test of these kinds uses (metrics._logdb_const, spelled out: this module imports nothing of the package)
NP_SCALES = {L2: float(10.0 / np.log(10.0) * np.sqrt(2.0)), L1: 3.0, SQL2: 0.5}
NP_DISTS = {form: np_dist(form, c) for form, c in NP_SCALES.items()}
FORM_NAMES = {L2: "scaled L2", L1: "scaled L1", SQL2: "scaled squared L2"}


def _pairs(D, count, seed):
    rng = np.random.RandomState(seed)
    for q in range(count):
        s = (1.0, 1e3, 1e-3)[q % 3]
        yield s * rng.randn(D), s * rng.randn(D)


def test_restated_summation_order_is_numpys_at_every_accepted_width():
    bad = []
    for D in range(1, NP_MAX_DIMS + 1):
        for x, y in _pairs(D, 20, D):
            for form in (L2, L1, SQL2):
                want = float(NP_DISTS[form](x, y))
                got = np_cost(form, x, y, NP_SCALES[form])
                if got != want:
                    bad.append((FORM_NAMES[form], D, got, want))
    assert not bad, ("numpy %s sums a contiguous float64 vector in another order than csrc/dtw_fast.hip np_cost assumes; first "
                     "mismatches (form, width, restatement, numpy): %r" % (np.__version__, bad[:5]))


def test_logdb_const_is_the_packages():
    from nnmnkwii_amd import metrics
    assert NP_SCALES[L2] == float(metrics._logdb_const)


def test_the_order_differs_above_the_limit():
    """Why the limit exists: beyond 128 elements numpy splits the vector, and the eight-way form no longer gives its bits."""
    differing = set()
    for D in range(NP_MAX_DIMS + 1, 200):
        for x, y in _pairs(D, 20, D):
            if any(np_cost(form, x, y, NP_SCALES[form]) != float(NP_DISTS[form](x, y)) for form in (L2, L1, SQL2)):
                differing.add(D)
    assert differing, "numpy %s sums more than 128 elements like fewer: the kernel's width limit could go" % np.__version__
