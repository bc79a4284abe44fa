"""GPU tests (-m gpu): the four local costs of csrc/dtw_fast.hip at every feature width.

1. Bit-exact costs through forced paths.  A pair with one frame on one side has exactly one warping path, and its reported cost
   is the plain left-to-right float64 sum of the local costs along it (0 + c_0, + c_1, ...), which Python floats reproduce: the
   kernel's `cost` is compared with `==`.  The shapes reach the single cell, `l2_cost2` with two real cells, a pair plus a last
   single cell, and one-cell rows (the pair split by a row boundary: `l2_cost` twice).  Default distance against oracle.dtw.l2
   (sequential, separate multiply and add) at D = 1..130, 200, 257; each _NP kind against the numpy expression it stands for at
   D = 1..128.
2. Path parity at the widths DTW is used with, against the C oracle (default distance) and against the literal restatement of
   fastdtw driven by the same numpy callable (_NP kinds), through the C entry and through DTWAligner.
3. The _NP kinds refuse more than 128 dims at the C entry, touching nothing; DTWAligner evaluates such a `dist` on the host.

No tolerance is introduced: comparisons are exact, or the suite's 1e-12 bar for accumulated DTW costs."""
import warnings
from functools import lru_cache

import numpy as np
import pytest
import torch

from embed import Embedded, embedded, failed
from oracle import dtw as OD
from test_dtw_costs_cpu import L1, L2, NP_DISTS, NP_MAX_DIMS, NP_SCALES, SQL2

pytestmark = pytest.mark.gpu

EINVAL = -1
DEFAULT = -1                                                   # "form" of MLPG_HIP_DIST_L2 in the tables below
KIND = {DEFAULT: 0, L2: 1, L1: 2, SQL2: 3}                     # form -> MLPG_HIP_DIST_*
FORMS = [DEFAULT, L2, L1, SQL2]
FORM_ID = {DEFAULT: "l2", L2: "scaled_l2_np", L1: "scaled_l1_np", SQL2: "scaled_sql2_np"}


def _dist(form):
    return OD.l2 if form == DEFAULT else NP_DISTS[form]


def _scale(form):
    return 1.0 if form == DEFAULT else NP_SCALES[form]


def _tracks(rng, t, D):
    return np.cumsum(rng.randn(t, D), 0) * 0.1


def _pad(pairs):
    N, D = len(pairs), pairs[0][0].shape[1]
    Tx, Ty = max(len(x) for x, _ in pairs), max(len(y) for _, y in pairs)
    X, Y = np.zeros((N, Tx, D)), np.zeros((N, Ty, D))
    for n, (x, y) in enumerate(pairs):
        X[n, :len(x)], Y[n, :len(y)] = x, y
    lenx = np.array([len(x) for x, _ in pairs], dtype=np.int32)
    leny = np.array([len(y) for _, y in pairs], dtype=np.int32)
    return X, Y, lenx, leny


def _run(pairs, radius, form, tie=0):
    from nnmnkwii_amd import _hip
    X, Y, lenx, leny = _pad(pairs)
    out = _hip.fastdtw_l2(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(lenx).cuda(),
                          torch.from_numpy(leny).cuda(), radius, KIND[form], _scale(form), tie)
    return tuple(t.cpu().numpy() for t in out)


# ------------------------------------------------------------------------------------------ 1. forced paths, exact costs

FORCED_SHAPES = [(1, 1), (1, 2), (1, 3), (1, 8), (1, 9), (2, 1), (3, 1), (9, 1)]


def _forced_widths(form):
    return list(range(1, 131)) + [200, 257] if form == DEFAULT else list(range(1, NP_MAX_DIMS + 1))


@pytest.mark.parametrize("form", FORMS, ids=[FORM_ID[f] for f in FORMS])
def test_forced_path_costs_are_bit_exact_at_every_width(form):
    dist = _dist(form)
    bad = []
    for D in _forced_widths(form):
        rng = np.random.RandomState(1000 * (form + 2) + D)
        for s in (1.0, 1e3, 1e-3):
            pairs = [(s * rng.randn(tx, D), s * rng.randn(ty, D)) for tx, ty in FORCED_SHAPES]
            pi, pj, pl, cost = _run(pairs, 1, form)
            for n, (x, y) in enumerate(pairs):
                tx, ty = len(x), len(y)
                cells = [(i, j) for i in range(tx) for j in range(ty)]          # one side has one frame: the only path
                assert pl[n] == tx + ty - 1 == len(cells), (FORM_ID[form], D, s, (tx, ty), pl[n])
                assert list(zip(pi[n, :pl[n]].tolist(), pj[n, :pl[n]].tolist())) == cells, (FORM_ID[form], D, s, (tx, ty))
                # (oracle.dtw.l2 walks its arguments element by element: plain lists spare it numpy's scalar boxing)
                xr, yr = (x.tolist(), y.tolist()) if form == DEFAULT else (x, y)
                want = 0.0
                for i, j in cells:
                    want = want + float(dist(xr[i], yr[j]))
                if float(cost[n]) != want:
                    bad.append((D, s, (tx, ty), float(cost[n]), want))
    assert not bad, "%s: %d costs differ from the reference in their bits; first (D, scale, shape, kernel, reference): %r" % (
        FORM_ID[form], len(bad), bad[:8])


# ------------------------------------------------------------------------------------------------------- 2. path parity

PARITY_WIDTHS = [1, 7, 8, 13, 16, 31, 40, 60, 80, 128, 129, 200, 513]
PARITY_SIZES = [(33, 17), (64, 50), (129, 64), (100, 120)]


@lru_cache(maxsize=None)
def _parity_case(D, radius):
    """The pairs of one width and the C oracle's answer for both tie rules (continuous data: shared by the two tie cases)."""
    rng = np.random.RandomState(7000 + D)
    pairs = [(_tracks(rng, tx, D), _tracks(rng, ty, D)) for tx, ty in PARITY_SIZES]
    ref = {tie: [OD.fastdtw(x, y, radius, tie=tie) for x, y in pairs] for tie in (0, 1)}
    return pairs, ref


def _assert_parity(got, refs, what):
    pi, pj, pl, cost = got
    for n, (d, path) in enumerate(refs):
        path = np.asarray(path)
        assert pl[n] == len(path), what + (n,)
        assert np.array_equal(pi[n, :pl[n]], path[:, 0]) and np.array_equal(pj[n, :pl[n]], path[:, 1]), what + (n,)
        assert abs(cost[n] - d) <= 1e-12 * max(d, 1e-300), what + (n, cost[n], d)


@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("radius", [1, 2])
def test_default_distance_paths_at_real_widths(radius, tie):
    for D in PARITY_WIDTHS:
        pairs, ref = _parity_case(D, radius)
        _assert_parity(_run(pairs, radius, DEFAULT, tie), ref[tie], (D, radius, tie))


NP_PARITY_WIDTHS = [7, 8, 9, 13, 16, 24, 40, 60, 80, 127, 128]
NP_PARITY_SIZES = [(40, 37), (33, 17), (9, 40), (24, 24)]


@pytest.mark.parametrize("form", [L2, L1, SQL2], ids=[FORM_ID[f] for f in (L2, L1, SQL2)])
def test_numpy_order_kinds_paths_against_the_literal_restatement(form):
    for D in NP_PARITY_WIDTHS:
        rng = np.random.RandomState(8000 + 10 * D + form)
        pairs = [(_tracks(rng, tx, D), _tracks(rng, ty, D)) for tx, ty in NP_PARITY_SIZES]
        refs = [OD.fastdtw_py(x, y, 1, NP_DISTS[form]) for x, y in pairs]
        _assert_parity(_run(pairs, 1, form), refs, (FORM_ID[form], D))


def _ragged_batch(rng, N, T, D, dtype=np.float64):
    X, Y = np.zeros((N, T, D), dtype=dtype), np.zeros((N, T - 3, D), dtype=dtype)
    for n in range(N):
        a, b = int(rng.randint(T // 2, T + 1)), int(rng.randint(T // 2, T - 2))
        X[n, :a], Y[n, :b] = _tracks(rng, a, D) + 1.0, _tracks(rng, b, D) + 1.0
    return X, Y


def _assert_aligned(Xa, Ya, X, Y, dist, what):
    assert Xa.shape == Ya.shape and Xa.dtype == X.dtype
    for n in range(X.shape[0]):
        x, y = OD.trim_zeros_frames(X[n]), OD.trim_zeros_frames(Y[n])
        _, path = OD.fastdtw_py(x, y, 1, dist)
        path = np.asarray(path)
        k = len(path)
        assert np.array_equal(Xa[n, :k], x[path[:, 0]]) and np.array_equal(Ya[n, :k], y[path[:, 1]]), what + (n,)
        assert not Xa[n, k:].any() and not Ya[n, k:].any(), what + (n,)
    return True


@pytest.mark.parametrize("D", [13, 60])
def test_aligner_recognition_and_device_kind_agree(D, monkeypatch):
    """DTWAligner(dist=callable) for the three numpy forms and melcd: the callable is recognised, the alignment runs on the device
    kind (the host-evaluated route is closed for this test) and equals the restatement driven by the callable itself."""
    from nnmnkwii_amd import metrics
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner, _resolve_dist

    def closed(*a, **k):
        raise AssertionError("the host-evaluated route was taken")
    monkeypatch.setattr(DTWAligner, "_paths_callable", closed)
    X, Y = _ragged_batch(np.random.RandomState(D), 3, 40, D)
    for name, dist, form in [("l2", NP_DISTS[L2], L2), ("l1", NP_DISTS[L1], L1), ("sql2", NP_DISTS[SQL2], SQL2),
                             ("melcd", metrics.melcd, L2)]:
        kind, c = _resolve_dist(dist)
        assert kind == KIND[form] and abs(c - NP_SCALES[form]) <= 1e-9 * NP_SCALES[form], (name, kind, c)
        Xa, Ya = DTWAligner(dist=dist).transform((X, Y))
        _assert_aligned(Xa, Ya, X, Y, dist, (name, D))


# ----------------------------------------------------------------------------------------- 3. the width limit of the _NP kinds

@pytest.mark.parametrize("form", [L2, L1, SQL2], ids=[FORM_ID[f] for f in (L2, L1, SQL2)])
def test_numpy_order_kinds_refuse_129_dims_and_touch_nothing(form):
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = _hip._stream(dev)
    rng = np.random.RandomState(129 + form)
    shapes = [(12, 9), (5, 14)]

    def call(D):
        pairs = [(_tracks(rng, tx, D), _tracks(rng, ty, D)) for tx, ty in shapes]
        X, Y, lenx, leny = _pad(pairs)
        N, Tx, Ty = len(pairs), X.shape[1], Y.shape[1]
        ins = dict(X=embedded(X), Y=embedded(Y), lenx=embedded(lenx), leny=embedded(leny))
        outs = dict(path_i=Embedded((N, Tx + Ty), np.int32), path_j=Embedded((N, Tx + Ty), np.int32),
                    path_len=Embedded((N,), np.int32), cost=Embedded((N,), np.float64))
        rc = L.mlpg_hip_fastdtw(dev.index, stream, ins["X"].ptr(), ins["Y"].ptr(), ins["lenx"].ptr(), ins["leny"].ptr(), N, Tx, Ty, D,
                                1, KIND[form], NP_SCALES[form], 0, outs["path_i"].ptr(), outs["path_j"].ptr(),
                                outs["path_len"].ptr(), outs["cost"].ptr())
        torch.cuda.synchronize()
        assert not failed(ins, outs)
        return rc, pairs, outs

    rc, _, outs = call(NP_MAX_DIMS + 1)
    assert rc == EINVAL
    assert "128" in L.mlpg_hip_last_error().decode()
    assert all(bool((b.bytes_view() == 0xA5).all()) for b in outs.values())
    # the next valid call on the same stream
    rc, pairs, outs = call(NP_MAX_DIMS)
    assert rc == 0
    got = tuple(outs[k].host() for k in ("path_i", "path_j", "path_len", "cost"))
    _assert_parity(got, [OD.fastdtw_py(x, y, 1, NP_DISTS[form]) for x, y in pairs], (FORM_ID[form], "after the refusal"))


def test_aligner_evaluates_a_recognised_dist_on_the_host_above_128_dims(monkeypatch):
    """metrics.melcd and a city-block callable on 129- and 200-dim features, one pair (host-pointer route) and four (device-tensor
    route): no error, the alignment of the restatement driven by the same callable, and one RuntimeWarning for all of it."""
    from nnmnkwii_amd import metrics
    from nnmnkwii_amd.preprocessing import alignment as A
    monkeypatch.setattr(A, "_warned", set())
    cityblock = NP_DISTS[L1]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for D in (129, 200):
            for N in (1, 4):
                X, Y = _ragged_batch(np.random.RandomState(10 * D + N), N, 40, D)
                for name, dist in (("melcd", metrics.melcd), ("cityblock", cityblock)):
                    assert A._resolve_dist(dist)[0] != 0                        # a recognised, non-default kind
                    aligner = A.DTWAligner(dist=dist)
                    Xa, Ya = aligner.transform((X, Y))
                    _assert_aligned(Xa, Ya, X, Y, dist, (name, D, N))
                    pi, pj, pl = aligner._paths(X, Y)[:3]
                    for n in range(N):
                        x, y = OD.trim_zeros_frames(X[n]), OD.trim_zeros_frames(Y[n])
                        path = np.asarray(OD.fastdtw_py(x, y, 1, dist)[1])
                        assert pl[n] == len(path), (name, D, N, n)
                        assert np.array_equal(pi[n, :pl[n]], path[:, 0]) and np.array_equal(pj[n, :pl[n]], path[:, 1]), (name, D, N, n)
    wide = [w for w in seen if issubclass(w.category, RuntimeWarning)]
    assert len(wide) == 1 and "128" in str(wide[0].message), [str(w.message) for w in seen]
