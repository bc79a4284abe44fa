"""tools/joint_model.py against itself and against the reference (-m "not gpu").

* Its kernel form (tiles, masks, scan, ranks, cap) equals its literal form bit for bit on every case of tests/joint_cases.py.
* It equals tests/golden/joint_ref.npz, the reference's own results (tests/golden/make_golden_joint.py): remove_zeros_frames on
  single matrices bit for bit; the recipe's joint rows bit for bit for float64 inputs; for float32 inputs the same rows are
  selected and every value lies within 2 * taps * 2^-24 * sum_k |c_k x_k| of the reference's (the reference rounds to float32, at
  most 2 * taps - 1 roundings of relative size 2^-24 on terms bounded by sum |c x|; the model's float64 value adds none that
  matters).  Worst ratio seen: 0.991 of 1 * 2^-24 * sum |c x|, that is 0.17 of the bound at three taps."""
import os

import numpy as np
import pytest

import joint_cases as JC
from joint_cases import JM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = JC.cases()
WINDOWS = {0: [], 2: JC.W2, 3: JC.W3}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "joint_ref.npz"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_form_equals_literal_form(case):
    X, Y = JC.typed(case)
    rows, offs = JC.expected(case)
    W, cap = JC.width(case), JC.capacity(case)
    out = np.full((cap, W + case["pad"]), -7.0, dtype=case["dtypes"][2])
    out, offsets, masks, toff = JM.tiled(X, Y, case["len_x"], case["len_y"], case["wins"], case["keep"], case["eps"], case["dtypes"][2], cap, out)
    assert JC.verdict(case, out, offsets) == []
    B, Tmax = X.shape[:2]
    assert len(masks) == len(toff) == B * -(-Tmax // JM.TILE) and 16 * len(masks) == JM.workspace_bytes(B, Tmax)
    assert offsets[-1] == len(rows) and (np.diff(offsets) >= 0).all()


def test_case_list_covers_what_it_names():
    T = JM.TILE
    assert {c["X"].shape[1] for c in CASES} >= {1, T - 1, T, T + 1, 2 * T + 3} and {c["X"].shape[0] for c in CASES} >= {1, 3, 70}
    widths = {c["X"].shape[2] for c in CASES} | {c["Y"].shape[2] for c in CASES if c["Y"] is not None}
    assert widths >= {1, 5, 63, 64, 65, 130} and any(c["Y"] is None for c in CASES)
    assert any(c["len_x"] is None for c in CASES) and any(c["len_x"] is not None and (c["len_x"] != c["len_y"]).any() for c in CASES if c["Y"] is not None)
    lens = set(np.concatenate([c["len_x"] for c in CASES if c["len_x"] is not None]).tolist())
    assert lens >= {0, 1, 2}
    ns = {c["name"]: len(JC.expected(c)[0]) for c in CASES}
    assert ns["all-dropped"] == 0 and ns["all-kept-null-lengths"] == 3 * (T + 1) and ns["static-zero-delta-not"] == 8
    assert ns["threshold-1e-7"] == 3 and ns["threshold-quarter-f32"] == 2
    assert {c["keep"] for c in CASES} == {JM.NONZERO, JM.LIVE} and len({c["dtypes"] for c in CASES}) >= 5
    assert JC.capacity(next(c for c in CASES if c["name"] == "cap-below")) == ns["cap-below"] - 3
    assert JC.capacity(next(c for c in CASES if c["name"] == "cap-zero")) == 0 and any(c["pad"] for c in CASES)
    # a whole empty tile inside a live utterance, and a NaN row that is dropped
    c = next(c for c in CASES if c["name"] == "t131-b3-d65-130-w3-f32")
    masks = JM.tiled(*JC.typed(c), c["len_x"], c["len_y"], c["wins"], c["keep"], c["eps"], c["dtypes"][2])[2]
    assert masks[4] == 0 and masks[3] != 0 and masks[5] != 0
    assert not np.isnan(JC.expected(next(c for c in CASES if c["name"] == "negzero-nan-w0"))[0]).any()
    kept = JC.expected(next(c for c in CASES if c["name"] == "negzero-nan-w0"))[0]
    assert np.signbit(kept[kept == 0]).any()                                  # -0.0 survives in a kept row


def test_remove_zeros_frames_equals_the_reference_bit_for_bit(golden):
    for i in range(int(golden["m"])):
        x, want = golden["mx%d" % i], golden["my%d" % i]
        got = JM.remove_zeros_frames(x)
        assert JC.same_bits(got, want), i


def test_recipe_equals_the_reference(golden):
    worst, seen = 0.0, set()
    for i in range(int(golden["n"])):
        X, Y, start, win = golden["X%d" % i], golden["Y%d" % i], int(golden["start%d" % i]), int(golden["win%d" % i])
        want, lx, ly = golden["XY%d" % i], golden["lx%d" % i], golden["ly%d" % i]
        Xa, Ya = X[:, :, start:], Y[:, :, start:]
        got, _ = JM.literal(Xa, Ya, lx, ly, WINDOWS[win], JM.NONZERO, 1e-7, want.dtype)      # (float64 behind apply_each2d_*, else the input's)
        assert got.shape == want.shape and got.dtype == want.dtype, (i, got.shape, want.shape)
        seen.add((X.dtype.name, win, start))
        if X.dtype == np.float64 or not win:
            assert JC.same_bits(got, want), i
            continue
        absw = [(l, u, np.abs(c)) for l, u, c in WINDOWS[win]]
        scale, _ = JM.literal(np.abs(Xa), np.abs(Ya), lx, ly, absw, JM.LIVE, 0.0, np.float64)            # sum_k |c_k x_k| of every element
        live, _ = JM.literal(Xa, Ya, lx, ly, WINDOWS[win], JM.LIVE, 0.0, np.float64)
        keep = JM.abs_sums(live) > 1e-7
        err, scale = np.abs(got - want), scale[keep]
        assert (err[scale == 0] == 0).all()
        taps = np.tile(np.repeat([l + u + 1 for l, u, _ in WINDOWS[win]], Xa.shape[2]), 2)[None, :]      # of every column
        ratio = np.where(scale > 0, err / (2.0 ** -24 * np.where(scale > 0, scale, 1.0)), 0.0)
        worst = max(worst, ratio.max())
        assert (ratio <= 2 * taps).all(), (i, ratio.max())
    print("float32 recipe against the reference: worst error %.3f of 2^-24 sum |c x| (bound: 2 * taps = 6)" % worst)
    assert seen == {(d, w, s) for d in ("float32", "float64") for w in (0, 2, 3) for s in (0, 1)}


def test_workspace_bytes():
    T = JM.TILE
    assert [JM.workspace_bytes(*a) for a in ((0, 0), (1, 1), (1, T), (1, T + 1), (3, 2 * T + 3), (-1, 4), (4, -1))] == [0, 16, 16, 32, 144, -1, -1]
