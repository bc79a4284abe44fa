"""GPU tests (-m gpu) of continuous F0 (csrc/f0_interp.hip): the device result equals tools/f0_model.py bit for
bit (integer views, so NaNs and -0.0 count) -- on the case list of tests/f0_cases.py through the C entry point (x a column slice
of wider rows that hold NaN elsewhere, the outputs pre-filled with -7), on the golden tracks packed into padded batches through
``interp1d_batch`` and one by one through ``interp1d``, for float32 and float64, dtype mixes and every kind; numpy in gives numpy
out; a column of a 187-wide tensor is filled in place; one launch per call; the same bits on a second call; the padded-batch
glue and the recipe interp1d_batch -> delta_features."""
import os

import numpy as np
import pytest
import torch

import f0_cases as FC
from f0_cases import F0

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = FC.cases()
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


@pytest.fixture(scope="module")
def golden_tracks():
    G = np.load(os.path.join(ROOT, "tests", "golden", "f0_ref.npz"))
    return [(G["x%d" % i], G["y%d" % i], str(G["kinds"][i])) for i in range(int(G["n"]))]


def launches():
    from nnmnkwii_amd import _f0_hip
    return _f0_hip.lib().nnmk_f0_launch_count()


def device_run(case):
    """tests/test_f0_host_cpu.py's host_run on the device: (x after the call, y, vuv, x before it, offsets)."""
    from nnmnkwii_amd import _f0_hip as FH
    dx, dy, dv = (np.dtype(t) for t in case["dtypes"])
    X = case["X"].astype(dx)
    B, Tmax, C = X.shape
    (ld_x, off_x), (ld_y, off_y), (ld_v, off_v) = (C + 2, 1), (C + 3, 2), (C + 1, 0)
    wide = np.full((B, Tmax, ld_x), np.nan, dtype=dx)
    wide[:, :, off_x:off_x + C] = X
    xt = torch.from_numpy(wide).cuda()
    yt = torch.full((B, Tmax, ld_y), FC.SENTINEL, dtype=TORCH_DT[dy], device="cuda")
    vt = torch.full((B, Tmax, ld_v), FC.SENTINEL, dtype=TORCH_DT[dv], device="cuda")
    lengths = None if case["lengths"] is None else torch.from_numpy(case["lengths"]).cuda()
    xs = xt[:, :, off_x:off_x + C]
    mode = case["mode"]
    y = None if mode == "vuv" else (xs if mode in ("inplace", "inplace_y") else yt[:, :, off_y:off_y + C])
    v = None if mode in ("y", "inplace_y") else vt[:, :, off_v:off_v + C]
    FH.interp(xs, lengths, F0.kind_of(case["kind"]), y, v)
    return xt.cpu().numpy(), yt.cpu().numpy(), vt.cpu().numpy(), wide, (off_x, off_y, off_v)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_list_through_the_c_entry(case):
    n0 = launches()
    got = device_run(case)
    assert launches() == n0 + 1
    assert FC.verdict(case, got) == []
    again = device_run(case)
    assert all(FC.same_bits(a, b) for a, b in zip(got[:3], again[:3]))


def test_golden_tracks_packed_into_padded_batches(golden_tracks):
    from nnmnkwii_amd import preprocessing as P
    groups = {}
    for x, _, kind in golden_tracks:
        groups.setdefault((kind, x.dtype), []).append(x.ravel())
    assert len(groups) == 14
    for (kind, dt), tracks in sorted(groups.items(), key=str):
        X, lengths = FC.pack(tracks)
        X = X.astype(dt)
        want_y, want_v = F0.batch(X, lengths, kind)
        n0 = launches()
        y, v = P.interp1d_batch(X, lengths, kind, return_vuv=True)
        assert launches() == n0 + 1
        assert isinstance(y, np.ndarray) and FC.same_bits(y, want_y) and FC.same_bits(v, want_v), (kind, dt)
        y2 = P.interp1d_batch(X[:, :, 0], lengths, kind)
        assert y2.shape == X.shape[:2] and FC.same_bits(y2, want_y[:, :, 0])


def test_interp1d_on_every_golden_track(golden_tracks):
    """numpy in, numpy out, shape and dtype kept; bit-equal to the model, and within the model's bounds of the reference."""
    from nnmnkwii_amd import preprocessing as P
    for x, ref, kind in golden_tracks:
        x0 = x.copy()
        n0 = launches()
        y = P.interp1d(x, kind)
        assert launches() == n0 + 1
        assert isinstance(y, np.ndarray) and y.shape == x.shape and y.dtype == x.dtype and FC.same_bits(x, x0)
        assert FC.same_bits(y, F0.literal(x.ravel(), kind).reshape(x.shape))
        assert np.array_equal(np.isnan(y), np.isnan(ref))
        if kind not in ("slinear", "linear"):
            assert FC.same_bits(y, ref)
        else:
            ok = ~np.isnan(ref)
            assert np.allclose(y[ok], ref[ok], rtol=4e-7 if x.dtype == np.float32 else 4e-15, atol=0)


def test_tensors_in_tensors_out_and_one_frame():
    from nnmnkwii_amd import preprocessing as P
    rng = np.random.RandomState(3)
    for dt in (np.float32, np.float64):
        x = FC.runs(rng, 777).astype(dt)
        for shape in ((777,), (777, 1)):
            xt = torch.from_numpy(x.reshape(shape)).cuda()
            y = P.interp1d(xt, "linear")
            assert torch.is_tensor(y) and y.is_cuda and y.shape == xt.shape and y.dtype == xt.dtype
            assert FC.same_bits(y.cpu().numpy().ravel(), F0.literal(x, "linear"))
            assert FC.same_bits(xt.cpu().numpy().ravel(), x)
        strided = torch.from_numpy(np.stack([x, x], 1)).cuda()[:, 1]                 # a column of a (T, 2) tensor
        assert FC.same_bits(P.interp1d(strided).cpu().numpy(), F0.literal(x))
    for v in (5.0, 0.0, -1e10, np.nan):
        one = np.array([v])
        assert FC.same_bits(P.interp1d(one), one)                                    # (the reference raises for the voiced one)
    assert P.interp1d(np.zeros(0)).shape == (0,) and P.interp1d_batch(np.zeros((0, 4, 2))).shape == (0, 4, 2)
    ints = np.array([0, 4, 0, 0, 8, 0])
    assert np.array_equal(P.interp1d(ints), [4, 4, 5, 6, 8, 8]) and P.interp1d(ints).dtype == ints.dtype


def test_a_column_of_a_187_wide_tensor_in_place():
    from nnmnkwii_amd import preprocessing as P
    rng = np.random.RandomState(4)
    B, Tmax, W, LF0, VUV = 4, 600, 187, 180, 181
    lengths = np.array([600, 513, 0, 255])
    X = rng.randn(B, Tmax, W).astype(np.float32)
    for b in range(B):
        X[b, :, LF0] = FC.runs(rng, Tmax, 0.6)
    Xt = torch.from_numpy(X).cuda()
    want_y, want_v = F0.batch(X[:, :, LF0], lengths)
    n0 = launches()
    y, v = P.interp1d_batch(Xt[:, :, LF0:LF0 + 1], lengths, out=Xt[:, :, LF0:LF0 + 1], vuv=Xt[:, :, VUV:VUV + 1])
    assert launches() == n0 + 1
    assert y.data_ptr() == Xt[:, :, LF0:].data_ptr() and v.data_ptr() == Xt[:, :, VUV:].data_ptr()
    got = Xt.cpu().numpy()
    assert FC.same_bits(got[:, :, LF0], want_y) and FC.same_bits(got[:, :, VUV], want_v)
    rest = np.ones(W, dtype=bool)
    rest[[LF0, VUV]] = False
    assert FC.same_bits(np.ascontiguousarray(got[:, :, rest]), np.ascontiguousarray(X[:, :, rest]))
    # the (B, Tmax) form of the same columns, float64 flag out of a float32 track, no lengths
    Xt = torch.from_numpy(X).cuda()
    flag = torch.full((B, Tmax), -7.0, dtype=torch.float64, device="cuda")
    y, v = P.interp1d_batch(Xt[:, :, LF0], kind="nearest", out=Xt[:, :, LF0], vuv=flag)
    want_y, want_v = F0.batch(X[:, :, LF0], None, "nearest", vuv_dtype=np.float64)
    assert v is flag and FC.same_bits(Xt[:, :, LF0].cpu().numpy(), want_y) and FC.same_bits(flag.cpu().numpy(), want_v)
    y = P.interp1d_batch(Xt[:, :, VUV:VUV + 2], torch.tensor([3, 700, 2, 1], device="cuda"), "next")
    assert y.is_contiguous() and FC.same_bits(y.cpu().numpy(), F0.batch(X[:, :, VUV:VUV + 2], [3, 700, 2, 1], "next")[0])


def test_padded_batch_glue_dispatches_to_the_batch_form():
    from nnmnkwii_amd import preprocessing as P, util
    rng = np.random.RandomState(5)
    lengths = np.array([300, 120, 1, 257])
    X, _ = FC.pack([FC.runs(rng, n, 0.4, unvoiced=(0.0,)) for n in lengths])
    X = np.nan_to_num(X)                                                            # zero padding, as the reference's batches
    for kind in ("slinear", "nearest"):
        want = F0.batch(X, lengths, kind)[0]
        n0 = launches()
        got = util.apply_each2d_padded(P.interp1d, X, lengths, kind)
        assert launches() == n0 + 1
        assert got.dtype == np.float64 and FC.same_bits(got, want) and FC.same_bits(got, P.interp1d_batch(X, lengths, kind))
        assert FC.same_bits(util.apply_each2d_padded(P.interp1d, X, lengths, kind=kind), want)
    for b, n in enumerate(lengths):                                                 # trailing zero frames are trimmed: end on a voiced one
        X[b, n - 1] = 5.0
    assert FC.same_bits(util.apply_each2d_trim(P.interp1d, X), F0.batch(X, lengths)[0])
    with pytest.raises(RuntimeError, match="1d array is only supported"):            # two columns: the per-utterance path, as the reference
        util.apply_each2d_padded(P.interp1d, np.concatenate([X, X], 2), lengths)


def test_recipe_interp1d_batch_then_delta_features():
    from nnmnkwii_amd import preprocessing as P
    rng = np.random.RandomState(6)
    lengths = np.array([400, 256, 31])
    X, _ = FC.pack([FC.runs(rng, n) for n in lengths], 2, rng)
    X = X.astype(np.float32)
    windows = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]
    Xt = torch.from_numpy(X).cuda()
    filled = P.interp1d_batch(Xt, lengths)
    want = torch.from_numpy(F0.batch(X, lengths)[0]).cuda()
    assert torch.equal(filled, want)
    got, ref = P.delta_features(filled, windows), P.delta_features(want, windows)
    assert got.shape == (3, 400, 6) and FC.same_bits(got.cpu().numpy(), ref.cpu().numpy())
