"""GPU tests (-m gpu) of the joint rows (csrc/joint_rows.hip): the device result equals tools/joint_model.py bit for
bit (byte views, so NaNs and -0.0 count), `offsets` included -- on the case list of tests/joint_cases.py through the C entries (the
sources column slices of wider rows that hold NaN elsewhere and at or past the lengths, `out` a column slice pre-filled with -7),
exactly one count and one write per call, the same bits on a second call; the golden data of the reference through
``joint_features_batch`` and ``remove_zeros_frames`` (float64 bit for bit, float32 within the bound tests/test_joint_model.py
derives); numpy in gives numpy out; ``out=`` without a synchronisation and ``N > cap``; ``X[:, :, 1:]`` used in place; and the
recipe DTWAligner on CUDA tensors -> joint rows -> fit_gaussian_mixture, with the aligner's refusals for tensors."""
import os

import numpy as np
import pytest
import torch

import joint_cases as JC
from joint_cases import JM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = JC.cases()
TORCH_DT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
WINDOWS = {0: None, 2: JC.W2, 3: JC.W3}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "joint_ref.npz"))


def launches():
    from nnmnkwii_amd import _joint_hip
    return _joint_hip.lib().nnmk_joint_launch_count()


def device_run(case):
    """tests/test_joint_host_cpu.py's host_run on the device: (out (cap, ld_out), offsets, off_out)."""
    from nnmnkwii_amd import _joint_hip as JH
    X, Y = JC.typed(case)
    W, cap = JC.width(case), JC.capacity(case)
    lx, ly = case["len_x"], case["len_y"]
    xs = torch.from_numpy(JC.wide_source(X, lx, 2, 1)).cuda()[:, :, 1:1 + X.shape[2]]
    ys = None if Y is None else torch.from_numpy(JC.wide_source(Y, ly, 3, 2)).cuda()[:, :, 2:2 + Y.shape[2]]
    lxt, lyt = (None if n is None else torch.from_numpy(n).cuda() for n in (lx, ly))
    do = TORCH_DT[np.dtype(case["dtypes"][2])]
    wide = torch.full((cap, W + case["pad"] + 2), -7.0, dtype=do, device="cuda")
    plan, offsets = JH.count(xs, ys, lxt, lyt if Y is not None else None, case["wins"], case["keep"], case["eps"], do)
    plan.write(wide[:, 1:1 + W])
    return wide.cpu().numpy(), offsets.cpu().numpy(), 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_list_through_the_c_entries(case):
    n0 = launches()
    out, offsets, off = device_run(case)
    assert launches() == n0 + 1 + (JC.capacity(case) > 0)                  # one count, one write
    assert JC.verdict(case, out, offsets, off=off) == []
    again = device_run(case)
    assert JC.same_bits(out, again[0]) and JC.same_bits(offsets, again[1])


def test_an_empty_batch_launches_nothing_and_zeroes_the_offsets():
    from nnmnkwii_amd import _joint_hip as JH
    n0 = launches()
    for shape in ((3, 0, 4), (3, 5, 0), (0, 5, 4)):
        x = torch.zeros(shape, dtype=torch.float32, device="cuda")
        offsets = torch.full((shape[0] + 1,), -7, dtype=torch.int64, device="cuda")
        plan, offsets = JH.count(x, None, None, None, [], JH.NONZERO, 1e-7, torch.float32, offsets=offsets)
        plan.write(torch.empty((4, shape[2]), dtype=torch.float32, device="cuda"))
        assert offsets.cpu().tolist() == ([0] * (shape[0] + 1) if shape[0] else [-7])
    assert launches() == n0


def test_golden_matrices_through_remove_zeros_frames(golden):
    from nnmnkwii_amd import preprocessing as P
    for i in range(int(golden["m"])):
        x, want = golden["mx%d" % i], golden["my%d" % i]
        got = P.remove_zeros_frames(x)
        assert isinstance(got, np.ndarray) and JC.same_bits(got, want), i
        t = P.remove_zeros_frames(torch.from_numpy(x).cuda())
        assert t.is_cuda and JC.same_bits(t.cpu().numpy(), want), i
    ints = (np.arange(12).reshape(4, 3) % 4 == 0).astype(np.int64) * 3          # another dtype: computed in float64, cast back
    got = P.remove_zeros_frames(ints)
    assert got.dtype == np.int64 and (got == ints[np.abs(ints).sum(1) > 0]).all()


def test_golden_recipe_through_joint_features_batch(golden):
    from nnmnkwii_amd import preprocessing as P
    worst = 0.0
    for i in range(int(golden["n"])):
        X, Y, start, win = golden["X%d" % i], golden["Y%d" % i], int(golden["start%d" % i]), int(golden["win%d" % i])
        want, lx, ly = golden["XY%d" % i], golden["lx%d" % i], golden["ly%d" % i]
        Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        rows, offsets = P.joint_features_batch(Xt[:, :, start:], Yt[:, :, start:], (lx, ly), WINDOWS[win], dtype=TORCH_DT[want.dtype],
                                               return_offsets=True)
        got = rows.cpu().numpy()
        model, moffs = JM.literal(X[:, :, start:], Y[:, :, start:], lx, ly, JC.W0 if not win else WINDOWS[win], JM.NONZERO, 1e-7, want.dtype)
        assert JC.same_bits(got, model) and JC.same_bits(offsets.cpu().numpy(), moffs), i
        assert got.shape == want.shape, (i, got.shape, want.shape)                      # the same rows are selected
        if X.dtype == np.float64 or not win:
            assert JC.same_bits(got, want), i
            continue
        absw = [(l, u, np.abs(c)) for l, u, c in WINDOWS[win]]
        scale = P.joint_features_batch(np.abs(X[:, :, start:]), np.abs(Y[:, :, start:]), (lx, ly), absw, eps=None)       # numpy in, numpy out
        live = JM.literal(X[:, :, start:], Y[:, :, start:], lx, ly, WINDOWS[win], JM.LIVE, 0.0, np.float64)[0]
        scale = scale[JM.abs_sums(live) > 1e-7]
        taps = np.tile(np.repeat([l + u + 1 for l, u, _ in WINDOWS[win]], X.shape[2] - start), 2)[None, :]
        err = np.abs(got - want)
        assert (err[scale == 0] == 0).all()
        ratio = np.where(scale > 0, err / (2.0 ** -24 * np.where(scale > 0, scale, 1.0)), 0.0)
        worst = max(worst, ratio.max())
        assert (ratio <= 2 * taps).all(), (i, ratio.max())
    print("float32 recipe on the device against the reference: worst error %.3f of 2^-24 sum |c x| (bound: 2 * taps)" % worst)


def test_numpy_in_gives_numpy_out():
    from nnmnkwii_amd import preprocessing as P
    c = next(c for c in CASES if c["name"] == "mix-float32-float32-float32")
    X, Y = JC.typed(c)
    rows, offs = JC.expected(c)
    got, goffs = P.joint_features_batch(X, Y, (c["len_x"], c["len_y"]), c["wins"], dtype=np.float32, return_offsets=True)
    assert isinstance(got, np.ndarray) and isinstance(goffs, np.ndarray) and JC.same_bits(got, rows) and JC.same_bits(goffs, offs)
    c = next(c for c in CASES if c["name"] == "t131-b70-d130-w0-f32")
    got = P.remove_zeros_frames_batch(JC.typed(c)[0], c["len_x"])
    assert isinstance(got, np.ndarray) and JC.same_bits(got, JC.expected(c)[0])
    cpu = P.remove_zeros_frames_batch(torch.from_numpy(JC.typed(c)[0]), torch.from_numpy(c["len_x"]))
    assert torch.is_tensor(cpu) and not cpu.is_cuda and JC.same_bits(cpu.numpy(), JC.expected(c)[0])


def test_out_without_a_synchronisation_and_too_small_a_capacity():
    from nnmnkwii_amd import preprocessing as P
    from nnmnkwii_amd.preprocessing.frames import JointRows
    c = next(c for c in CASES if c["name"] == "cap-above")
    X, Y = (torch.from_numpy(a).cuda() for a in JC.typed(c))
    rows, offs = JC.expected(c)
    N, W = rows.shape
    lens = (torch.from_numpy(c["len_x"]).cuda(), torch.from_numpy(c["len_y"]).cuda())
    out = torch.full((N + 5, W), -7.0, dtype=torch.float64, device="cuda")
    n0 = launches()
    res, offsets = P.joint_features_batch(X, Y, lens, c["wins"], out=out, return_offsets=True)
    assert isinstance(res, JointRows) and res._n is None and res.out is out and launches() == n0 + 2      # N has not been read
    assert len(res) == N and res.rows.data_ptr() == out.data_ptr() and JC.same_bits(res.rows.cpu().numpy(), rows)
    assert bool((out[N:] == -7.0).all().item()) and JC.same_bits(offsets.cpu().numpy(), offs)
    small = torch.full((N - 3, W), -7.0, dtype=torch.float64, device="cuda")
    res = P.joint_features_batch(X, Y, lens, c["wins"], out=small)
    with pytest.raises(ValueError, match="rows past its capacity were not written"):
        res.rows
    assert JC.same_bits(small.cpu().numpy(), rows[:N - 3])                         # the first cap rows are there
    with pytest.raises(ValueError, match=r"out must be a \(cap, %d\)" % W):
        P.joint_features_batch(X, Y, lens, c["wins"], out=torch.empty((N, W), dtype=torch.float32, device="cuda"))


def test_slices_of_wider_tensors_are_used_in_place():
    from nnmnkwii_amd import preprocessing as P
    from nnmnkwii_amd.preprocessing import frames as PF
    rng = np.random.RandomState(5)
    X, Y = JC.frames(rng, 3, 70, 6), JC.frames(rng, 3, 70, 4)
    X[1, 10] = 0.0
    Y[1, 10] = 0.0
    lens = np.array([70, 33, 2], dtype=np.int32)
    Xt, Yt = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    assert PF._source(Xt[:, :, 1:]).data_ptr() == Xt.data_ptr() + 8 and PF._source(Xt[:, :, 1:]).stride() == (420, 6, 1)
    assert PF._source(Xt[:, :, ::2]).is_contiguous()                                 # (stride(2) != 1: a copy)
    got = P.joint_features_batch(Xt[:, :, 1:], Yt[:, :, 1:3], lens, JC.W3)
    want, _ = JM.literal(X[:, :, 1:], Y[:, :, 1:3], lens, lens, JC.W3)
    assert JC.same_bits(got.cpu().numpy(), want)
    got = P.joint_features_batch(Xt[:, :, ::2], None, lens, JC.W2, dtype=torch.float32)
    assert JC.same_bits(got.cpu().numpy(), JM.literal(X[:, :, ::2], None, lens, None, JC.W2, dtype_out=np.float32)[0])


# ---- the recipe ---------------------------------------------------------------------------------------------------------------------

def pairs():
    rng = np.random.RandomState(8)
    lx, ly = (40, 90, 55, 71, 64, 83), (47, 85, 60, 66, 41, 90)
    X, Y = np.zeros((6, 90, 8)), np.zeros((6, 90, 8))
    for n, (a, b) in enumerate(zip(lx, ly)):
        base = np.cumsum(rng.randn(max(a, b), 8), axis=0) * 0.3 + 1.0
        X[n, :a] = base[np.linspace(0, len(base) - 1, a).astype(int)] + 0.05 * rng.randn(a, 8)
        Y[n, :b] = base[np.linspace(0, len(base) - 1, b).astype(int)] + 0.05 * rng.randn(b, 8)
    X[0, 5:7] = 0.0                                       # silence inside both sides of one pair
    Y[0, 6:8] = 0.0
    return X, Y


def test_recipe_aligner_to_joint_rows_to_gmm():
    from nnmnkwii_amd import preprocessing as P, util
    from nnmnkwii_amd.mixture import fit_gaussian_mixture
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner
    X, Y = pairs()
    host = DTWAligner()
    Xa, Ya = host.transform((X, Y))
    assert isinstance(host.path_lengths_, np.ndarray) and host.path_lengths_.dtype == np.int32
    aligner = DTWAligner()
    Xt, Yt = aligner.transform((torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()))
    plen = aligner.path_lengths_
    assert Xt.is_cuda and Yt.is_cuda and plen.is_cuda and plen.dtype == torch.int32 and Xt.dtype == torch.float64
    assert JC.same_bits(Xt.cpu().numpy(), Xa) and JC.same_bits(Yt.cpu().numpy(), Ya) and JC.same_bits(plen.cpu().numpy(), host.path_lengths_)
    # float32 tensors: the dtype of the longer input, as for numpy
    Xa32, Ya32 = DTWAligner().transform((X.astype(np.float32), Y[:, :85]))
    X32, Y32 = aligner.transform((torch.from_numpy(X.astype(np.float32)).cuda(), torch.from_numpy(Y[:, :85].copy()).cuda()))
    assert X32.dtype == torch.float32 and JC.same_bits(X32.cpu().numpy(), Xa32) and JC.same_bits(Y32.cpu().numpy(), Ya32)
    aligner.transform((torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()))
    windows = JC.W3
    n0 = launches()
    rows = P.joint_features_batch(Xt[:, :, 1:], Yt[:, :, 1:], aligner.path_lengths_, windows)
    assert launches() == n0 + 2 and rows.is_cuda and rows.dtype == torch.float64
    Xd = util.apply_each2d_padded(P.delta_features, Xa[:, :, 1:], host.path_lengths_, windows)
    Yd = util.apply_each2d_padded(P.delta_features, Ya[:, :, 1:], host.path_lengths_, windows)
    XY = np.concatenate((Xd, Yd), axis=-1).reshape(-1, 2 * 7 * 3)
    want = XY[np.sum(np.abs(XY), axis=1) > 1e-7]
    assert JC.same_bits(rows.cpu().numpy(), want) and JC.same_bits(P.remove_zeros_frames(XY), want)
    assert len(want) < int(host.path_lengths_.sum()) + 1 and len(want) > 300
    gmm = fit_gaussian_mixture(rows, 2, max_iter=2)
    assert gmm.means_.shape == (2, 42) and np.isfinite(gmm.means_).all()


def test_aligner_refusals_for_tensors():
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner
    X, Y = (torch.from_numpy(a).cuda() for a in pairs())
    with pytest.raises(ValueError, match="called on the host once per window cell"):
        DTWAligner(dist=lambda x, y: float(np.abs(x - y).max())).transform((X, Y))
    wide = torch.ones((2, 4, 129), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="at most 128 feature dims"):
        DTWAligner(dist=lambda x, y: float(np.abs(x - y).sum())).transform((wide, wide))
    with pytest.raises(ValueError, match="devices"):
        DTWAligner(devices=[0]).transform((X, Y))
    with pytest.raises(ValueError, match="CUDA tensors"):
        DTWAligner().transform((X, Y.cpu()))
    with pytest.raises(ValueError, match="CUDA tensors"):
        DTWAligner().transform((X.to(torch.float16), Y.to(torch.float16)))
    Z = X.clone()
    Z[2] = 0.0
    with pytest.raises(ValueError, match="pair 2 has an empty"):
        DTWAligner().transform((Z, Y))
