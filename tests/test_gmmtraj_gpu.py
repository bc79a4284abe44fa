"""Batched trajectory GMM conversion on the device: the kernel of mlpg_hip_gmm_trajectory_stats (csrc/gmm_traj.hip) against the
numpy specification tools/gmmtraj_model.py, and ``MLPG.transform_padded`` / ``transform_batch`` against the reference's goldens
and against the per-utterance route.

Bounds.  Means of the kernel: |got - ref| <= 2 (D + 4) eps S per element, S[d] = |mu_y[m, d]| + sum_k |A[m, d, k]| |x_k - mu_x[m, k]|
(a (D + 1)-term sum in any order, one rounding per product and per difference, on both sides).  Variances: bit-equal cvar[label].
Pad rows: exactly 0 and 1.  Trajectories: rtol 1e-9, atol 1e-9 max|ref|, the bound tests/test_align_gpu.py uses for this path."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gmmtraj_model as GM  # noqa: E402
import gmm_em64 as R  # noqa: E402
from cases import WINDOW_SETS, gmm_joint_data  # noqa: E402
from embed import Embedded, embedded, failed  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
MLPG_KINDS = tuple(range(10))


def _tile():
    from nnmnkwii_amd import _hip
    assert _hip.GMM_TRAJ_ROW_TILE == GM.ROW_TILE
    return _hip.GMM_TRAJ_ROW_TILE


def _counts():
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return [L.mlpg_hip_launch_count(k) for k in range(34)]


def tables(M, D, seed):
    """Random tables with distinct column scales and an asymmetric A: a transposed or permuted tile is an O(1) error."""
    rng = np.random.RandomState(seed)
    scales = rng.permutation(np.linspace(0.5, 3.0, D))
    mu_x = rng.randn(M, D) * scales
    mu_y = rng.randn(M, D) * scales[::-1]
    A = rng.randn(M, D, D) / np.sqrt(D) * scales[None, :, None] / scales[None, None, :]
    cvar = rng.rand(M, D) + 0.1
    return mu_x, mu_y, np.ascontiguousarray(A), cvar


def call(L, dev, x, ld_x, lengths, B, T, D, labels, mu_x, mu_y, A, cvar, M, mean, ld_mean, var, ld_var):
    from nnmnkwii_amd import _hip
    p = lambda b: None if b is None else ctypes.c_void_p(b.ptr())  # noqa: E731
    return L.mlpg_hip_gmm_trajectory_stats(dev.index, _hip._stream(dev), p(x), ld_x, p(lengths), B, T, D, p(labels), p(mu_x), p(mu_y), p(A),
                                           p(cvar), M, p(mean), ld_mean, p(var), ld_var)


def label_patterns(M, rows):
    r = np.arange(rows)
    return {"equal": np.full(rows, M - 1), "cycle": r % M, "runs": (r // 5) % M}


@pytest.mark.parametrize("M", [3, 70])
@pytest.mark.parametrize("D", [1, 3, 4, 6, 15, 16, 17, 60, 72, 128])
def test_kernel_parity_on_guarded_offset_buffers(D, M):
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    tile = _tile()
    mu_x, mu_y, A, cvar = tables(M, D, 100 * D + M)
    ld_x, ld_o = 2 * D, D + 3
    shapes = [(1, n, None) for n in (1, tile - 1, tile, tile + 1, 2 * tile + 3)] + [(5, 37, [37, 0, 1, 36, 20])]
    rng = np.random.RandomState(D + M)
    worst = 0.0
    for off in (0, 1):
        mdl = dict(mu_x=embedded(mu_x, off), mu_y=embedded(mu_y, off), A=embedded(A, off), cvar=embedded(cvar, off))
        for B, T, lengths in shapes:
            rows = B * T
            live = (np.arange(T)[None] < GM.live_frames(lengths, B, T)[:, None]).reshape(rows)
            for pname, lab in label_patterns(M, rows).items():
                lab = lab.astype(np.int32)
                xw = rng.randn(rows, ld_x) * 2.0
                xw[~live] = np.nan                                                # a pad row's x is not read
                lab[~live] = np.where(np.arange((~live).sum()) % 2 == 0, -7, M + 9)   # nor is its label
                bad_row = None
                if rows == 2 * tile + 3 and pname == "cycle":
                    bad_row = tile + 6                                            # one live row with label M: NaN rows, no fault
                    lab[bad_row] = M
                ins = dict(x=embedded(xw, off), labels=embedded(lab, off), **mdl)
                if lengths is not None:
                    ins["lengths"] = embedded(np.asarray(lengths, dtype=np.int32), off)
                mean, var = Embedded((rows, ld_o), np.float64, off), Embedded((rows, ld_o), np.float64, off)
                rc = call(L, dev, ins["x"], ld_x, ins.get("lengths"), B, T, D, ins["labels"], ins["mu_x"], ins["mu_y"], ins["A"], ins["cvar"],
                          M, mean, ld_o, var, ld_o)
                torch.cuda.synchronize()
                assert rc == 0, (off, B, T, pname, rc, L.mlpg_hip_last_error())
                bad = failed(ins, dict(mean=mean, var=var))
                assert not bad, (off, B, T, pname, bad)
                gm, gv = mean.host(), var.host()
                assert (gm[:, D:].view(np.uint64) == FILL).all() and (gv[:, D:].view(np.uint64) == FILL).all(), (off, B, T, pname)
                gm, gv = gm[:, :D], gv[:, :D]
                x = xw[:, :D].reshape(B, T, D)
                rm, rv = GM.stats_padded(x, lengths, lab, mu_x, mu_y, A, cvar)
                rm, rv = rm.reshape(rows, D), rv.reshape(rows, D)
                assert (gm[~live] == 0).all() and (gv[~live] == 1).all(), (off, B, T, pname)
                ok = live.copy()
                if bad_row is not None:
                    ok[bad_row] = False
                    assert np.isnan(gm[bad_row]).all() and np.isnan(gv[bad_row]).all()
                assert gv[ok].tobytes() == cvar[lab[ok]].tobytes() == rv[ok].tobytes(), (off, B, T, pname)
                assert np.isfinite(gm[ok]).all()
                S = GM.error_scale(x.reshape(rows, D)[ok], lab[ok], mu_x, mu_y, A)
                ratio = float((np.abs(gm[ok] - rm[ok]) / (2 * (D + 4) * EPS * S)).max()) if ok.any() else 0.0
                worst = max(worst, ratio)
                assert ratio <= 1.0, (off, B, T, pname, ratio)
    print("D %d M %d: worst mean error %.3f of the bound 2 (D + 4) eps S" % (D, M, worst))


@pytest.mark.parametrize("D,M", [(17, 5), (72, 64)])
def test_rows_do_not_depend_on_their_tile_or_batch(D, M):
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda")
    tile = _tile()
    N = 2 * tile + 3
    mu_x, mu_y, A, cvar = (torch.from_numpy(a).to(dev) for a in tables(M, D, 7 * D + M))
    rng = np.random.RandomState(D)
    x = rng.randn(N, D)
    lab = ((np.arange(N) // 3) % M).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    m0, v0 = _hip.gmm_trajectory_stats(t(x[None]), None, t(lab), mu_x, mu_y, A, cvar)
    m1, v1 = _hip.gmm_trajectory_stats(t(x[None]), None, t(lab), mu_x, mu_y, A, cvar)
    assert torch.equal(m0, m1) and torch.equal(v0, v1)                # two calls: the same bits
    m0, v0 = m0[0].cpu().numpy(), v0[0].cpu().numpy()
    # the same rows in another order
    perm = rng.permutation(N)
    mp, vp = _hip.gmm_trajectory_stats(t(x[perm][None]), None, t(lab[perm]), mu_x, mu_y, A, cvar)
    assert mp[0].cpu().numpy().tobytes() == m0[perm].tobytes() and vp[0].cpu().numpy().tobytes() == v0[perm].tobytes()
    # the same rows cut into three utterances of other lengths, pad rows between them
    T = 50
    lens = np.array([T, N - 2 * T, T], dtype=np.int32)
    assert 0 < lens[1] < T and lens.sum() == N
    xb, lb = np.full((3, T, D), np.nan), np.full((3, T), -5, dtype=np.int32)
    o = 0
    for b, n in enumerate(lens):
        xb[b, :n], lb[b, :n] = x[o:o + n], lab[o:o + n]
        o += n
    mb, vb = _hip.gmm_trajectory_stats(t(xb), t(lens), t(lb), mu_x, mu_y, A, cvar)
    mb, vb = mb.cpu().numpy(), vb.cpu().numpy()
    got_m = np.concatenate([mb[b, :n] for b, n in enumerate(lens)])
    got_v = np.concatenate([vb[b, :n] for b, n in enumerate(lens)])
    assert got_m.tobytes() == m0.tobytes() and got_v.tobytes() == v0.tobytes()
    assert (mb[1, lens[1]:] == 0).all() and (vb[1, lens[1]:] == 1).all()


def test_wrapper_takes_column_slices_and_counts_its_launches():
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda")
    B, T, D, M = 2, 41, 6, 4
    mu_x, mu_y, A, cvar = (torch.from_numpy(a).to(dev) for a in tables(M, D, 1))
    rng = np.random.RandomState(2)
    joint = torch.from_numpy(rng.randn(B, T, 2 * D)).to(dev)          # [x | y]: the source half is a column slice
    lab = torch.from_numpy(rng.randint(M, size=(B, T)).astype(np.int32)).to(dev)
    lens = torch.tensor([T, 17], dtype=torch.int32, device=dev)
    c0 = _counts()
    m0, v0 = _hip.gmm_trajectory_stats(joint[:, :, :D].contiguous(), lens, lab, mu_x, mu_y, A, cvar)
    wide = torch.full((B, T, 2 * D + 5), -3.0, dtype=torch.float64, device=dev)
    m1, v1 = _hip.gmm_trajectory_stats(joint[:, :, :D], lens, lab, mu_x, mu_y, A, cvar, mean=wide[:, :, 2:2 + D], var=wide[:, :, 3 + D:3 + 2 * D])
    _hip.gmm_trajectory_stats(joint[:0, :, :D], lens[:0], lab[:0], mu_x, mu_y, A, cvar)              # B == 0: nothing is launched
    _hip.gmm_trajectory_stats(joint[:, :0, :D], lens, lab[:, :0], mu_x, mu_y, A, cvar)               # Tmax == 0
    torch.cuda.synchronize()
    c1 = _counts()
    assert c1[33] == c0[33] + 2 and [b - a for k, (a, b) in enumerate(zip(c0, c1)) if k != 33] == [0] * 33
    assert torch.equal(m1, m0) and torch.equal(v1, v0) and m1.data_ptr() == wide[:, :, 2:].data_ptr()
    keep = torch.ones(2 * D + 5, dtype=torch.bool, device=dev)
    keep[2:2 + D] = False
    keep[3 + D:3 + 2 * D] = False
    assert (wide[:, :, keep] == -3.0).all()
    with pytest.raises(_hip.HipExtensionError):
        _hip.gmm_trajectory_stats(joint.transpose(0, 1)[:, :, :D], None, lab, mu_x, mu_y, A, cvar)   # no dense (B, Tmax, ld) layout


# ---- end to end --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "align_golden.npz"))


def _gmm_from(golden, key):
    from sklearn.mixture import GaussianMixture
    w = golden[key + "/weights"]
    g = GaussianMixture(n_components=len(w), covariance_type="full")
    g.weights_, g.means_, g.covariances_ = w, golden[key + "/means"], golden[key + "/covariances"]
    return g


def close(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64
    if ref.size == 0:
        return
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("posterior", ["sklearn", "device"])
@pytest.mark.parametrize("wname", ["std2", "std3"])
def test_trajectories_match_the_reference_goldens(golden, wname, posterior):
    from nnmnkwii_amd.baseline.gmm import MLPG
    windows = WINDOW_SETS[wname]
    _, src = gmm_joint_data(wname, 3)
    gmm = _gmm_from(golden, "gmm/%s" % wname)
    for swap in (False, True):
        for diff in (False, True):
            ref = golden["gmm/%s/y-swap%d-diff%d" % (wname, swap, diff)]
            g = MLPG(gmm, windows=windows, swap=swap, diff=diff, posterior=posterior)
            (y,) = g.transform_batch([src])
            close(y, ref)
            yp = g.transform_padded(src[None])
            assert yp.shape == (1,) + ref.shape
            close(yp[0], ref)


_models = {}


def joint_model(D, K, n, seed=3):
    """As tests/test_gmm_em_gpu.py::joint_model, with enough rows for the width (2 D features per component)."""
    from sklearn.mixture import GaussianMixture
    if (D, K) not in _models:
        rng = np.random.RandomState(seed)
        src = R.synthetic(n, D, K, seed=seed)
        tgt = src @ (np.eye(D) + 0.2 * rng.randn(D, D) / np.sqrt(D / 6.0)) + 0.3 * rng.randn(n, D)
        # (n = 600, D = 6 is that test's model exactly; the wide one stops after 20 iterations: any fitted model will do here)
        gm = GaussianMixture(n_components=K, covariance_type="full", random_state=0, max_iter=100 if n == 600 else 20)
        _models[D, K] = gm.fit(np.hstack([src, tgt])), src
    return _models[D, K]


LENS = [40, 1, 119, 0, 64]


@pytest.mark.parametrize("posterior", ["sklearn", "device"])
@pytest.mark.parametrize("D,nw,K,n", [(6, 2, 4, 600), (72, 3, 8, 4000)])
def test_batch_equals_the_per_utterance_route(D, nw, K, n, posterior):
    import warnings
    from nnmnkwii_amd.baseline.gmm import MLPG
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gmm, src = joint_model(D, K, n)
    windows = WINDOW_SETS["std%d" % nw]
    g = MLPG(gmm, windows=windows, posterior=posterior)
    assert g.static_dim == D // nw
    offs = np.concatenate([[0], np.cumsum(LENS)])
    utts = [src[a:b] for a, b in zip(offs[:-1], offs[1:])]
    # precondition: arg-max labels are discontinuous -- every live frame's best and second-best weighted log-probabilities must
    # be clearly apart (scikit-learn, float64, on the host), or the two routes may legitimately pick different mixtures
    wlp = np.sort(g.px._estimate_weighted_log_prob(np.concatenate(utts)), axis=1)
    assert (wlp[:, -1] - wlp[:, -2] > 1e-6).all()
    ref = [g.transform(u) if len(u) else np.zeros((0, g.static_dim)) for u in utts]
    c0 = _counts()
    got = g.transform_batch(utts)
    c1 = _counts()
    assert len(got) == len(utts)
    for y, r in zip(got, ref):
        close(y, r)
    d = [b - a for a, b in zip(c0, c1)]
    assert d[33] == 1 and d[22] == (1 if posterior == "device" else 0) and sum(d[k] for k in MLPG_KINDS) == 1
    assert sum(d[k] for k in MLPG_KINDS + (22, 33)) == (3 if posterior == "device" else 2)
    # a resident float64 tensor: a tensor comes back, pad frames are zero
    Tmax = max(LENS)
    X = np.zeros((len(utts), Tmax, D))
    for i, u in enumerate(utts):
        X[i, :len(u)] = u
    Xd = torch.from_numpy(X).cuda()
    Ld = torch.tensor(LENS, dtype=torch.int32, device="cuda")
    c0 = _counts()
    Y = g.transform_padded(Xd, Ld)
    c1 = _counts()
    d = [b - a for a, b in zip(c0, c1)]
    assert sum(d[k] for k in MLPG_KINDS + (22, 33)) == (3 if posterior == "device" else 2)
    assert torch.is_tensor(Y) and Y.is_cuda and Y.dtype == torch.float64 and Y.shape == (len(utts), Tmax, g.static_dim)
    Yh = Y.cpu().numpy()
    for i, (n_i, r) in enumerate(zip(LENS, ref)):
        close(Yh[i, :n_i], r)
        assert (Yh[i, n_i:] == 0).all()
    # numpy in, numpy out, lengths as a list; float32 input is converted once and computed in float64
    Yn = g.transform_padded(X, LENS)
    assert isinstance(Yn, np.ndarray) and Yn.tobytes() == Yh.tobytes()
    assert g.transform_batch([u[:0] for u in utts[:2]])[0].shape == (0, g.static_dim)


@pytest.mark.parametrize("posterior", ["sklearn", "device"])
def test_static_only_batches_keep_the_inherited_conversion(posterior):
    import warnings
    from nnmnkwii_amd.baseline.gmm import MLPG, MLPGBase
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gmm, src = joint_model(6, 4, 600)
    utts = [src[:40], src[40:41], src[41:160].astype(np.float32)]
    a = MLPG(gmm, windows=[(0, 0, np.array([1.0]))], posterior=posterior).transform_batch(utts)
    b = MLPGBase(gmm, posterior=posterior).transform_batch(utts)
    assert len(a) == len(b) == 3
    for x, y, u in zip(a, b, utts):
        assert x.dtype == y.dtype == u.dtype and x.shape == y.shape == u.shape and x.tobytes() == y.tobytes()
