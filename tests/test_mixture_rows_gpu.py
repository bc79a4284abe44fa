"""The k-means and EM kernels (csrc/kmeans.hip, csrc/gmm_em.hip) at the row counts of the aligner's joint matrix, where the launch
geometry differs from every smaller test: more than one 64-row tile per k-means slice (N > 65536; three at N = 131137), trailing
slices without rows (N = 65601), more than one partial per thread in the mean's finalisation (N > 16384), the caps of the M-step's
slice counts.  Single steps against tests/kmeans64.py and tests/gmm_em64.py with the inputs, checks and bounds of
tests/test_kmeans_gpu.py::test_single_steps and tests/test_gmm_em_gpu.py: 1e-10 of the reference array's maximum, counts and labels
exact, no row left out of the label comparison.

Every call goes to the C entry point with buffers of tests/embed.py: the inputs at offset 0 and again one double in (8 mod 16),
unchanged afterwards; every output between guard bands; the workspace exactly the bytes the library's formula gives (the seed step:
exactly the first region include/mlpg_hip.h documents), 8-byte aligned and not more.  All guards must be intact, and the results at
the two offsets equal bit for bit (the header: "two calls on the same inputs give the same bits").  The small shapes of the two
existing single-step tests run the same way once, for the LDS-maximal kernels."""
import functools
import warnings

import numpy as np
import pytest
import torch

import gmm_em64 as G
import kmeans64 as R
from embed import Embedded, Workspace, embedded, ptr
from test_gmm_em_gpu import EPS, check, check_labels, model, rows

pytestmark = pytest.mark.gpu

OFFSET_BYTES = (0, 8)
KMEANS_ROWS = [(65537, 1, 1), (65601, 2, 3), (65601, 17, 16), (66000, 128, 64), (131137, 50, 16)]
GMM_ROWS = [(16449, 33, 64), (65601, 2, 3), (65601, 17, 16), (65601, 50, 16)]
SMALL = [(N, F, K) for F, K in ((1, 1), (17, 16), (128, 64)) for N in (1, 65, 1025)]


def _call():
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda", torch.cuda.current_device())
    return _hip.lib(), dev.index, _hip._stream(dev)


def _in(a, off_bytes, dtype=None):
    dt = np.dtype(a.dtype if dtype is None else dtype)
    return embedded(a, off_bytes // dt.itemsize, dtype=dt)


def _out(shape, dtype, off_bytes):
    return Embedded(shape, dtype, off_bytes // np.dtype(dtype).itemsize, 0xA5)


def _settle(bufs_in, bufs_out, works):
    torch.cuda.synchronize()
    for name, b in bufs_in.items():
        assert b.unchanged() and b.guards_ok(), "input %s" % name
    for name, b in bufs_out.items():
        assert b.guards_ok(), "guard of output %s" % name
    for name, w in works.items():
        assert w.guards_ok(), "guard of workspace %s" % name


def _same_bits(a, b, what):
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), "%s: %s differs between the offsets" % (what, name)


# ------------------------------------------------------------------------------------------------------------------ k-means

def _r256(b):
    return -(-b // 256) * 256


@functools.lru_cache(maxsize=None)
def _kmeans_case(N, F, K):
    C = 1 + (N + F + K) % 8
    case = R.step_case(N, F, K, C, 1000 * F + 10 * K + N)
    Xc = case["X"] - case["shift"]
    seeds = [R.seed_step(Xc, case["cand"], closest) for closest in (None, case["closest"])]
    return case, seeds, R.step_expected(case)


def _kmeans_once(N, F, K, off):
    """Both seed steps, the Lloyd step and the step without the centre update at one byte offset; every result as host arrays."""
    L, dev, stream = _call()
    case, _, _ = _kmeans_case(N, F, K)
    C = len(case["cand"])
    ins = dict(X=_in(case["X"], off), shift=_in(case["shift"], off), cand=_in(case["cand"], off, np.int32),
               closest=_in(case["closest"], off), centers=_in(case["centers"], off), prev=_in(case["prev"], off, np.int32))
    S = min(max(-(-N // 64), 1), 1024)
    seed_bytes = _r256(64 * S)
    full_bytes = int(L.mlpg_hip_kmeans_workspace_bytes(N, F, K))
    assert full_bytes == seed_bytes + _r256(8 * S * K * (F + 1)) + 2 * _r256(8 * S) + _r256(8 * K)
    works = dict(seed=Workspace(seed_bytes, 8), full=Workspace(full_bytes, 8))
    got = {}
    outs = {}
    for tag, closest in (("0", None), ("1", ins["closest"])):
        d, pots = _out((C, N), np.float64, off), _out((C,), np.float64, off)
        outs["d" + tag], outs["pots" + tag] = d, pots
        rc = L.mlpg_hip_kmeans_seed_step(dev, stream, ins["X"].ptr(), ins["shift"].ptr(), N, F, ins["cand"].ptr(), C, ptr(closest),
                                         d.ptr(), pots.ptr(), works["seed"].ptr(), seed_bytes)
        assert rc == 0, rc
    o = dict(labels=_out((N,), np.int32, off), min_dist=_out((N,), np.float64, off), sums=_out((K, F), np.float64, off),
             counts=_out((K,), np.float64, off), centers=_out((K, F), np.float64, off), stats=_out((4,), np.int64, off))
    rc = L.mlpg_hip_kmeans_lloyd_step(dev, stream, ins["X"].ptr(), ins["shift"].ptr(), ins["centers"].ptr(), ins["prev"].ptr(), N, F, K,
                                      1, o["labels"].ptr(), o["min_dist"].ptr(), o["sums"].ptr(), o["counts"].ptr(), o["centers"].ptr(),
                                      o["stats"].ptr(), works["full"].ptr(), full_bytes)
    assert rc == 0, rc
    outs.update(o)
    # the centre update turned off, from the labels just found: centers_out and min_dist are NULL
    o2 = dict(labels2=_out((N,), np.int32, off), sums2=_out((K, F), np.float64, off), counts2=_out((K,), np.float64, off),
              stats2=_out((4,), np.int64, off))
    rc = L.mlpg_hip_kmeans_lloyd_step(dev, stream, ins["X"].ptr(), ins["shift"].ptr(), ins["centers"].ptr(), o["labels"].ptr(), N, F, K,
                                      0, o2["labels2"].ptr(), None, o2["sums2"].ptr(), o2["counts2"].ptr(), None,
                                      o2["stats2"].ptr(), works["full"].ptr(), full_bytes)
    assert rc == 0, rc
    outs.update(o2)
    _settle(ins, outs, works)
    for name, b in outs.items():
        got[name] = b.host()
    return got


def _kmeans_check(N, F, K, got):
    case, seeds, ref = _kmeans_case(N, F, K)
    for tag, (d_r, p_r) in zip("01", seeds):
        e = R.dist(got["d" + tag], d_r), R.dist(got["pots" + tag], p_r)
        print("N %d F %d K %d seed step %s: d %.2e pots %.2e" % (N, F, K, tag, *e))
        assert max(e) <= 1e-10, (tag, e)
    fl = got["stats"].view(np.float64)
    move, inertia, changed, empty = float(fl[0]), float(fl[1]), int(got["stats"][2]), int(got["stats"][3])
    R.check_step(case, ref, dict(labels=got["labels"], min_dist=got["min_dist"], sums=got["sums"], counts=got["counts"],
                                 centers=got["centers"], shift=move, inertia=inertia, changed=changed, empty=empty))
    fl2 = got["stats2"].view(np.float64)
    assert np.array_equal(got["labels2"], got["labels"]) and got["sums2"].tobytes() == got["sums"].tobytes()
    assert got["counts2"].tobytes() == got["counts"].tobytes()
    assert int(got["stats2"][2]) == 0 and fl2[0] == 0.0 and int(got["stats2"][3]) == ref["empty"]
    assert fl2[1:2].tobytes() == fl[1:2].tobytes()                       # the same inertia bits


def _kmeans_test(N, F, K):
    a = _kmeans_once(N, F, K, OFFSET_BYTES[0])
    _kmeans_check(N, F, K, a)
    b = _kmeans_once(N, F, K, OFFSET_BYTES[1])
    _same_bits(a, b, "k-means N %d F %d K %d" % (N, F, K))


@pytest.mark.parametrize("N,F,K", KMEANS_ROWS)
def test_kmeans_steps_at_aligner_row_counts(N, F, K):
    _kmeans_test(N, F, K)


@pytest.mark.parametrize("N,F,K", SMALL)
def test_kmeans_small_shapes_on_exact_workspaces(N, F, K):
    _kmeans_test(N, F, K)


# ---------------------------------------------------------------------------------------------------------------------- GMM

@functools.lru_cache(maxsize=None)
def _gmm_case(N, F, K):
    weights, means, cov, U, log_det, cond = model(F, K)
    Xe = rows(N, F, K, means, cov, N)
    Xm = rows(N, F, K, means, cov, N + 1)
    resp = np.random.RandomState(N + K).dirichlet(np.full(K, 0.7), size=N)
    return dict(weights=weights, means=means, cov=cov, U=U, log_det=log_det, Xe=Xe, Xm=Xm, resp=resp), cond, \
        G.e_step(Xe, weights, means, U, log_det), G.m_step(Xm, resp, 1e-6)


def _gmm_once(N, F, K, off):
    L, dev, stream = _call()
    case = _gmm_case(N, F, K)[0]
    ins = {name: _in(a, off) for name, a in case.items()}
    nbytes = int(L.mlpg_hip_gmm_workspace_bytes(N, F, K))
    assert nbytes > 0
    works = dict(estep=Workspace(nbytes, 8), mstep=Workspace(nbytes, 8))
    outs = dict(resp=_out((N, K), np.float64, off), log_prob_norm=_out((N,), np.float64, off), labels=_out((N,), np.int32, off),
                mean_log_prob=_out((1,), np.float64, off), weights=_out((K,), np.float64, off), means=_out((K, F), np.float64, off),
                covariances=_out((K, F, F), np.float64, off), prec_chol=_out((K, F, F), np.float64, off),
                log_det=_out((K,), np.float64, off), status=_out((K,), np.int32, off))
    rc = L.mlpg_hip_gmm_estep(dev, stream, ins["Xe"].ptr(), ins["weights"].ptr(), ins["means"].ptr(), ins["U"].ptr(),
                              ins["log_det"].ptr(), N, F, K, outs["resp"].ptr(), outs["log_prob_norm"].ptr(), outs["labels"].ptr(),
                              outs["mean_log_prob"].ptr(), works["estep"].ptr(), nbytes)
    assert rc == 0, rc
    rc = L.mlpg_hip_gmm_mstep(dev, stream, ins["Xm"].ptr(), ins["resp"].ptr(), N, F, K, 1e-6, outs["weights"].ptr(),
                              outs["means"].ptr(), outs["covariances"].ptr(), works["mstep"].ptr(), nbytes)
    assert rc == 0, rc
    # the wrapper hands the kernel zeroed factors (it writes the upper triangle and the diagonal): do the same
    outs["prec_chol"].payload().zero_()
    outs["log_det"].payload().zero_()
    rc = L.mlpg_hip_gmm_precisions(dev, stream, ins["cov"].ptr(), F, K, outs["prec_chol"].ptr(), outs["log_det"].ptr(),
                                   outs["status"].ptr())
    assert rc == 0, rc
    _settle(ins, outs, works)
    return {name: b.host() for name, b in outs.items()}


def _gmm_check(N, F, K, got):
    case, cond, (resp_r, lpn_r, _, mean_r), (w_r, mu_r, cov_r) = _gmm_case(N, F, K)
    tag = "F=%d K=%d N=%d " % (F, K, N)
    check(tag + "resp", got["resp"], resp_r)
    check(tag + "log_prob_norm", got["log_prob_norm"], lpn_r)
    check(tag + "mean", got["mean_log_prob"][0], mean_r)
    check_labels(got["labels"], resp_r)
    check(tag + "weights", got["weights"], w_r)
    check(tag + "means", got["means"], mu_r)
    check(tag + "covariances", got["covariances"], cov_r)
    assert np.array_equal(got["covariances"], got["covariances"].transpose(0, 2, 1))
    assert not got["status"].any()
    check(tag + "U", got["prec_chol"], case["U"], max(1e-10, 8 * EPS * cond))
    check(tag + "log_det", got["log_det"], case["log_det"])
    assert np.array_equal(got["prec_chol"], np.triu(got["prec_chol"]))


def _gmm_test(N, F, K):
    a = _gmm_once(N, F, K, OFFSET_BYTES[0])
    _gmm_check(N, F, K, a)
    b = _gmm_once(N, F, K, OFFSET_BYTES[1])
    _same_bits(a, b, "GMM N %d F %d K %d" % (N, F, K))


@pytest.mark.parametrize("N,F,K", GMM_ROWS)
def test_gmm_steps_at_aligner_row_counts(N, F, K):
    _gmm_test(N, F, K)


@pytest.mark.parametrize("N,F,K", SMALL)
def test_gmm_small_shapes_on_exact_workspaces(N, F, K):
    _gmm_test(N, F, K)


# ---------------------------------------------------------------------------------------------------------------- whole fit

def test_whole_fit_with_two_tiles_per_slice():
    """fit_gaussian_mixture with the device k-means start at N = 65601 against the float64 references end to end."""
    from sklearn.exceptions import ConvergenceWarning
    from nnmnkwii_amd import mixture
    N, F, K = 65601, 4, 3
    X = R.aligner_like(N, F, 0, 0.3)
    labels, _, _, _ = R.kmeans(X, K, random_state=0)
    w, mu, cov, U, lower, n_iter, converged = G.fit(X, *R.mixture_start(X, labels, K), 3, 0.0, 1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        g = mixture.fit_gaussian_mixture(X, K, init="kmeans", max_iter=3, tol=0, random_state=0)
    assert g.n_iter_ == 3 == n_iter and not g.converged_ and not converged
    check("weights", g.weights_, w)
    check("means", g.means_, mu)
    check("covariances", g.covariances_, cov)
    check("lower bound", g.lower_bound_, lower)
    check("precisions_cholesky_", g.precisions_cholesky_, U, max(1e-10, 8 * EPS * G.cond(cov)))
