"""The device k-means of csrc/kmeans.hip on the GPU: single seed and Lloyd steps against tests/kmeans64.py (pinned
on scikit-learn by tests/test_kmeans64_cpu.py), whole fits and mixture starts against scikit-learn itself, the relocation of an
empty cluster, bitwise repeatability, and an aligner that never enters scikit-learn's fit.  Bounds: 1e-10 of the reference
array's maximum; counts, the changed-label count and -- on rows whose best and second-best value are more than 1e-9 of the
largest apart, which is every row of the data used here -- labels exact."""
import functools
import warnings

import numpy as np
import pytest

import kmeans64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda") if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda").to(dtype)


@pytest.mark.parametrize("K", [1, 3, 16, 64])
@pytest.mark.parametrize("F", [1, 2, 17, 50, 128])
def test_single_steps(torch, F, K):
    from nnmnkwii_amd import _hip
    for N in (1, 63, 64, 65, 257, 1025):
        C = 1 + (N + F + K) % 8
        case = R.step_case(N, F, K, C, 1000 * F + 10 * K + N)
        Xc = case["X"] - case["shift"]
        x, shift = _dev(torch, case["X"]), _dev(torch, case["shift"])
        cand = _dev(torch, case["cand"], torch.int32)
        before = _hip.lib().mlpg_hip_launch_count(26), _hip.lib().mlpg_hip_launch_count(27)
        for closest in (None, case["closest"]):
            d, pots = _hip.kmeans_seed_step(x, shift, cand, None if closest is None else _dev(torch, closest))
            d_r, p_r = R.seed_step(Xc, case["cand"], closest)
            e = R.dist(d.cpu().numpy(), d_r), R.dist(pots.cpu().numpy(), p_r)
            print("N %d F %d K %d C %d: d %.2e pots %.2e" % (N, F, K, C, *e))
            assert max(e) <= 1e-10, (N, e)
        ref = R.step_expected(case)
        centers, prev = _dev(torch, case["centers"]), _dev(torch, case["prev"])
        labels, min_dist, sums, counts, out, stats = _hip.kmeans_lloyd_step(x, shift, centers, prev, want_min_dist=True)
        move, inertia, changed, empty = _hip.kmeans_stats(stats)
        R.check_step(case, ref, dict(labels=labels.cpu().numpy(), min_dist=min_dist.cpu().numpy(), sums=sums.cpu().numpy(),
                                     counts=counts.cpu().numpy(), centers=out.cpu().numpy(), shift=move, inertia=inertia,
                                     changed=changed, empty=empty))
        assert torch.equal(x, _dev(torch, case["X"]))                      # the caller's rows are never modified
        # the centre update turned off, from the labels just found: nothing changed, no shift, no centres, the same inertia
        labels2, md2, sums2, counts2, out2, stats2 = _hip.kmeans_lloyd_step(x, shift, centers, labels, update_centers=False)
        move2, inertia2, changed2, empty2 = _hip.kmeans_stats(stats2)
        assert out2 is None and md2 is None and torch.equal(labels2, labels) and torch.equal(sums2, sums) and torch.equal(counts2, counts)
        assert changed2 == 0 and move2 == 0.0 and empty2 == ref["empty"] and inertia2 == inertia
        after = _hip.lib().mlpg_hip_launch_count(26), _hip.lib().mlpg_hip_launch_count(27)
        assert after == (before[0] + 2, before[1] + 2)


@functools.lru_cache(maxsize=None)
def _sklearn_fit(i):
    """(X, KMeans fitted, GaussianMixture(max_iter=0) fitted) of data set i, computed once."""
    from sklearn.cluster import KMeans
    from sklearn.mixture import GaussianMixture
    from sklearn.utils import check_random_state
    N, F, K, seed, zero_share = R.DATA_SETS[i]
    X = R.aligner_like(N, F, seed, zero_share)
    km = KMeans(n_clusters=K, n_init=1, random_state=check_random_state(seed)).fit(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = GaussianMixture(K, max_iter=0, random_state=seed).fit(X)
    return X, km, gm


@pytest.mark.parametrize("i", range(len(R.DATA_SETS)))
def test_whole_fit_against_sklearn(torch, i):
    from nnmnkwii_amd import mixture
    K, seed = R.DATA_SETS[i][2], R.DATA_SETS[i][3]
    X, km, gm = _sklearn_fit(i)
    labels, centers, inertia, n_iter = mixture.kmeans(X, K, random_state=seed)
    print("n_iter %d (sklearn %d), centres %.2e, inertia %.2e, labels differing %d"
          % (n_iter, km.n_iter_, R.dist(centers, km.cluster_centers_), R.dist(inertia, km.inertia_), np.sum(labels != km.labels_)))
    assert labels.dtype == np.int64 and np.array_equal(labels, km.labels_)
    assert n_iter == km.n_iter_
    assert R.dist(centers, km.cluster_centers_) <= 1e-10 and R.dist(inertia, km.inertia_) <= 1e-10
    # a float64 CUDA tensor is used in place and tensors come back
    xt = torch.from_numpy(X).cuda()
    lt, ct, it, nt = mixture.kmeans(xt, K, random_state=seed)
    assert lt.is_cuda and lt.dtype == torch.int32 and ct.is_cuda and torch.equal(xt, torch.from_numpy(X).cuda())
    assert np.array_equal(lt.cpu().numpy(), labels) and np.array_equal(ct.cpu().numpy(), centers) and it == inertia and nt == n_iter


@pytest.mark.parametrize("i", range(len(R.DATA_SETS)))
def test_mixture_start_against_sklearn(torch, i):
    from nnmnkwii_amd import mixture
    K, seed = R.DATA_SETS[i][2], R.DATA_SETS[i][3]
    X, km, gm = _sklearn_fit(i)
    fit = mixture.fit_gaussian_mixture(X, K, init="kmeans", max_iter=0, random_state=seed)
    for name, got, ref in (("weights", fit.weights_, gm.weights_), ("means", fit.means_, gm.means_),
                           ("covariances", fit.covariances_, gm.covariances_)):
        print("%s %.2e" % (name, R.dist(got, ref)))
        assert R.dist(got, ref) <= 1e-10, (name, R.dist(got, ref))
    with pytest.raises(ValueError):
        mixture.fit_gaussian_mixture(X, K, init="k-means", max_iter=0)


def test_random_state_none_consumes_the_global_generator_as_sklearn_does(torch):
    from sklearn.mixture import GaussianMixture
    from nnmnkwii_amd import mixture
    N, F, K, seed, zero_share = R.DATA_SETS[4]
    X = R.aligner_like(N, F, seed, zero_share)
    np.random.seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = GaussianMixture(K, max_iter=0).fit(X)
    after_sklearn = np.random.rand()
    np.random.seed(7)
    fit = mixture.fit_gaussian_mixture(X, K, init="kmeans", max_iter=0)
    assert np.random.rand() == after_sklearn
    for got, ref in ((fit.weights_, gm.weights_), (fit.means_, gm.means_), (fit.covariances_, gm.covariances_)):
        assert R.dist(got, ref) <= 1e-10


def test_one_empty_cluster_is_relocated_as_sklearn_does(torch):
    from sklearn.cluster import KMeans
    from nnmnkwii_amd import _hip, mixture
    X, init = R.relocation_case()
    mean = X.mean(axis=0)
    stats = _hip.kmeans_lloyd_step(_dev(torch, X), _dev(torch, mean), _dev(torch, init - mean),
                                   torch.full((len(X),), -1, dtype=torch.int32, device="cuda"))[5]
    assert _hip.kmeans_stats(stats)[3] == 1                  # exactly one cluster is empty in the first iteration
    km = KMeans(n_clusters=len(init), init=init, n_init=1).fit(X)
    labels, centers, inertia, n_iter = mixture.kmeans(X, len(init), init=init)
    assert np.array_equal(labels, km.labels_) and n_iter == km.n_iter_
    assert R.dist(centers, km.cluster_centers_) <= 1e-10 and R.dist(inertia, km.inertia_) <= 1e-10


def test_two_calls_give_the_same_bits(torch):
    from nnmnkwii_amd import _hip, mixture
    N, F, K, seed, zero_share = R.DATA_SETS[0]
    x = torch.from_numpy(R.aligner_like(N, F, seed, zero_share)).cuda()
    a, b = (mixture.kmeans(x, K, random_state=seed) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    case = R.step_case(1025, 50, 16, 6, 5)
    xs, shift, cand, closest = (_dev(torch, case[k]) for k in ("X", "shift", "cand", "closest"))
    p, q = (_hip.kmeans_seed_step(xs, shift, cand.to(torch.int32), closest) for _ in range(2))
    assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])


def test_aligner_without_sklearns_fit(torch, monkeypatch):
    import sklearn.cluster
    import sklearn.mixture
    from nnmnkwii_amd.preprocessing.alignment import IterativeDTWAligner
    rng = np.random.RandomState(3)
    n, T, D = 8, 60, 5
    X, Y = np.zeros((n, T, D)), np.zeros((n, T, D))
    for i in range(n):
        a, b = T - rng.randint(0, 12), T - rng.randint(0, 12)
        base = np.cumsum(rng.randn(80, D), axis=0)             # two time warpings of one random walk, a little noise on one
        X[i, :a] = base[np.sort(rng.choice(80, a, replace=False))]
        Y[i, :b] = base[np.sort(rng.choice(80, b, replace=False))] + 0.05 * rng.randn(b, D)
    with pytest.raises(ValueError):
        IterativeDTWAligner(gmm="sklearn", gmm_init="kmeans-device")
    assert IterativeDTWAligner().gmm_init == "sklearn"
    np.random.seed(5)
    Xs, Ys = IterativeDTWAligner(n_iter=2, n_components_gmm=4, gmm="device", gmm_init="sklearn").transform((X, Y))

    def refuse(self, *a, **k):
        raise AssertionError("scikit-learn's fit was called")
    monkeypatch.setattr(sklearn.cluster.KMeans, "fit", refuse)
    monkeypatch.setattr(sklearn.mixture.GaussianMixture, "fit", refuse)
    np.random.seed(5)
    Xa, Ya = IterativeDTWAligner(n_iter=2, n_components_gmm=4, gmm="device", gmm_init="kmeans-device").transform((X, Y))
    assert Xa.shape == Ya.shape
    assert np.linalg.norm(Xa - Ya) < np.linalg.norm(X - Y)
    assert Xa.shape == Xs.shape and np.allclose(Xa, Xs, rtol=1e-6) and np.allclose(Ya, Ys, rtol=1e-6)
