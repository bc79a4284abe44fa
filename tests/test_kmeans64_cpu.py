"""tests/kmeans64.py -- the float64 numpy restatement of the mixture's k-means start that the HIP kernels are checked against --
pinned on scikit-learn itself (-m "not gpu"): KMeans(n_init=1) for the labels, the iteration count, the centres and the inertia,
GaussianMixture(max_iter=0) for the start of the EM, on aligner-like data (random walks with a share of rows exactly zero), and
the relocation of one empty cluster from given centres.  Labels must be equal on every row: over all iterations the gap between
a row's best and second-best distance is many orders of magnitude above rounding on these data sets."""
import warnings

import numpy as np
import pytest
from sklearn.cluster import KMeans
from sklearn.mixture import GaussianMixture
from sklearn.utils import check_random_state

import kmeans64 as R


@pytest.mark.parametrize("N,F,K,seed,zero_share", R.DATA_SETS)
def test_restatement_against_sklearn(N, F, K, seed, zero_share):
    X = R.aligner_like(N, F, seed, zero_share)
    km = KMeans(n_clusters=K, n_init=1, random_state=check_random_state(seed)).fit(X)
    labels, centers, inertia, n_iter = R.kmeans(X, K, random_state=seed)
    print("n_iter %d, centres %.2e, inertia %.2e" % (n_iter, R.dist(centers, km.cluster_centers_), R.dist(inertia, km.inertia_)))
    assert np.array_equal(labels, km.labels_)
    assert n_iter == km.n_iter_
    assert R.dist(centers, km.cluster_centers_) <= 1e-10
    assert R.dist(inertia, km.inertia_) <= 1e-10
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm = GaussianMixture(K, max_iter=0, random_state=seed).fit(X)
    w, mu, cov = R.mixture_start(X, labels, K)
    for name, got, ref in (("weights", w, gm.weights_), ("means", mu, gm.means_), ("covariances", cov, gm.covariances_)):
        assert R.dist(got, ref) <= 1e-10, (name, R.dist(got, ref))


def test_draws_come_from_the_global_generator_in_sklearns_order():
    N, F, K, seed, zero_share = R.DATA_SETS[4]
    X = R.aligner_like(N, F, seed, zero_share)
    np.random.seed(7)
    km = KMeans(n_clusters=K, n_init=1).fit(X)
    after_sklearn = np.random.rand()
    np.random.seed(7)
    labels, centers, _, n_iter = R.kmeans(X, K)
    assert np.random.rand() == after_sklearn
    assert np.array_equal(labels, km.labels_) and n_iter == km.n_iter_ and R.dist(centers, km.cluster_centers_) <= 1e-10


def test_one_empty_cluster_is_relocated_as_sklearn_does():
    X, init = R.relocation_case()
    first = R.lloyd_step(X - X.mean(axis=0), init - X.mean(axis=0), np.full(len(X), -1))
    assert first["empty"] == 1
    km = KMeans(n_clusters=len(init), init=init, n_init=1).fit(X)
    labels, centers, inertia, n_iter = R.kmeans(X, len(init), init=init)
    assert np.array_equal(labels, km.labels_) and n_iter == km.n_iter_
    assert R.dist(centers, km.cluster_centers_) <= 1e-10 and R.dist(inertia, km.inertia_) <= 1e-10
