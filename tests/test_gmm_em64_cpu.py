"""Pins tests/gmm_em64.py -- the float64 numpy reference the GPU tests of the EM kernels compare against -- on scikit-learn itself
(-m "not gpu"): five EM iterations with tol=0 from a max_iter=0 start, against GaussianMixture(max_iter=5, tol=0, *_init=...).
Bounds: 1e-11 of each array's maximum for weights, means, covariances and the lower bound; max(1e-10, 8 eps cond) for everything
that passes through the triangular factors (precisions_cholesky_, predict_proba, score), cond being the largest condition number
of the reference's covariances: the factor of a matrix of condition cond is determined to about eps cond."""
import warnings

import numpy as np
import pytest
from sklearn.mixture import GaussianMixture

import gmm_em64 as R

EPS = np.finfo(np.float64).eps
SHAPES = [(257, 6, 3), (1000, 33, 4), (1500, 128, 3), (700, 2, 16), (2000, 50, 16)]


@pytest.mark.parametrize("zero_tail", [0.0, 0.3])
@pytest.mark.parametrize("N,F,K", SHAPES)
def test_reference_follows_sklearn(N, F, K, zero_tail):
    X = R.synthetic(N, F, K, seed=N + F, zero_tail=zero_tail)
    g0 = GaussianMixture(n_components=K, covariance_type="full", max_iter=0, random_state=0).fit(X)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = GaussianMixture(n_components=K, covariance_type="full", max_iter=5, tol=0, weights_init=g0.weights_,
                             means_init=g0.means_, precisions_init=g0.precisions_).fit(X)
    w, mu, cov, U, lower, n_iter, converged = R.fit(X, g0.weights_, g0.means_, g0.covariances_, 5, 0.0, 1e-6)
    assert n_iter == 5 == sk.n_iter_ and not converged and not sk.converged_
    for name, got, ref in (("weights", w, sk.weights_), ("means", mu, sk.means_), ("covariances", cov, sk.covariances_),
                           ("lower bound", lower, sk.lower_bound_)):
        d = R.dist(got, ref)
        print(name, d)
        assert d <= 1e-11, (name, d)
    bound = max(1e-10, 8 * EPS * R.cond(cov))
    log_det = np.sum(np.log(U.reshape(K, -1)[:, ::F + 1]), axis=1)
    resp, lpn, labels, mean = R.e_step(X, w, mu, U, log_det)
    for name, got, ref in (("precisions_cholesky_", U, sk.precisions_cholesky_), ("predict_proba", resp, sk.predict_proba(X)),
                           ("score_samples", lpn, sk.score_samples(X)), ("score", mean, sk.score(X))):
        d = R.dist(got, ref)
        print(name, d, bound)
        assert d <= bound, (name, d, bound)
    assert np.allclose(U, np.triu(U)) and np.array_equal(U, np.triu(U))


def test_reference_loop_stops_on_tol_and_refuses_a_singular_covariance():
    X = R.synthetic(400, 3, 2, seed=1)
    g0 = GaussianMixture(n_components=2, covariance_type="full", max_iter=0, random_state=0).fit(X)
    sk = GaussianMixture(n_components=2, covariance_type="full", max_iter=100, tol=1e-3, weights_init=g0.weights_,
                         means_init=g0.means_, precisions_init=g0.precisions_).fit(X)
    out = R.fit(X, g0.weights_, g0.means_, g0.covariances_, 100, 1e-3, 1e-6)
    assert out[6] and sk.converged_ and out[5] == sk.n_iter_
    x = np.array([[1.0, 2.0, 3.0]] * 2)
    with pytest.raises(np.linalg.LinAlgError):
        R.fit(x, np.array([0.5, 0.5]), np.stack([x[0], x[0] + 100.0]), np.stack([np.eye(3)] * 2), 5, 0.0, 0.0)
