"""Float64 numpy reference of the EM for full-covariance Gaussian mixtures: scikit-learn's _e_step / _m_step / precisions and its
fit loop restated (sklearn/mixture/_base.py, _gaussian_mixture.py), with log p taken from (x - mu_k) U_k as the device does.
tests/test_gmm_em64_cpu.py pins it on scikit-learn itself; tests/test_gmm_em_gpu.py checks the HIP kernels against it."""
import numpy as np
from scipy import linalg
from scipy.special import logsumexp


def precisions(cov):
    """(U (K, F, F) upper with U U^T = cov^-1, log_det (K)); LinAlgError when a covariance is not positive definite."""
    K, F, _ = cov.shape
    U = np.empty((K, F, F))
    for k in range(K):
        L = linalg.cholesky(cov[k], lower=True)
        U[k] = linalg.solve_triangular(L, np.eye(F), lower=True).T
    return U, np.sum(np.log(U.reshape(K, -1)[:, ::F + 1]), axis=1)


def weighted_log_prob(X, weights, means, U, log_det):
    N, F = X.shape
    sq = np.stack([np.sum(np.square((X - mu) @ u), axis=1) for mu, u in zip(means, U)], axis=1)
    return -0.5 * (F * np.log(2 * np.pi) + sq) + log_det + np.log(weights)


def e_step(X, weights, means, U, log_det):
    """(resp (N, K), log_prob_norm (N), labels (N), mean of log_prob_norm)."""
    wlp = weighted_log_prob(X, weights, means, U, log_det)
    lpn = logsumexp(wlp, axis=1)
    return np.exp(wlp - lpn[:, None]), lpn, wlp.argmax(axis=1), np.mean(lpn)


def m_step(X, resp, reg_covar):
    """(weights (K), means (K, F), covariances (K, F, F))."""
    N, F = X.shape
    nk = resp.sum(axis=0) + 10 * np.finfo(np.float64).eps
    means = resp.T @ X / nk[:, None]
    cov = np.empty((len(nk), F, F))
    for k in range(len(nk)):
        d = X - means[k]
        cov[k] = (resp[:, k] * d.T) @ d / nk[k]
        cov[k].flat[::F + 1] += reg_covar
    return nk / nk.sum(), means, cov


def fit(X, weights, means, cov, max_iter, tol, reg_covar):
    """sklearn's loop from a given start: (weights, means, cov, U, lower_bound, n_iter, converged)."""
    U, log_det = precisions(cov)
    lower, converged, n_iter = -np.inf, False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        resp, _, _, lower = e_step(X, weights, means, U, log_det)
        weights, means, cov = m_step(X, resp, reg_covar)
        U, log_det = precisions(cov)
        if abs(lower - prev) < tol:
            converged = True
            break
    return weights, means, cov, U, lower, n_iter, converged


def synthetic(N, F, K, seed=0, zero_tail=0.0):
    """Overlapping correlated clusters, every column on its own scale; the last ``zero_tail`` share of the rows zero."""
    rng = np.random.RandomState(seed)
    scales = rng.permutation(np.linspace(0.5, 3.0, F))
    centers = 2.0 * rng.randn(K, F) / np.sqrt(F)
    mix = np.eye(F) + 0.3 * rng.randn(K, F, F) / np.sqrt(F)
    lab = rng.randint(K, size=N)
    X = (centers[lab] + np.einsum("nf,nfg->ng", rng.randn(N, F), mix[lab])) * scales
    X[N - int(round(zero_tail * N)):] = 0.0
    return X


def cond(cov):
    return max(np.linalg.cond(c) for c in cov)


def dist(a, ref):
    """max |a - ref| as a share of max |ref|."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - ref)) / max(np.max(np.abs(ref)), np.finfo(np.float64).tiny))
