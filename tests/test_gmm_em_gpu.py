"""The float64 EM kernels for full-covariance mixtures (csrc/gmm_em.hip, nnmnkwii_amd.mixture) against the numpy reference
tests/gmm_em64.py, which tests/test_gmm_em64_cpu.py pins on scikit-learn.

Bounds: the project's float64 bound, 1e-10 of the reference array's maximum, for resp, log_prob_norm, the lower bound, weights,
means and covariances; max(1e-10, 8 eps cond) for the triangular factors U, cond being the largest condition number of the
reference's covariances.  Arg-max labels are compared on the rows whose two largest reference posteriors differ by more than 1e-9;
at most 1 % of the rows may be left out.  The columns of every input carry distinct scales, so a permuted or transposed MFMA tile
is an O(1) error.

Not yet run on a device (none could be had when this was written): no figures to report.  The same kernel text passes the same
bounds on the CPU behind an emulation of the documented lane maps (tests/test_gmm_em_host_cpu.py)."""
import warnings

import numpy as np
import pytest
import torch

import gmm_em64 as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
FS = [1, 2, 15, 16, 17, 33, 128]
KS = [1, 3, 16, 64]
NS = [1, 15, 17, 257, 1025]
_cache = {}


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def model(F, K):
    """A random mixture with distinct column scales, shared by the single-step tests: (weights, means, cov, U, log_det, cond)."""
    if (F, K) not in _cache:
        rng = np.random.RandomState(1000 * F + K)
        scales = rng.permutation(np.linspace(0.5, 3.0, F))
        A = rng.randn(K, F, F) / np.sqrt(F)
        cov = (A @ A.transpose(0, 2, 1) + 0.5 * np.eye(F)) * np.outer(scales, scales)
        cov = 0.5 * (cov + cov.transpose(0, 2, 1))
        means = 2.0 * rng.randn(K, F) / np.sqrt(F) * scales
        weights = rng.dirichlet(np.full(K, 5.0))
        U, log_det = R.precisions(cov)
        _cache[F, K] = (weights, means, cov, U, log_det, R.cond(cov))
    return _cache[F, K]


def rows(N, F, K, means, cov, seed):
    rng = np.random.RandomState(seed)
    lab = rng.randint(K, size=N)
    L = np.linalg.cholesky(cov)
    return means[lab] + np.einsum("nfg,ng->nf", L[lab], rng.randn(N, F))


def check(name, got, ref, bound=1e-10):
    d = R.dist(got.cpu().numpy() if torch.is_tensor(got) else got, ref)
    print("%s: %.3g (bound %.3g)" % (name, d, bound))
    assert d <= bound, (name, d, bound)


def check_labels(labels, resp_ref):
    top = np.sort(resp_ref, axis=1)[:, ::-1]
    clear = np.ones(len(resp_ref), bool) if resp_ref.shape[1] == 1 else (top[:, 0] - top[:, 1] > 1e-9)
    assert (~clear).mean() <= 0.01, (~clear).mean()
    assert np.array_equal(np.asarray(labels)[clear], resp_ref.argmax(axis=1)[clear])


@pytest.mark.parametrize("F", FS)
def test_estep_single_steps(F):
    from nnmnkwii_amd import _hip
    for K in KS:
        weights, means, cov, U, log_det, _ = model(F, K)
        for N in NS:
            X = rows(N, F, K, means, cov, N)
            resp_r, lpn_r, _, mean_r = R.e_step(X, weights, means, U, log_det)
            resp, lpn, labels, mean = _hip.gmm_estep(dev(X), dev(weights), dev(means), dev(U), dev(log_det), want_resp=True,
                                                     want_log_prob_norm=True, want_labels=True, want_mean=True)
            tag = "F=%d K=%d N=%d " % (F, K, N)
            check(tag + "resp", resp, resp_r)
            check(tag + "log_prob_norm", lpn, lpn_r)
            check(tag + "mean", mean, mean_r)
            check_labels(labels.cpu().numpy(), resp_r)
            # every output is optional
            only = _hip.gmm_estep(dev(X), dev(weights), dev(means), dev(U), dev(log_det), want_resp=False, want_labels=True)
            assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2], labels)


@pytest.mark.parametrize("F", FS)
def test_mstep_single_steps(F):
    from nnmnkwii_amd import _hip
    for K in KS:
        _, means, cov, _, _, _ = model(F, K)
        for N in NS:
            X = rows(N, F, K, means, cov, N + 1)
            resp = np.random.RandomState(N + K).dirichlet(np.full(K, 0.7), size=N)
            w_r, mu_r, cov_r = R.m_step(X, resp, 1e-6)
            w, mu, c = _hip.gmm_mstep(dev(X), dev(resp), 1e-6)
            tag = "F=%d K=%d N=%d " % (F, K, N)
            check(tag + "weights", w, w_r)
            check(tag + "means", mu, mu_r)
            check(tag + "covariances", c, cov_r)
            assert torch.equal(c, c.transpose(1, 2))
            w2, mu2, c2 = _hip.gmm_mstep(dev(X), dev(resp), 1e-6)
            assert torch.equal(w, w2) and torch.equal(mu, mu2) and torch.equal(c, c2)


@pytest.mark.parametrize("F", FS)
def test_precisions_single_steps(F):
    from nnmnkwii_amd import _hip
    for K in KS:
        _, _, cov, U_r, log_det_r, cond = model(F, K)
        U, log_det, status = _hip.gmm_precisions(dev(cov))
        assert not status.any().item()
        tag = "F=%d K=%d " % (F, K)
        check(tag + "U", U, U_r, max(1e-10, 8 * EPS * cond))
        check(tag + "log_det", log_det, log_det_r)
        assert torch.equal(U, torch.triu(U))
    # a pivot that is <= 0 or NaN sets the component's status word to its 1-based index; the others are untouched by it
    _, _, cov, U_r, _, cond = model(F, 3)
    bad = cov.copy()
    bad[1] = 0.0 if F == 1 else bad[1]
    if F > 1:
        bad[1, F - 1, :] = bad[1, F - 2, :]
        bad[1, :, F - 1] = bad[1, :, F - 2]
        bad[1, F - 1, F - 1] = bad[1, F - 2, F - 2] * (1 - 1e-3)      # the Schur complement of the last pivot is negative
    bad[2, 0, 0] = np.nan
    U, _, status = _hip.gmm_precisions(dev(bad))
    assert status.cpu().tolist() == [0, F, 1]
    check("U of the good component", U[0], U_r[0], max(1e-10, 8 * EPS * cond))


def start(X, K):
    from sklearn.mixture import GaussianMixture
    g0 = GaussianMixture(n_components=K, covariance_type="full", max_iter=0, random_state=0).fit(X)
    return g0.weights_, g0.means_, g0.covariances_


def fit5(X, K, init):
    from sklearn.exceptions import ConvergenceWarning
    from nnmnkwii_amd.mixture import fit_gaussian_mixture
    with pytest.warns(ConvergenceWarning):
        return fit_gaussian_mixture(X, K, max_iter=5, tol=0, init=init)


@pytest.mark.parametrize("N,F,K,zero_tail", [(257, 6, 3, 0.0), (1000, 33, 4, 0.0), (700, 2, 16, 0.0), (1000, 33, 4, 0.3)])
def test_five_iteration_fits(N, F, K, zero_tail):
    X = R.synthetic(N, F, K, seed=N + F, zero_tail=zero_tail)
    init = start(X, K)
    w, mu, cov, U, lower, n_iter, converged = R.fit(X, *init, 5, 0.0, 1e-6)
    g = fit5(X, K, init)
    assert g.n_iter_ == 5 and not g.converged_ and len(g.lower_bounds_) == 5
    check("weights", g.weights_, w)
    check("means", g.means_, mu)
    check("covariances", g.covariances_, cov)
    check("lower bound", g.lower_bound_, lower)
    check("precisions_cholesky_", g.precisions_cholesky_, U, max(1e-10, 8 * EPS * R.cond(cov)))
    check("precisions_", g.precisions_, U @ U.transpose(0, 2, 1), max(1e-10, 8 * EPS * R.cond(cov)))
    # bitwise equality of two fits
    g2 = fit5(X, K, init)
    for a in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
        assert np.array_equal(getattr(g, a), getattr(g2, a)), a
    assert g.lower_bound_ == g2.lower_bound_
    # the result is an ordinary fitted mixture: scikit-learn evaluates it, and so do the device functions
    from nnmnkwii_amd import mixture as M
    log_det = np.sum(np.log(U.reshape(K, -1)[:, ::F + 1]), axis=1)
    resp_r, lpn_r, _, _ = R.e_step(X, w, mu, U, log_det)
    check("sklearn predict_proba of the result", g.predict_proba(X), resp_r)
    check("predict_proba", M.predict_proba(g, X), resp_r)
    check("score_samples", M.score_samples(g, X.astype(np.float32).astype(np.float64)), R.e_step(
        X.astype(np.float32).astype(np.float64), w, mu, U, log_det)[1])
    out32 = M.score_samples(g, X.astype(np.float32))
    assert out32.dtype == np.float64 and np.array_equal(out32, M.score_samples(g, X.astype(np.float32).astype(np.float64)))
    labels = M.predict(g, X)
    assert labels.dtype == np.int64
    check_labels(labels, resp_r)
    t = M.predict_proba(g, dev(X))
    assert torch.is_tensor(t) and t.is_cuda and np.array_equal(t.cpu().numpy(), M.predict_proba(g, X))


def test_fit_stops_on_tol_defaults_to_sklearns_start_and_checks_its_arguments():
    from sklearn.mixture import GaussianMixture
    from nnmnkwii_amd.mixture import fit_gaussian_mixture
    X = R.synthetic(400, 3, 2, seed=1)
    init = start(X, 2)
    ref = R.fit(X, *init, 100, 1e-3, 1e-6)
    from sklearn.exceptions import ConvergenceWarning
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        g = fit_gaussian_mixture(X, 2, init=init)
        assert g.converged_ and g.n_iter_ == ref[5]
        check("means", g.means_, ref[1])
        g0 = fit_gaussian_mixture(X, 2, max_iter=0, random_state=0)         # scikit-learn's own start, no iteration, no warning
    assert g0.n_iter_ == 0 and not g0.converged_ and g0.lower_bound_ == -np.inf
    check("start means", g0.means_, init[1])
    h = fit_gaussian_mixture(dev(X), 2, init=GaussianMixture(2, max_iter=0, random_state=0).fit(X))      # a CUDA tensor, a fitted start
    assert np.array_equal(h.means_, g.means_)
    for kw, word in ((dict(X=np.zeros((10, 129)), n_components=2), "128"), (dict(X=X, n_components=65), "64"),
                     (dict(X=X, n_components=0), "64")):
        with pytest.raises(ValueError, match=word):
            fit_gaussian_mixture(kw["X"], kw["n_components"], init=init)


def test_singular_covariance_raises_sklearns_error():
    from nnmnkwii_amd.mixture import fit_gaussian_mixture
    x = np.array([[1.0, 2.0, 3.0]] * 2)
    init = (np.array([0.5, 0.5]), np.stack([x[0], x[0] + 100.0]), np.stack([np.eye(3)] * 2))
    with pytest.raises(np.linalg.LinAlgError):
        R.fit(x, *init, 5, 0.0, 0.0)
    with pytest.raises(ValueError, match="^Fitting the mixture model failed because some components have ill-defined empirical "
                                         "covariance"):
        fit_gaussian_mixture(x, 2, max_iter=5, tol=0, reg_covar=0.0, init=init)


def joint_model(D, K, seed=3):
    from sklearn.mixture import GaussianMixture
    rng = np.random.RandomState(seed)
    src = R.synthetic(600, D, K, seed=seed)
    tgt = src @ (np.eye(D) + 0.2 * rng.randn(D, D)) + 0.3 * rng.randn(600, D)
    return GaussianMixture(n_components=K, covariance_type="full", random_state=0).fit(np.hstack([src, tgt])), src


def test_device_posteriors_in_the_conversion():
    from nnmnkwii_amd.baseline.gmm import MLPG, MLPGBase
    gmm, src = joint_model(6, 4)
    for cls, kw in ((MLPGBase, {}), (MLPG, dict(windows=[(0, 0, np.array([1.0]))]))):
        a, b = cls(gmm, **kw), cls(gmm, posterior="device", **kw)
        check(cls.__name__ + " transform", b.transform(src[:77]), a.transform(src[:77]))
        if cls is MLPGBase:
            check("MLPGBase frame", b.transform(src[5]), a.transform(src[5]))
        for x, y in zip(b.transform_batch([src[:40], src[40:41], src[41:160]]), a.transform_batch([src[:40], src[40:41], src[41:160]])):
            check(cls.__name__ + " transform_batch", x, y)
    # with delta windows: the arg-max mixture of each frame, then the trajectory
    a, b = MLPG(gmm), MLPG(gmm, posterior="device")
    assert a.static_dim == 3
    check("MLPG trajectory", b.transform(src[:90]), a.transform(src[:90]))
    with pytest.raises(ValueError):
        MLPG(gmm, posterior="host")


def test_aligner_with_the_device_mixture(monkeypatch):
    from sklearn.mixture import GaussianMixture
    from nnmnkwii_amd.preprocessing.alignment import IterativeDTWAligner
    rng = np.random.RandomState(7)
    N, T, D = 4, 48, 3
    X, Y = np.zeros((N, T, D)), np.zeros((N, T + 4, D))
    lens = [(40, 44), (37, 41), (48, 39), (42, 52)]
    for n, (a, b) in enumerate(lens):
        base = np.cumsum(rng.randn(60, D), axis=0)
        X[n, :a] = base[np.sort(rng.choice(60, a, replace=False))] + 0.05 * rng.randn(a, D)
        Y[n, :b] = 0.8 * base[np.sort(rng.choice(60, b, replace=False))] + 0.3 + 0.05 * rng.randn(b, D)
    fit = GaussianMixture.fit
    calls = []

    def only_the_start(self, X, y=None):
        assert self.max_iter == 0, "the EM iterations belong to the device"
        calls.append(X.shape)
        return fit(self, X, y)
    monkeypatch.setattr(GaussianMixture, "fit", only_the_start)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Xa, Ya = IterativeDTWAligner(n_iter=2, n_components_gmm=2, max_iter_gmm=10, gmm="device").transform((X, Y))
    assert len(calls) == 2 and all(s[1] == 2 * D for s in calls)
    assert Xa.shape == Ya.shape and Xa.shape[0] == N and Xa.shape[2] == D and Xa.shape[1] >= T + 4
    assert Xa.dtype == X.dtype and Ya.dtype == Y.dtype
    for n, (a, b) in enumerate(lens):
        # the live rows: a warping path from (0, 0) to the last frames, non-decreasing, every row a row of the pair
        i = j = 0
        k = 0
        assert np.array_equal(Xa[n, 0], X[n, 0]) and np.array_equal(Ya[n, 0], Y[n, 0])
        while (i, j) != (a - 1, b - 1):
            k += 1
            steps = [(i + di, j + dj) for di, dj in ((1, 1), (1, 0), (0, 1)) if i + di < a and j + dj < b]
            hit = [(p, q) for p, q in steps if np.array_equal(Xa[n, k], X[n, p]) and np.array_equal(Ya[n, k], Y[n, q])]
            assert len(hit) == 1, (n, k, i, j)
            i, j = hit[0]
        assert k + 1 >= max(a, b)
    with pytest.raises(ValueError):
        IterativeDTWAligner(gmm="gpu")
