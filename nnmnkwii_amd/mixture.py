"""Full-covariance Gaussian mixtures fitted and evaluated on the GPU.

scikit-learn's float64 EM -- ``_e_step`` / ``_m_step`` of ``sklearn.mixture.GaussianMixture`` -- restated on the HIP kernels of
``csrc/gmm_em.hip`` (``mlpg_hip_gmm_estep`` / ``_mstep`` / ``_precisions``).  The result of :func:`fit_gaussian_mixture` is an
ordinary fitted ``GaussianMixture``: ``baseline.gmm.MLPG(gmm)`` takes it unchanged.  Only ``covariance_type="full"`` and one
initialisation (``n_init=1``); at most 128 features and 64 components.  There is no CPU fallback.

:func:`kmeans` is scikit-learn's ``KMeans(n_init=1)`` -- k-means++ seeding and Lloyd iterations -- on the kernels of
``csrc/kmeans.hip``; ``fit_gaussian_mixture(..., init="kmeans")`` starts the EM from it without X leaving the device.
"""
import warnings

import numpy as np

from . import _hip

_ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance "
                "caused by singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or "
                "scale the input data.")


def _check_limits(F, K):
    if not 1 <= F <= _hip.GMM_MAX_FEATURES:
        raise ValueError("the device mixture takes 1 to %d features, got %d" % (_hip.GMM_MAX_FEATURES, F))
    if not 1 <= K <= _hip.GMM_MAX_COMPONENTS:
        raise ValueError("the device mixture takes 1 to %d components, got %d" % (_hip.GMM_MAX_COMPONENTS, K))


def _is_tensor(X):
    return type(X).__module__.startswith("torch")


def _device_rows(X):
    """(float64 contiguous CUDA tensor (N, F), was a tensor).  numpy input of any dtype is widened to float64; a float64 CUDA
    tensor is used in place."""
    torch = _hip.torch_mod()
    if _is_tensor(X):
        if not X.is_cuda or X.dtype != torch.float64:
            raise ValueError("tensor input must be a float64 CUDA tensor, got %s on %s" % (X.dtype, X.device))
        _hip.require_gpu(X.device)
        if X.dim() != 2:
            raise ValueError("expected a 2-d array of rows, got %d dimensions" % X.dim())
        return X.contiguous(), True
    dev = _hip.require_gpu()
    a = np.ascontiguousarray(X, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("expected a 2-d array of rows, got %d dimensions" % a.ndim)
    return torch.from_numpy(a).to(dev), False


def _to_dev(a, dev):
    return _hip.torch_mod().from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _model(gmm, dev):
    """(weights, means, prec_chol, log_det) of a fitted full-covariance mixture as float64 tensors on ``dev``."""
    if getattr(gmm, "covariance_type", "full") != "full":
        raise ValueError("the device mixture takes covariance_type='full' only, got %r" % gmm.covariance_type)
    U = np.asarray(gmm.precisions_cholesky_, dtype=np.float64)
    K, F, _ = U.shape
    _check_limits(F, K)
    log_det = np.sum(np.log(U.reshape(K, -1)[:, ::F + 1]), axis=1)
    return _to_dev(gmm.weights_, dev), _to_dev(gmm.means_, dev), _to_dev(U, dev), _to_dev(log_det, dev)


def _evaluate(gmm, X, **want):
    """((resp, log_prob_norm, labels, mean) of the device E-step -- None where not asked for --, X was a tensor)."""
    x, was_tensor = _device_rows(X)
    w, mu, U, log_det = _model(gmm, x.device)
    if x.shape[1] != mu.shape[1]:
        raise ValueError("X has %d features, the mixture has %d" % (x.shape[1], mu.shape[1]))
    want.setdefault("want_resp", False)
    return _hip.gmm_estep(x, w, mu, U, log_det, **want), was_tensor


def predict_proba(gmm, X):
    """Posterior of every component for every row of ``X`` (``gmm.predict_proba(X)``) by the device E-step.  numpy input of any
    float dtype is computed and returned in float64 (scikit-learn would stay in float32 for float32 input); a float64 CUDA
    tensor is used in place and a CUDA tensor comes back."""
    (resp, _, _, _), was_tensor = _evaluate(gmm, X, want_resp=True)
    return resp if was_tensor else resp.cpu().numpy()


def predict(gmm, X):
    """The most likely component of every row (``gmm.predict(X)``): int64 ndarray for numpy input, int32 CUDA tensor for a CUDA
    tensor.  Computed in float64 whatever the input's dtype (see :func:`predict_proba`)."""
    (_, _, labels, _), was_tensor = _evaluate(gmm, X, want_labels=True)
    return labels if was_tensor else labels.cpu().numpy().astype(np.int64)


def score_samples(gmm, X):
    """The log-likelihood of every row (``gmm.score_samples(X)``), in float64 whatever the input's dtype (see
    :func:`predict_proba`)."""
    (_, lpn, _, _), was_tensor = _evaluate(gmm, X, want_log_prob_norm=True)
    return lpn if was_tensor else lpn.cpu().numpy()


def _start(X_host, n_components, reg_covar, init, random_state):
    """(weights, means, covariances) the EM starts from, float64 ndarrays."""
    from sklearn.mixture import GaussianMixture
    if init is None:
        # scikit-learn's own initialisation (k-means on the host; with random_state=None the draw comes from numpy's global generator)
        init = GaussianMixture(n_components=n_components, covariance_type="full", reg_covar=reg_covar, max_iter=0,
                               random_state=random_state).fit(X_host())
    if isinstance(init, GaussianMixture):
        if init.covariance_type != "full":
            raise ValueError("init must be a full-covariance mixture, got %r" % init.covariance_type)
        init = (init.weights_, init.means_, init.covariances_)
    w, mu, cov = (np.ascontiguousarray(a, dtype=np.float64) for a in init)
    K = n_components
    if w.shape != (K,) or mu.ndim != 2 or mu.shape[0] != K or cov.shape != (K, mu.shape[1], mu.shape[1]):
        raise ValueError("init must hold weights (K,), means (K, F) and covariances (K, F, F) for K = %d; got %s, %s, %s"
                         % (K, w.shape, mu.shape, cov.shape))
    return w, mu, cov


def _relocate(xc, centers, labels, min_dist, sums, counts):
    """scikit-learn's _relocate_empty_clusters_dense by torch operations (the rare path): the rows farthest from their centre, one
    per empty cluster in descending order, become the empty clusters' sums with count 1 and leave their old clusters.  Returns
    (new centres, their shift as a 0-dim tensor); the labels stay."""
    torch = _hip.torch_mod()
    sums, counts = sums.clone(), counts.clone()
    empty = torch.nonzero(counts == 0).flatten()
    far = torch.topk(min_dist, int(empty.numel())).indices
    for new, n in zip(empty.tolist(), far.tolist()):
        old = int(labels[n])
        row = xc(n)
        sums[old] -= row
        sums[new] = row
        counts[new] = 1.0
        counts[old] -= 1.0
    pos = counts > 0
    new_centers = torch.where(pos[:, None], sums / torch.where(pos, counts, torch.ones_like(counts))[:, None], sums)
    return new_centers, torch.sum(torch.square(new_centers - centers))


def _kmeans_device(x, K, max_iter, tol, random_state, init):
    """k-means on float64 CUDA rows: (labels int32 (N), centres (K, F), inertia, n_iter), the tensors on x's device."""
    from sklearn.utils import check_random_state
    torch = _hip.torch_mod()
    N, F = x.shape
    dev = x.device
    rs = check_random_state(random_state)
    tol_abs = float(torch.var(x, dim=0, unbiased=False).mean()) * tol if tol != 0 else 0.0
    shift = x.mean(dim=0).contiguous()
    ws = _hip.kmeans_workspace(dev, N, F, K)

    if init is None:
        # k-means++: the draws on the host in scikit-learn's order, everything over the rows on the device
        trials = 2 + int(np.log(K))
        first = rs.choice(N, p=np.ones(N) / N)
        idx = torch.empty((K,), dtype=torch.int64, device=dev)
        idx[0] = int(first)
        d, pots = _hip.kmeans_seed_step(x, shift, idx[:1].to(torch.int32), None, workspace=ws)
        closest, pot = d[0], float(pots.cpu()[0])
        for c in range(1, K):
            rand = torch.from_numpy(rs.uniform(size=trials) * pot).to(dev)
            cand = torch.searchsorted(torch.cumsum(closest, dim=0), rand).clamp_(max=N - 1)
            d, pots = _hip.kmeans_seed_step(x, shift, cand.to(torch.int32), closest, workspace=ws)
            back = pots.cpu().numpy()                       # the centre's one read-back: the pots of its candidates
            best = int(np.argmin(back))
            closest, pot = d[best], float(back[best])
            idx[c] = cand[best]
        centers = (x[idx] - shift).contiguous()
    else:
        centers = (_to_dev(init, dev) - shift).contiguous()

    labels_prev = torch.full((N,), -1, dtype=torch.int32, device=dev)
    labels, strict, relocated, n_iter = labels_prev, False, False, 0
    for n_iter in range(1, int(max_iter) + 1):
        labels, _, sums, counts, new_centers, stats = _hip.kmeans_lloyd_step(x, shift, centers, labels_prev, workspace=ws)
        move, _, changed, empty = _hip.kmeans_stats(stats)             # the iteration's one read-back
        relocated = empty > 0
        if relocated:
            # the same step again for the distances to the old centres (the same bits), then scikit-learn's relocation
            labels, min_dist, sums, counts, _, _ = _hip.kmeans_lloyd_step(x, shift, centers, labels_prev, want_min_dist=True,
                                                                          workspace=ws)
            new_centers, move_t = _relocate(lambda n: x[n] - shift, centers, labels, min_dist, sums, counts)
            new_centers, move = new_centers.contiguous(), float(move_t)
        centers = new_centers
        if changed == 0:
            strict = True
            break
        if move <= tol_abs:
            break
        labels_prev = labels
    # inertia against the final centres; without strict convergence the labels are assigned once more
    last, min_dist, _, _, _, stats = _hip.kmeans_lloyd_step(x, shift, centers, labels, update_centers=False,
                                                            want_min_dist=strict and relocated, workspace=ws)
    if not strict:
        labels = last
        inertia = _hip.kmeans_stats(stats)[1]
    elif relocated:
        inertia = float(torch.sum(torch.square(x - shift - centers[labels.long()])))
    else:
        inertia = _hip.kmeans_stats(stats)[1]        # unchanged labels gave unchanged centres: `last` is `labels`
    return labels, centers + shift, inertia, n_iter


def kmeans(X, n_clusters, *, max_iter=300, tol=1e-4, random_state=None, init=None):
    """scikit-learn's ``KMeans(n_clusters, n_init=1, max_iter=max_iter, tol=tol, random_state=random_state).fit(X)`` on the GPU:
    returns ``(labels, centers, inertia, n_iter)``.

    X: (N, F) ndarray of any float dtype -- computed in float64 (scikit-learn would stay in float32 for float32 input); int64
    labels and float64 centres come back as ndarrays -- or a float64 CUDA tensor, used in place (never modified: the column means
    are subtracted as the rows are read); int32 labels and the centres come back as CUDA tensors.  ``init``: None for k-means++,
    or a (K, F) array of centres.  The draws of k-means++ come from ``check_random_state(random_state)`` on the host in
    scikit-learn's order -- with ``random_state=None`` from numpy's global generator, exactly as a host fit consumes it --; per
    seeded centre the pots of its candidates are read back, per Lloyd iteration one 32-byte record.  An iteration that leaves a
    cluster empty relocates it as scikit-learn does.  1 <= F <= 128, 1 <= n_clusters <= 64 and n_clusters <= N.
    """
    K = int(n_clusters)
    x, was_tensor = _device_rows(X)
    N, F = x.shape
    _check_limits(F, K)
    if N < K:
        raise ValueError("n_samples=%d should be >= n_clusters=%d." % (N, K))
    if init is not None and tuple(np.shape(init) if not _is_tensor(init) else init.shape) != (K, F):
        raise ValueError("init must hold %d centres of %d features" % (K, F))
    if _is_tensor(init):
        init = init.detach().cpu().numpy()
    labels, centers, inertia, n_iter = _kmeans_device(x, K, max_iter, tol, random_state, init)
    if was_tensor:
        return labels, centers, inertia, n_iter
    return labels.cpu().numpy().astype(np.int64), centers.cpu().numpy(), inertia, n_iter


def _kmeans_start(x, K, reg_covar, random_state, ws):
    """(weights, means, covariances) on the device as GaussianMixture._initialize_parameters(init_params="kmeans") gives them:
    the one-hot responsibilities of the device k-means through the M-step, weights nk / N (not renormalised)."""
    torch = _hip.torch_mod()
    N = x.shape[0]
    labels = _kmeans_device(x, K, 300, 1e-4, random_state, None)[0].long()
    resp = torch.zeros((N, K), dtype=torch.float64, device=x.device)
    resp.scatter_(1, labels[:, None], 1.0)
    _, mu, cov = _hip.gmm_mstep(x, resp, reg_covar, workspace=ws)
    nk = torch.bincount(labels, minlength=K).to(torch.float64) + 10.0 * np.finfo(np.float64).eps
    return (nk / N).contiguous(), mu, cov


def fit_gaussian_mixture(X, n_components, *, max_iter=100, tol=1e-3, reg_covar=1e-6, init=None, random_state=None):
    """Fit a full-covariance Gaussian mixture by EM on the GPU; returns a fitted ``sklearn.mixture.GaussianMixture``.

    The loop is scikit-learn's: E-step, M-step, precisions, then one small read-back (the lower bound and the status words of the
    Cholesky factorisations); it stops when ``abs(change of the lower bound) < tol`` and warns (``ConvergenceWarning``) when
    ``max_iter > 0`` iterations end unconverged.  Sets ``weights_, means_, covariances_, precisions_cholesky_, precisions_,
    converged_, n_iter_, lower_bound_, lower_bounds_``.

    X: (N, F) ndarray of any float dtype -- computed and returned in float64 (scikit-learn would stay in float32 for float32
    input) -- or a float64 CUDA tensor, used in place.  ``init``: None (scikit-learn's own initialisation on the host:
    ``GaussianMixture(..., max_iter=0, random_state=random_state).fit(X)``, the same k-means draw a host fit would start from),
    ``"kmeans"`` (the same initialisation by :func:`kmeans` and the M-step on the device, from the same draws: X never leaves the
    device), a fitted ``GaussianMixture``, or a ``(weights, means, covariances)`` triple.  1 <= F <= 128, 1 <= n_components <= 64; a
    covariance that is not positive definite raises scikit-learn's ``ValueError``.
    """
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.mixture import GaussianMixture
    torch = _hip.torch_mod()
    K = int(n_components)
    x, was_tensor = _device_rows(X)
    N, F = x.shape
    _check_limits(F, K)
    if N < 1:
        raise ValueError("fit_gaussian_mixture needs at least one row")
    dev = x.device
    ws = _hip.gmm_workspace(dev, N, F, K)
    if isinstance(init, str):
        if init != "kmeans":
            raise ValueError("init must be None, 'kmeans', a fitted GaussianMixture or a (weights, means, covariances) triple; got %r"
                             % (init,))
        if N < K:
            raise ValueError("n_samples=%d should be >= n_components=%d." % (N, K))
        w, mu, cov = _kmeans_start(x, K, reg_covar, random_state, ws)
    else:
        w0, mu0, cov0 = _start(lambda: x.cpu().numpy() if was_tensor else np.ascontiguousarray(X, dtype=np.float64), K, reg_covar,
                               init, random_state)
        if mu0.shape[1] != F:
            raise ValueError("X has %d features, init has %d" % (F, mu0.shape[1]))
        w, mu, cov = _to_dev(w0, dev), _to_dev(mu0, dev), _to_dev(cov0, dev)

    U, log_det, status = _hip.gmm_precisions(cov)
    if bool(status.any().item()):
        raise ValueError(_ILL_DEFINED)
    lower, converged, n_iter, bounds = -np.inf, False, 0, []
    for n_iter in range(1, int(max_iter) + 1):
        prev = lower
        resp, _, _, mean = _hip.gmm_estep(x, w, mu, U, log_det, want_resp=True, want_mean=True, workspace=ws)
        w, mu, cov = _hip.gmm_mstep(x, resp, reg_covar, workspace=ws)
        U, log_det, status = _hip.gmm_precisions(cov)
        back = torch.cat((mean.reshape(1), status.to(torch.float64))).cpu().numpy()      # the iteration's one read-back
        if back[1:].any():
            raise ValueError(_ILL_DEFINED)
        lower = float(back[0])
        bounds.append(lower)
        if abs(lower - prev) < tol:
            converged = True
            break
    if not converged and max_iter > 0:
        warnings.warn("Best performing initialization did not converge. Try different init parameters, or increase max_iter, "
                      "tol, or check for degenerate data.", ConvergenceWarning)

    gmm = GaussianMixture(n_components=K, covariance_type="full", tol=tol, reg_covar=reg_covar, max_iter=max_iter,
                          random_state=random_state)
    gmm.weights_, gmm.means_, gmm.covariances_ = w.cpu().numpy(), mu.cpu().numpy(), cov.cpu().numpy()
    gmm.precisions_cholesky_ = U.cpu().numpy()
    gmm.precisions_ = gmm.precisions_cholesky_ @ gmm.precisions_cholesky_.transpose(0, 2, 1)
    gmm.converged_, gmm.n_iter_, gmm.lower_bound_, gmm.lower_bounds_ = converged, n_iter, lower, bounds
    gmm.n_features_in_ = F
    return gmm
