"""Float64 numpy reference of the k-means start of a Gaussian mixture: scikit-learn's KMeans(n_init=1) -- k-means++ seeding, Lloyd
iterations, the relocation of empty clusters (sklearn/cluster/_kmeans.py: KMeans.fit, _kmeans_plusplus, _kmeans_single_lloyd,
_tolerance; _k_means_common.pyx: _relocate_empty_clusters_dense) -- and GaussianMixture._initialize_parameters
(sklearn/mixture/_base.py:98-141) restated, with squared distances taken as the direct sum over the features as the device does.
tests/test_kmeans64_cpu.py pins it on scikit-learn itself; tests/test_kmeans_gpu.py and tests/test_kmeans_host_cpu.py check the
HIP kernels against it."""
import numpy as np
from sklearn.utils import check_random_state

import gmm_em64


def sqdist(X, c):
    """sum_f (x_nf - c_f)^2 for every row, the direct form."""
    return np.sum(np.square(X - c), axis=1)


def seed_step(Xc, cand, closest=None):
    """(d (C, N), pots (C)): d[j][n] = min(closest[n], |x_n - x_cand[j]|^2) on centred rows."""
    d = np.stack([sqdist(Xc, Xc[j]) for j in cand])
    if closest is not None:
        d = np.minimum(closest, d)
    return d, d.sum(axis=1)


def kmeans_plusplus(Xc, K, rs):
    """(centres (K, F), indices (K)) of k-means++ on centred rows, the draws taken from ``rs`` in scikit-learn's order."""
    N = Xc.shape[0]
    trials = 2 + int(np.log(K))
    idx = np.empty(K, dtype=np.int64)
    idx[0] = rs.choice(N, p=np.ones(N) / N)
    d, pots = seed_step(Xc, [idx[0]])
    closest, pot = d[0], pots[0]
    for c in range(1, K):
        rand = rs.uniform(size=trials) * pot
        cand = np.clip(np.searchsorted(np.cumsum(closest), rand), None, N - 1)
        d, pots = seed_step(Xc, cand, closest)
        best = int(np.argmin(pots))
        closest, pot, idx[c] = d[best], pots[best], cand[best]
    return Xc[idx].copy(), idx


def assign(Xc, centers):
    """Labels: the arg-min over k of |c_k|^2 - 2 x.c_k, the first of equals; and the gap between the best and the second best of
    these as a share of the largest |value| (inf for K == 1)."""
    v = np.sum(np.square(centers), axis=1) - 2.0 * (Xc @ centers.T)
    labels = np.argmin(v, axis=1).astype(np.int32)
    if centers.shape[0] == 1:
        return labels, np.full(Xc.shape[0], np.inf)
    two = np.partition(v, 1, axis=1)
    return labels, (two[:, 1] - two[:, 0]) / max(np.max(np.abs(v)), np.finfo(np.float64).tiny)


def relocate(Xc, centers_old, labels, sums, counts):
    """_relocate_empty_clusters_dense on the unaveraged sums and the counts, in place; the number of empty clusters."""
    empty = np.flatnonzero(counts == 0)
    if empty.size:
        dist = sqdist(Xc, centers_old[labels])
        far = np.argpartition(dist, -empty.size)[:-empty.size - 1:-1]
        for new, n in zip(empty, far):
            old = labels[n]
            sums[old] -= Xc[n]
            sums[new] = Xc[n]
            counts[new] = 1
            counts[old] -= 1
    return empty.size


def lloyd_step(Xc, centers, labels_prev, update=True):
    """One Lloyd iteration on centred rows: dict(labels, min_dist, sums, counts, centers, shift, changed, empty, inertia).  sums and
    counts are the plain per-cluster ones (before any relocation); centers, shift: after it (update=False: the old centres, 0)."""
    K = centers.shape[0]
    labels, _ = assign(Xc, centers)
    min_dist = sqdist(Xc, centers[labels])
    sums = np.zeros_like(centers)
    np.add.at(sums, labels, Xc)
    counts = np.bincount(labels, minlength=K).astype(np.float64)
    out = dict(labels=labels, min_dist=min_dist, sums=sums, counts=counts, changed=int(np.sum(labels != labels_prev)),
               empty=int(np.sum(counts == 0)), inertia=float(min_dist.sum()), centers=centers, shift=0.0)
    if update:
        s, c = sums.copy(), counts.copy()
        relocate(Xc, centers, labels, s, c)
        new = np.where(c[:, None] > 0, s / np.where(c > 0, c, 1.0)[:, None], s)
        out["centers"], out["shift"] = new, float(np.sum(np.square(new - centers)))
    return out


def lloyd(Xc, centers, tol_abs, max_iter=300):
    """(labels, centres, inertia, n_iter) of _kmeans_single_lloyd on centred rows."""
    labels_prev = np.full(Xc.shape[0], -1, dtype=np.int32)
    strict, n_iter = False, 0
    labels = labels_prev
    for n_iter in range(1, max_iter + 1):
        st = lloyd_step(Xc, centers, labels_prev)
        labels, centers = st["labels"], st["centers"]
        if st["changed"] == 0:
            strict = True
            break
        if st["shift"] <= tol_abs:
            break
        labels_prev = labels
    if not strict:
        labels, _ = assign(Xc, centers)
    return labels, centers, float(sqdist(Xc, centers[labels]).sum()), n_iter


def kmeans(X, K, random_state=None, init=None, max_iter=300, tol=1e-4):
    """(labels (N) int32, centres (K, F), inertia, n_iter) of KMeans(K, n_init=1, init=..., random_state=...).fit(X)."""
    X = np.asarray(X, dtype=np.float64)
    rs = check_random_state(random_state)
    tol_abs = np.mean(np.var(X, axis=0)) * tol
    mean = X.mean(axis=0)
    Xc = X - mean
    centers = kmeans_plusplus(Xc, K, rs)[0] if init is None else np.array(init, dtype=np.float64) - mean
    labels, centers, inertia, n_iter = lloyd(Xc, centers, tol_abs, max_iter)
    return labels, centers + mean, inertia, n_iter


def mixture_start(X, labels, K, reg_covar=1e-6):
    """(weights, means, covariances) GaussianMixture._initialize gives for the one-hot responsibilities of ``labels``."""
    X = np.asarray(X, dtype=np.float64)
    resp = np.zeros((X.shape[0], K))
    resp[np.arange(X.shape[0]), labels] = 1.0
    nk = resp.sum(axis=0) + 10 * np.finfo(np.float64).eps
    _, means, cov = gmm_em64.m_step(X, resp, reg_covar)
    return nk / X.shape[0], means, cov


def aligner_like(N, F, seed, zero_share):
    """Concatenated 200-frame random walks with a share of the rows exactly zero (the aligner fits on its zero padding too)."""
    rng = np.random.RandomState(seed)
    X = np.concatenate([np.cumsum(rng.randn(200, F), axis=0) * 0.1 + rng.randn(F) for _ in range((N + 199) // 200)])[:N]
    X[rng.rand(N) < zero_share] = 0.0
    return X


# (N, F, K, seed, zero share)
DATA_SETS = [(4000, 50, 16, 0, 0.3), (4000, 50, 16, 1, 0.3), (4000, 50, 16, 2, 0.3), (4000, 50, 16, 3, 0.3), (2000, 10, 4, 1, 0.0),
             (3000, 128, 3, 2, 0.3), (1000, 2, 64, 3, 0.1), (600, 1, 5, 4, 0.0)]


def relocation_case():
    """(X, init): three clusters of rows and four initial centres, the last far from every row, so that exactly one cluster is
    empty in the first iteration."""
    rng = np.random.RandomState(11)
    X = np.concatenate([rng.randn(60, 3) + m for m in ([0, 0, 0], [6, 0, 0], [0, 7, 1])])
    init = np.array([[0.0, 0, 0], [6, 0, 0], [0, 7, 1], [500, 500, 500]])
    return X, init


def step_case(N, F, K, C, seed):
    """Inputs of one seed step and one Lloyd step: randn rows with every column on its own scale and off zero, a non-zero shift,
    C candidate rows, a closest-distance vector, K centres and previous labels.  dict(X, shift, cand, closest, centers, prev)."""
    rng = np.random.RandomState(seed)
    scales = rng.permutation(np.linspace(0.5, 3.0, F))
    X = (rng.randn(N, F) + 0.7) * scales
    shift = X.mean(axis=0) + 0.1 * rng.randn(F) * scales
    Xc = X - shift
    return dict(X=X, shift=shift, cand=rng.randint(N, size=C), closest=sqdist(Xc, Xc[rng.randint(N)]),
                centers=Xc[rng.randint(N, size=K)] + 0.3 * rng.randn(K, F) * scales, prev=rng.randint(K, size=N).astype(np.int32))


def step_expected(case):
    """What the device's Lloyd step gives on a step_case: lloyd_step's plain results, the rows whose label is clear (best and
    second best more than 1e-9 of the largest value apart), and -- the step itself relocates nothing -- the averaged centres where
    the count is positive (the old centre elsewhere) with their shift."""
    Xc, centers = case["X"] - case["shift"], case["centers"]
    st = lloyd_step(Xc, centers, case["prev"], update=False)
    st["clear"] = assign(Xc, centers)[1] > 1e-9
    c = st["counts"]
    st["centers"] = np.where(c[:, None] > 0, st["sums"] / np.where(c > 0, c, 1.0)[:, None], centers)
    st["shift"] = float(np.sum(np.square(st["centers"] - centers)))
    return st


def check_step(case, ref, got):
    """Assert one Lloyd step's results (dict: labels, min_dist, sums, counts, centers, shift, inertia, changed, empty; centers and
    shift may be missing) against step_expected's, with the bounds of the GPU test; prints every figure first."""
    clear = ref["clear"]
    print("left out %d of %d rows" % (np.sum(~clear), len(clear)))
    assert np.sum(~clear) == 0                                   # the reference leaves out no row on this data
    assert np.mean(got["labels"][clear] != ref["labels"][clear]) == 0 and np.mean(got["labels"] != ref["labels"]) <= 0.01
    for name in ("min_dist", "sums", "centers", "shift", "inertia"):
        if name in got and got[name] is not None:
            e = dist(got[name], ref[name]) if np.max(np.abs(ref[name])) > 0 else float(np.max(np.abs(got[name])))
            print("%s %.2e" % (name, e))
            assert e <= 1e-10, (name, e)
    assert np.array_equal(got["counts"], ref["counts"]) and got["empty"] == ref["empty"]
    assert got["changed"] == int(np.sum(got["labels"] != case["prev"])) == ref["changed"]


dist = gmm_em64.dist
