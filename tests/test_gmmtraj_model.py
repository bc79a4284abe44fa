"""tools/gmmtraj_model.py, the numpy specification of batched trajectory GMM conversion (-m "not gpu"): its table form against
the literal per-frame form of the reference's baseline/gmm.py:225-244, the padded-batch rules of mlpg_hip_gmm_trajectory_stats,
and its transform_batch against goldens the reference produced (MLPG there by the model's own dense normal equations)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gmmtraj_model as GM  # noqa: E402
from cases import WINDOW_SETS, gmm_joint_data  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "align_golden.npz"))


def _gmm_from(golden, key):
    from sklearn.mixture import GaussianMixture
    w = golden[key + "/weights"]
    g = GaussianMixture(n_components=len(w), covariance_type="full")
    g.weights_, g.means_, g.covariances_ = w, golden[key + "/means"], golden[key + "/covariances"]
    return g


def random_model(M, D, seed):
    rng = np.random.RandomState(seed)
    F = 2 * D
    Q = rng.randn(M, F, F) / np.sqrt(F)
    cov = Q @ Q.transpose(0, 2, 1) + 0.3 * np.eye(F)
    cov = 0.5 * (cov + cov.transpose(0, 2, 1))
    mu = rng.randn(M, F)
    return mu[:, :D], mu[:, D:], cov[:, :D, :D], cov[:, :D, D:], cov[:, D:, :D], cov[:, D:, D:]


@pytest.mark.parametrize("M,D,T", [(1, 1, 5), (3, 6, 40), (8, 72, 30), (5, 17, 70)])
def test_table_form_agrees_with_the_literal_form(M, D, T):
    mu_x, mu_y, cxx, cxy, cyx, cyy = random_model(M, D, 11 * M + D)
    rng = np.random.RandomState(T)
    labels = rng.randint(M, size=T)
    x = mu_x[labels] + rng.randn(T, D)
    E, Dv = GM.stats_literal(x, labels, mu_x, mu_y, cxx, cxy, cyx, cyy)
    A, cvar = GM.tables(cxx, cxy, cyx, cyy)
    mean, var = GM.stats_table(x, labels, mu_x, mu_y, A, cvar)
    err = np.abs(mean - E).max() / np.abs(E).max()
    print("table against literal, M %d D %d: %.2e of the maximum" % (M, D, err))
    assert err <= 1e-10
    assert np.array_equal(var, Dv)            # the same three operations on the same diagonals
    S = GM.error_scale(x, labels, mu_x, mu_y, A)
    assert S.shape == mean.shape and (S >= np.abs(mean) * (1 - 1e-12)).all()


def test_padded_batch_rules():
    M, D, B, T = 3, 4, 3, 7
    mu_x, mu_y, cxx, cxy, cyx, cyy = random_model(M, D, 5)
    A, cvar = GM.tables(cxx, cxy, cyx, cyy)
    rng = np.random.RandomState(0)
    x = rng.randn(B, T, D)
    lengths = np.array([7, 0, 3])
    labels = rng.randint(M, size=(B, T))
    labels[0, 2] = M          # a live row with a bad label
    labels[0, 5] = -1
    labels[2, 3:] = 99        # pad rows: never looked at
    labels[1, :] = -7
    xp = x.copy()
    xp[1] = np.nan            # pad rows' x is not read
    xp[2, 3:] = np.inf
    mean, var = GM.stats_padded(xp, lengths, labels, mu_x, mu_y, A, cvar)
    live = np.arange(T)[None] < lengths[:, None]
    assert (mean[~live] == 0).all() and (var[~live] == 1).all()
    assert np.isnan(mean[0, 2]).all() and np.isnan(var[0, 2]).all() and np.isnan(mean[0, 5]).all() and np.isnan(var[0, 5]).all()
    ok = live.copy()
    ok[0, 2] = ok[0, 5] = False
    m2, v2 = GM.stats_table(x[ok], labels[ok], mu_x, mu_y, A, cvar)
    assert np.array_equal(mean[ok], m2) and np.array_equal(var[ok], v2) and np.isfinite(m2).all()
    # lengths outside [0, Tmax] are clipped; None means every row is live
    assert np.array_equal(GM.live_frames([-3, 99], 2, 5), [0, 5]) and np.array_equal(GM.live_frames(None, 2, 5), [5, 5])
    # a row does not depend on its neighbours: the flattened rows in another order
    perm = rng.permutation(int(ok.sum()))
    m3, _ = GM.stats_table(x[ok][perm], labels[ok][perm], mu_x, mu_y, A, cvar)
    assert np.array_equal(m3, m2[perm])


def test_dense_mlpg_of_static_windows_is_the_mean():
    rng = np.random.RandomState(1)
    mean, var = rng.randn(9, 4), rng.rand(9, 4) + 0.5
    np.testing.assert_allclose(GM.mlpg_dense(mean, var, WINDOW_SETS["static"]), mean, rtol=1e-13, atol=0)
    assert GM.mlpg_dense(mean[:0], var[:0], WINDOW_SETS["std2"]).shape == (0, 2)


@pytest.mark.parametrize("wname", ["std2", "std3"])
def test_transform_batch_reproduces_the_reference_goldens(golden, wname):
    from nnmnkwii_amd.baseline.gmm import MLPG
    windows = WINDOW_SETS[wname]
    _, src = gmm_joint_data(wname, 3)
    gmm = _gmm_from(golden, "gmm/%s" % wname)
    for swap in (False, True):
        for diff in (False, True):
            ref = golden["gmm/%s/y-swap%d-diff%d" % (wname, swap, diff)]
            g = MLPG(gmm, windows=windows, swap=swap, diff=diff)      # the constructor is host arithmetic only
            A, cvar = GM.tables(g.covarXX, g.covarXY, g.covarYX, g.covarYY)
            # the utterance alone, and between a longer and an empty one: the padding changes nothing
            other = np.concatenate([src, src[::-1]])[:47]
            for utts, at in (([src], 0), ([other, src, src[:0]], 1)):
                got = GM.transform_batch(utts, g.px.predict, g.src_means, g.tgt_means, A, cvar, windows)
                assert [len(y) for y in got] == [len(u) for u in utts]
                y = got[at]
                assert y.shape == ref.shape and y.dtype == np.float64
                np.testing.assert_allclose(y, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
    assert GM.transform_batch([], None, None, None, None, None, windows) == []
