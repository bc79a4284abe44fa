"""tools/gvmlpg_model.py, the executable specification of MLPG with the gv likelihood (-m "not gpu"): the banded chunk-per-lane
form against the literal one, the gradient against central differences of the objective in long double, the starts, the
degenerate systems, the ascent under the derived step, the status of a too-large step, and the padded-batch rules."""
import numpy as np
import pytest

import gvmlpg_cases as C
from gvmlpg_cases import GV

LENGTHS = [1, 2, 3, 5, 63, 64, 65, 130]
MODES = [GV.VAR_FRAME, GV.VAR_GLOBAL, GV.VAR_UNIT]


def one_system(T, wname, mode, tight=False, seed=0):
    """(mu, tau, windows, y0, mu_v, p_v) of the one system of a (1, T, 1) case."""
    case = C.make_case(seed + T, 1, T, 1, wname, mode, np.float64, None, tight)
    win = case["windows"]
    mu = np.stack([case["mean"][0, :, w] for w in range(len(win))])
    tau = GV.precisions(case["var"][0] if mode == GV.VAR_FRAME else case["var"], mode, win, T, 1, 0)
    return mu, tau, win, case["y_in"][0, :, 0].copy(), case["gv_mean"][0], case["gv_prec"][0]


@pytest.mark.parametrize("wname", ["std2", "std3", "static"])
@pytest.mark.parametrize("mode", MODES)
def test_banded_form_equals_literal_form(wname, mode):
    for T in LENGTHS:
        mu, tau, win, y0, mu_v, p_v = one_system(T, wname, mode)
        P, r = GV.system_literal(mu, tau, win)
        pk, rb = GV.system_banded(mu, tau, win)
        scale = np.abs(P).max()
        assert np.abs(GV.band_to_dense(pk) - P).max() <= 1e-14 * scale and np.abs(rb - r).max() <= 1e-14 * max(np.abs(r).max(), 1e-300)
        for init in (0, 1):
            ya, ra, sa = GV.ascend_literal(P, r, y0, mu_v, p_v, n_iter=100, init=init)
            yb, rb_, sb = GV.ascend_banded(pk, rb, y0, mu_v, p_v, n_iter=100, init=init)
            assert np.abs(ya - yb).max() <= 1e-12 * np.abs(ya).max(), (T, init)
            assert sa == sb == 0
            assert np.abs(ra - rb_).max() <= 1e-10 * max(np.abs(ra).max(), 1e-300)


@pytest.mark.parametrize("T", [2, 3, 5, 64])
def test_gradient_is_the_derivative_of_the_objective(T):
    """Central differences of L in long double pin the formula of g independently of the iteration."""
    mu, tau, win, y0, mu_v, p_v = one_system(T, "std3", GV.VAR_FRAME)
    ld = np.longdouble
    P, r = GV.system_literal(mu, tau, win, ld)
    rng = np.random.RandomState(T)
    y = (y0 + 0.2 * rng.randn(T)).astype(ld)         # away from the stationary point
    g = GV.gradient(P, r, y, ld(mu_v), ld(p_v), 1.7)
    h = ld(2.0) ** -24
    for t in range(T):
        e = np.zeros(T, dtype=ld)
        e[t] = h
        fd = (GV.objective(P, r, y + e, ld(mu_v), ld(p_v), 1.7) - GV.objective(P, r, y - e, ld(mu_v), ld(p_v), 1.7)) / (2 * h)
        assert abs(fd - g[t]) <= 1e-9 * max(np.abs(g).max(), 1.0), (t, fd, g[t])
    # and the banded product under it is the dense one
    pk, _ = GV.system_banded(mu, tau, win)
    py, rows = GV._band_apply(pk[0], pk[1], pk[2], y0)
    Pd = GV.band_to_dense(pk)
    assert np.abs(py - Pd @ y0).max() <= 1e-14 * np.abs(Pd).max() * np.abs(y0).max()
    assert np.allclose(rows, np.abs(Pd).sum(axis=1), rtol=1e-15, atol=0)


def test_starts():
    mu, tau, win, y0, mu_v, p_v = one_system(65, "std3", GV.VAR_FRAME)
    pk, r = GV.system_banded(mu, tau, win)
    P = GV.band_to_dense(pk)
    for asc, A in ((GV.ascend_banded, pk), (GV.ascend_literal, P)):
        y, rep, st = asc(A, r, y0, mu_v, p_v, n_iter=0, init=0)
        assert np.array_equal(y, y0) and st == 0 and rep[0] == rep[1] and rep[2] == rep[3]
        y, rep, st = asc(A, r, y0, mu_v, p_v, n_iter=0, init=1)
        assert abs(y.var() - mu_v) <= 1e-13 * mu_v and abs(rep[3] - mu_v) <= 1e-13 * mu_v and st == 0
        assert abs(y.mean() - y0.mean()) <= 1e-14 * np.abs(y0).max()
        assert abs(rep[2] - y0.var()) <= 1e-14 * y0.var()


@pytest.mark.parametrize("init", [0, 1])
def test_degenerate_systems_do_not_divide_by_zero(init):
    with np.errstate(all="raise"):
        # T = 1: v is 0 whatever y is
        mu, tau, win, y0, mu_v, p_v = one_system(1, "std3", GV.VAR_FRAME)
        pk, r = GV.system_banded(mu, tau, win)
        y, rep, st = GV.ascend_banded(pk, r, y0, mu_v, p_v, n_iter=100, init=init)
        assert st == 0 and np.isfinite(y).all() and rep[2] == 0 and rep[3] == 0
        assert abs(y[0] - y0[0]) <= 1e-12 * abs(y0[0])          # y0 solves P y = r and the gv term has no gradient at T = 1
        # a constant trajectory: v(y0) = 0, the scaled start leaves it alone
        mu, tau, win, _, mu_v, p_v = one_system(5, "std2", GV.VAR_UNIT)
        pk, r = GV.system_banded(mu, tau, win)
        y0 = np.full(5, 0.7)
        for asc, A in ((GV.ascend_banded, pk), (GV.ascend_literal, GV.band_to_dense(pk))):
            y, rep, st = asc(A, r, y0, mu_v, p_v, n_iter=3, init=init)
            assert st == 0 and np.isfinite(y).all() and rep[2] == 0
        # mu_v = 0: no scaling either
        y, rep, st = GV.ascend_banded(pk, r, np.arange(5.0), 0.0, p_v, n_iter=0, init=init)
        assert np.array_equal(y, np.arange(5.0))


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("wname", ["std2", "std3", "static"])
def test_derived_step_ascends_and_moves_the_gv_towards_its_mean(wname, tight):
    for T in LENGTHS:
        for mode in MODES:
            mu, tau, win, y0, mu_v, p_v = one_system(T, wname, mode, tight)
            pk, r = GV.system_banded(mu, tau, win)
            for init in (0, 1):
                y, rep, st, Ls = GV.ascend_banded(pk, r, y0, mu_v, p_v, n_iter=100, init=init, trace=True)
                assert st == 0, (T, mode, init)
                slack = GV.SLACK * np.maximum(np.abs(Ls[1:]), np.abs(Ls[:-1]))
                assert (Ls[1:] >= Ls[:-1] - slack).all(), (T, mode, init)
                assert abs(rep[3] - mu_v) <= abs(rep[2] - mu_v), (T, mode, init)


def test_a_step_far_too_large_is_reported():
    for T in (3, 65, 130):
        mu, tau, win, y0, mu_v, p_v = one_system(T, "std3", GV.VAR_FRAME)
        pk, r = GV.system_banded(mu, tau, win)
        P = GV.band_to_dense(pk)
        omega = 1.0 / (2 * T)
        m, v = GV.mean_var(y0)
        for init in (0, 1):
            vs = mu_v if init else v
            derived = GV.derived_step(np.abs(P).sum(axis=1).max(), T, omega, p_v, vs, mu_v)
            for asc, A in ((GV.ascend_banded, pk), (GV.ascend_literal, P)):
                assert asc(A, r, y0, mu_v, p_v, n_iter=100, step=50 * derived, init=init)[2] in (1, 2), (T, init)
                assert asc(A, r, y0, mu_v, p_v, n_iter=100, step=derived, init=init)[2] == 0


def test_padded_batch_rules():
    lengths = [70, 0, 1, 69, 33]
    case = C.make_case(1, 5, 70, 3, "std3", GV.VAR_FRAME, np.float64, lengths)
    y, rep, st = C.model(case, 20)
    live = GV.live_frames(lengths, 5, 70)
    pad = np.arange(70)[None, :] >= live[:, None]
    assert (y[pad] == 0).all() and (rep[1] == 0).all() and (st == 0).all()
    yl = C.model(case, 20, form="literal")[0]
    assert np.abs(y - yl).max() <= 1e-12 * np.abs(y).max()
    # a system's bits depend on its own live frames alone: other garbage in the pad frames, another batch around it
    other = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    for k in ("mean", "var", "y_in"):
        other[k][pad] = 7.5
    assert np.array_equal(C.model(other, 20)[0], y)
    sub = dict(case, mean=case["mean"][3:4, :69], var=case["var"][3:4, :69], y_in=case["y_in"][3:4, :69], lengths=None, B=1, Tmax=69)
    ys, reps, _ = C.model(sub, 20)
    assert np.array_equal(ys[0], y[3, :69]) and np.array_equal(reps[0], rep[3])
    # lengths are clipped to [0, Tmax]
    assert np.array_equal(GV.live_frames([-3, 99, 5], 3, 70), [0, 70, 5])
    # float32 storage: float32 reciprocals, float64 arithmetic, float32 result
    c32 = C.make_case(1, 2, 33, 2, "std2", GV.VAR_GLOBAL, np.float32, [33, 20])
    y32 = C.model(c32, 10)[0]
    assert y32.dtype == np.float32
    tau = GV.precisions(c32["var"], GV.VAR_GLOBAL, c32["windows"], 33, 2, 1)
    assert tau[0, 5] == np.float64(np.float32(1) / c32["var"][1]) and tau[1, 0] == 0 and tau[1, 32] == 0 and tau[0, 0] != 0
    # the gv of a padded batch
    g = GV.gv_padded(case["y_in"], lengths)
    assert (g[1] == 0).all() and (g[2] == 0).all() and np.allclose(g[3], case["y_in"][3, :69].var(axis=0), rtol=1e-14)
