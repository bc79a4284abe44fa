"""tools/norm_model.py, the executable specification of corpus normalisation (-m "not gpu"): its literal form against what the
reference gave (tests/golden/norm_golden.npz), its kernel form against the exact truth within the error scales, streaming
through the state in 1, 2 and B pieces, exact constant columns, the NaN rules, and the apply kernel's form against the
reference's scalers bit for bit."""
import numpy as np
import pytest

import norm_cases as C
from norm_cases import NM

G = C.golden()
F64_CASES = ["probe64", "blocks64"]


def utterances(name):
    X, L = G[name + "/X"], G[name + "/lengths"]
    return [X[b, :L[b]] for b in range(len(L))]


@pytest.mark.parametrize("name", F64_CASES)
def test_literal_form_against_the_reference(name):
    """Both are the definition evaluated in float64 in another order: each within its own distance of the truth."""
    utts = utterances(name)
    mean, var, count = NM.literal_meanvar(utts)
    assert count == int(G[name + "/count"])
    truth = NM.exact(G[name + "/X"], G[name + "/lengths"])
    lit = NM.ratios(mean, var, truth, skip_zero_scale=True)
    ref = G[name + "/ref_ratio"]
    print("literal form %s, reference %s of (S_mean, S_var)" % (lit, ref))
    live = (truth["s_mean"] > 0), (truth["s_var"] > 0)
    assert (np.abs(mean - G[name + "/mean"])[live[0]] <= ((lit[0] + ref[0]) * truth["s_mean"])[live[0]]).all()
    assert (np.abs(var - G[name + "/var"])[live[1]] <= ((lit[1] + ref[1]) * truth["s_var"])[live[1]]).all()
    mn, mx = NM.literal_minmax(utts)
    assert np.array_equal(mn, G[name + "/min"]) and np.array_equal(mx, G[name + "/max"])
    # continued from the reference's own (mean_, var_, last_sample_count)
    m3, v3, c3 = NM.literal_meanvar(utts[2:], G[name + "/prior_mean"], G[name + "/prior_var"], int(G[name + "/prior_count"]))
    assert c3 == int(G[name + "/streamed_count"])
    assert (np.abs(m3 - G[name + "/streamed_mean"])[live[0]] <= ((lit[0] + ref[0]) * truth["s_mean"])[live[0]]).all()
    assert (np.abs(v3 - G[name + "/streamed_var"])[live[1]] <= ((lit[1] + ref[1]) * truth["s_var"])[live[1]]).all()


@pytest.mark.parametrize("name", ["probe64", "probe32", "blocks64", "arctic"])
def test_kernel_form_against_the_truth(name):
    X, L = G[name + "/X"], G[name + "/lengths"]
    state = NM.kernel_state(X, L)
    truth = NM.exact(X, L)
    count, mean, var, mn, mx = NM.stats_of(state)
    r = NM.ratios(mean, var, truth)                       # constant columns included: a miss there is infinite
    print("kernel form against the truth: %.3f S_mean, %.3f S_var" % r)
    assert count == int(G[name + "/count"]) and max(r) <= C.WORST_RATIO
    assert np.array_equal(mn, G[name + "/min"]) and np.array_equal(mx, G[name + "/max"])
    for k, const in C.CONSTANT.items():
        for d in range(k, X.shape[2], len(C.COLUMNS)):
            assert mean[d] == X.dtype.type(const) and var[d] == 0.0
    if X.dtype == np.float32:                              # the reference answers in float32 there: one float32 ulp apart at most
        const = np.array([d for k in C.CONSTANT for d in range(k, X.shape[2], len(C.COLUMNS))], dtype=np.int64)
        other = np.setdiff1d(np.arange(X.shape[2]), const)   # (the reference's variance of a constant column is not exact)
        assert (np.abs(mean.astype(np.float32) - G[name + "/mean"]) <= np.spacing(np.abs(G[name + "/mean"]))).all()
        assert (np.abs(var.astype(np.float32) - G[name + "/var"])[other] <= np.spacing(np.abs(G[name + "/var"]))[other]).all()


def test_streaming_in_one_two_and_B_pieces():
    X, L = G["blocks64/X"], G["blocks64/lengths"]
    truth = NM.exact(X, L)
    whole = NM.kernel_state(X, L)
    two = NM.kernel_state(X[2:], L[2:], NM.kernel_state(X[:2], L[:2]))
    each = None
    for b in range(len(L)):
        each = NM.kernel_state(X[b:b + 1], L[b:b + 1], each)
    for st in (whole, two, each):
        assert C.stats_ok(st, truth, 2 * C.WORST_RATIO)
        assert np.array_equal(st[0], whole[0]) and np.array_equal(st[3:], whole[3:])
    # from the reference's (mean_, var_, last_sample_count)
    prior = NM.state_from(G["blocks64/prior_mean"], G["blocks64/prior_var"], int(G["blocks64/prior_count"]), X.shape[2])
    st = NM.kernel_state(X[2:], L[2:], prior)
    live = truth["s_var"] > 0
    bound = C.WORST_RATIO + G["blocks64/ref_ratio"]
    assert st[0, 0] == truth["count"]
    assert (np.abs(st[1] - G["blocks64/streamed_mean"])[live] <= (bound[0] * truth["s_mean"])[live]).all()
    assert (np.abs(st[2] / st[0] - G["blocks64/streamed_var"])[live] <= (bound[1] * truth["s_var"])[live]).all()
    # a batch without a live frame hands the state through; without a state it is the empty one
    assert np.array_equal(NM.kernel_state(X, np.zeros_like(L), whole), whole)
    assert np.array_equal(NM.kernel_state(X, np.zeros_like(L)), NM.empty_state(X.shape[2]))


@pytest.mark.parametrize("const", [0.1, 1e4 + 0.3, -7.25, 0.0])
@pytest.mark.parametrize("lengths", [[1], [C.CHUNK + 1, 3], [C.BLOCK + 1, 0, 77]])
def test_constant_columns_are_exact(const, lengths):
    X = np.full((len(lengths), max(lengths), 3), np.nan)
    for b, n in enumerate(lengths):
        X[b, :n] = const
    count, mean, var, mn, mx = NM.stats_of(NM.kernel_state(X, lengths))
    assert count == sum(lengths) and (mean == const).all() and (var == 0.0).all() and (mn == const).all() and (mx == const).all()
    # ... and stay so through a state that holds the same constant
    st = NM.kernel_state(X, lengths, NM.kernel_state(X, lengths))
    assert (st[1] == const).all() and (st[2] == 0.0).all() and st[0, 0] == 2 * sum(lengths)


def test_nan_rules():
    X, L = C.padded(5, [40, 70], 4)
    X[0, 3, 0] = np.nan                 # the workgroup's first chunk
    X[1, 69, 1] = np.nan                # the last live frame
    X[1, 20, 2] = -np.inf
    count, mean, var, mn, mx = NM.stats_of(NM.kernel_state(X, L))
    live = np.concatenate([X[0, :40], X[1, :70]])
    assert count == 110
    assert np.isnan(mean[:3]).all() and np.isnan(var[:3]).all() and np.isfinite([mean[3], var[3]]).all()
    # np.minimum / np.maximum: NaN propagates (fmin / fmax would drop it), infinities are ordinary values
    assert np.array_equal(mn, np.minimum.reduce(live), equal_nan=True) and np.array_equal(mx, np.maximum.reduce(live), equal_nan=True)
    assert np.isnan(mn[:2]).all() and mn[2] == -np.inf and np.isfinite(mx[2])
    # pad frames hold NaN in C.padded: none of it arrived in column 3


@pytest.mark.parametrize("name", ["probe64", "probe32", "arctic"])
def test_apply_form_against_the_reference(name):
    X, L = G[name + "/X"], G[name + "/lengths"]
    x = X[1:2, :L[1]]
    mean, std, mn, mx = (G[name + "/" + k] for k in ("mean", "std", "min", "max"))
    min_, scale_ = G[name + "/min_"], G[name + "/scale_"]
    pairs = [("scale", 0, std, mean), ("inv_scale", 1, std, mean), ("minmax_scale", 1, scale_, min_),
             ("minmax_scale_params", 1, scale_, min_), ("inv_minmax_scale", 0, scale_, min_), ("inv_minmax_scale_params", 0, scale_, min_)]
    for key, mode, a, c in pairs:
        ref = G[name + "/" + key]
        y = NM.affine(x, a, c, mode)[0]
        if X.dtype == np.float64:
            assert np.array_equal(y, ref), key                       # separate operations in numpy's order: the same bits
        else:                                                        # numpy computed in float32, the model in float64
            ax = np.abs(a.astype(np.float64) * x[0].astype(np.float64))
            tol = 2 * 2.0 ** -23 * np.abs(y) if mode == 0 else 2.0 ** -23 * (ax + np.abs(y))
            assert (np.abs(y.astype(np.float32).astype(np.float64) - ref) <= tol).all(), key
    # pad rows are exact zeros
    y = NM.affine(X, std, mean, 0, L)
    assert all((y[b, L[b]:] == 0).all() for b in range(len(L)))
