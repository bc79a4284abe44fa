"""Corpus normalisation on the device: the kernels of mlpg_hip_column_stats and mlpg_hip_column_affine (csrc/colstats.hip)
against the numpy specification tools/norm_model.py through the C entries on guarded buffers at element offsets 0 and 1 and with
row strides above D, then the functions of ``nnmnkwii_amd.preprocessing`` end to end against what the reference gave
(tests/golden/norm_golden.npz).

Bounds (tests/norm_cases.py; S_mean = eps mean|x|, S_var = eps (var + |mean| sigma) from the exact truth).  Count, min, max:
equal.  Constant columns: mean == the constant, var == 0.  Kernel against the model's kernel form: the same bits -- every
operation is a separately rounded IEEE operation in the same order, the divisions included, and the host build of the kernel
text measured 0 ulp (tests/test_norm_host_cpu.py).  Against the truth: 8 WORST_RATIO scales.  Against the reference's values:
8 (WORST_RATIO + the reference's own ratio) scales.  Apply: the model's bits (float64 arithmetic, one rounding), which for
float64 output are the reference's; float32 x with float32 statistics against the reference, which computed in float32:
mode 0 |d| <= 2 2^-23 |y|, mode 1 |d| <= 2^-23 (|a x| + |y|).  Pad rows exactly 0, guard bands intact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import norm_cases as C
from embed import Embedded, Workspace, embedded, failed
from norm_cases import NM

pytestmark = pytest.mark.gpu

G = C.golden()
WINDOWS = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]


def _lib():
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts():
    L = _lib()
    return [L.mlpg_hip_launch_count(k) for k in range(44)]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def _wide(X, ld, fill):
    W = np.full(X.shape[:2] + (ld,), fill, dtype=X.dtype)
    W[:, :, :X.shape[2]] = X
    return W


p = lambda b: None if b is None else ctypes.c_void_p(b.ptr())  # noqa: E731


def run_stats(X, lengths, state=None, off=0, ld=None, in_place=False):
    """One call of mlpg_hip_column_stats on guarded buffers (the columns past D and the pad frames hold NaN).  Returns state_out
    as numpy; checks the return code, the guards, that the inputs are unchanged and that one call of kind 39 was counted."""
    from nnmnkwii_amd import _hip
    L = _lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, Tmax, D = X.shape
    ld = D if ld is None else ld
    ins = dict(x=embedded(_wide(X, ld, np.nan), off))
    if lengths is not None:
        ins["lengths"] = embedded(np.asarray(lengths, dtype=np.int32), off)
    st_in = embedded(state, off) if state is not None else None
    st_out = st_in if in_place else Embedded((5, D), np.float64, off)
    if st_in is not None and not in_place:
        ins["state_in"] = st_in
    nbytes = L.mlpg_hip_column_stats_workspace(B, Tmax, D)
    ws = Workspace(nbytes)
    c0 = _counts()
    rc = L.mlpg_hip_column_stats(dev.index, _hip._stream(dev), int(X.dtype == np.float64), p(ins["x"]), ld, p(ins.get("lengths")), B, Tmax, D,
                                 p(st_in), p(st_out), p(ws), nbytes)
    torch.cuda.synchronize()
    d = [b - a for a, b in zip(c0, _counts())]
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    assert d[39] == 1 and sum(d) == 1, d
    bad = failed(ins, dict(state_out=st_out), dict(workspace=ws))
    assert not bad, bad
    return st_out.host()


def run_affine(X, lengths, a, c, mode, out_dtype, off=0, ld_x=None, ld_y=None, in_place=False):
    """One call of mlpg_hip_column_affine on guarded buffers; the columns of x past D hold 3, those of y are prefilled with the
    guard byte.  Returns the whole (B, Tmax, ld_y) output."""
    from nnmnkwii_amd import _hip
    L = _lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, Tmax, D = X.shape
    ld_x = D if ld_x is None else ld_x
    ld_y = ld_x if in_place else (D if ld_y is None else ld_y)
    x = embedded(_wide(X, ld_x, 3.0), off)
    ins = dict(a=embedded(np.asarray(a, dtype=np.float64), off), c=embedded(np.asarray(c, dtype=np.float64), off))
    if lengths is not None:
        ins["lengths"] = embedded(np.asarray(lengths, dtype=np.int32), off)
    if in_place:
        y, out_dtype = x, X.dtype
    else:
        ins["x"] = x
        y = Embedded((B, Tmax, ld_y), out_dtype, off)
    c0 = _counts()
    rc = L.mlpg_hip_column_affine(dev.index, _hip._stream(dev), int(X.dtype == np.float64), int(np.dtype(out_dtype) == np.float64), mode, p(x), ld_x,
                                  p(y), ld_y, p(ins.get("lengths")), B, Tmax, D, p(ins["a"]), p(ins["c"]))
    torch.cuda.synchronize()
    d = [b - a for a, b in zip(c0, _counts())]
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    assert d[41] == 1 and sum(d) == 1, d
    bad = failed(ins, dict(y=y))
    assert not bad, bad
    return y.host()


@functools.lru_cache(maxsize=None)
def case(B, D, dtype_name):
    X, L = C.padded(B * 100 + D, C.LENGTHS[B], D, np.dtype(dtype_name))
    lengths = None if B == 1 else L                  # B == 1: lengths = NULL, every frame live
    X.setflags(write=False)
    return X, lengths, NM.kernel_state(X, lengths)


@functools.lru_cache(maxsize=None)
def truth_of(B, D, dtype_name):
    X, lengths, _ = case(B, D, dtype_name)
    return NM.exact(X, lengths)


def check_stats(state, X, lengths, truth):
    count, mean, var, mn, mx = NM.stats_of(state)
    live = np.concatenate([X[b, :n] for b, n in enumerate(NM.live_frames(lengths, X.shape[0], X.shape[1]))])
    assert count == truth["count"] == len(live)
    assert np.array_equal(mn, live.min(axis=0)) and np.array_equal(mx, live.max(axis=0))
    for k, const in C.CONSTANT.items():
        for d in range(k, X.shape[2], len(C.COLUMNS)):
            assert mean[d] == X.dtype.type(const) and var[d] == 0.0
    r = NM.ratios(mean, var, truth)
    print("against the truth: mean %.3f S_mean, var %.3f S_var (bound %.2f)" % (r[0], r[1], C.BOUND_RATIO))
    assert max(r) <= C.BOUND_RATIO
    return r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("B", [1, 2, 3, 5, 17])
@pytest.mark.parametrize("D", C.DIMS)
def test_statistics_kernel_against_the_model(D, B, dtype):
    X, lengths, model = case(B, D, np.dtype(dtype).name)
    state = run_stats(X, lengths, off=(B + D) % 2, ld=D + B % 3)
    assert same_bits(state[0], model[0]) and same_bits(state[3:], model[3:])         # count, min, max
    assert same_bits(state[1:3], model[1:3]), np.abs(state[1:3] - model[1:3]).max()   # mean and M2: the divisions are IEEE too
    if (B, D) in ((1, 1), (2, 5), (3, 63), (5, 64), (17, 65), (3, 187), (17, 5)):
        check_stats(state, X, lengths, truth_of(B, D, np.dtype(dtype).name))


def test_same_bits_on_every_call_and_behind_other_launches():
    X, lengths, model = case(17, 187, "float32")
    first = run_stats(X, lengths, off=1, ld=190)
    again = run_stats(X, lengths, off=0, ld=187)
    other = case(5, 63, "float64")
    run_stats(other[0], other[1])
    run_stats(X[::-1].copy(), lengths[::-1].copy())                                   # the same frames in another order: other bits are fine
    third = run_stats(X, lengths, off=1, ld=200)
    assert same_bits(first, again) and same_bits(first, third) and same_bits(first, model)


def test_streamed_calls_through_the_state():
    X, lengths, _ = case(17, 65, "float64")
    truth = truth_of(17, 65, "float64")
    whole = run_stats(X, lengths)
    st = None
    for lo, hi in ((0, 3), (3, 4), (4, 12), (12, 17)):
        st = run_stats(X[lo:hi], lengths[lo:hi], state=st, in_place=st is not None and lo != 3, off=lo % 2)
    check_stats(st, X, lengths, truth)
    assert same_bits(st[0], whole[0]) and same_bits(st[3:], whole[3:])
    model = None
    for lo, hi in ((0, 3), (3, 4), (4, 12), (12, 17)):
        model = NM.kernel_state(X[lo:hi], lengths[lo:hi], model)
    assert same_bits(st, model)


def test_no_live_frame_hands_the_state_through():
    X, lengths, model = case(3, 5, "float64")
    zeros = np.zeros(3, dtype=np.int32)
    assert same_bits(run_stats(X, zeros), NM.empty_state(5))
    assert same_bits(run_stats(X, zeros, state=model), model)
    assert same_bits(run_stats(X, -lengths, state=model, in_place=True, off=1), model)     # negative lengths count as 0
    assert same_bits(run_stats(X[:0], zeros[:0], state=model), model)                      # B == 0 still writes state_out
    beyond = run_stats(X, lengths + 1000)                                                  # lengths above Tmax count as Tmax
    assert beyond[0, 0] == X.shape[0] * X.shape[1] and np.isnan(beyond[1]).all()           # (the pad frames hold NaN)


def test_nan_and_inf_columns():
    X, L = C.padded(3, [40, C.BLOCK + 3], 5)
    X[0, 17, 1] = np.nan
    X[1, C.BLOCK + 2, 2] = np.inf
    X[1, 0, 3] = -np.inf                      # the workgroup's K
    state = run_stats(X, L)
    assert same_bits(state, NM.kernel_state(X, L))
    count, mean, var, mn, mx = NM.stats_of(state)
    assert count == 43 + C.BLOCK and np.isnan(mean[1:4]).all() and np.isnan(var[1:4]).all() and np.isfinite(mean[[0, 4]]).all()
    assert np.isnan(mn[1]) and np.isnan(mx[1]) and mx[2] == np.inf and mn[3] == -np.inf and np.isfinite([mn[2], mx[3]]).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dt_in,dt_out", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
def test_apply_kernel_against_the_model(mode, dt_in, dt_out):
    for D, lengths in ((65, [0, 70, 33, 1]), (187, [130, 64]), (1, [5]), (64, [63, 65, 2])):
        X, L = C.padded(D + mode, lengths, D, dt_in)
        rng = np.random.RandomState(D)
        a, c = rng.rand(D) + 0.5, rng.randn(D)
        ref = NM.affine(X, a, c, mode, L, dt_out)
        y = run_affine(X, L, a, c, mode, dt_out, off=D % 2, ld_x=D + 2, ld_y=D + 3)
        assert y.dtype == dt_out and same_bits(y[:, :, :D], ref)
        assert (y[:, :, D:].view(np.uint8) == 0xA5).all()                         # columns past D are not touched
        assert all((y[b, n:, :D] == 0).all() for b, n in enumerate(lengths))      # pad rows: exact zeros
        if dt_in == dt_out:                                                        # in place on a column slice of a wider array
            z = run_affine(X, L, a, c, mode, dt_out, off=1 - D % 2, ld_x=D + 2, in_place=True)
            assert same_bits(z[:, :, :D], ref) and (z[:, :, D:] == 3).all()
    X, _ = C.padded(9, [70, 33], 5, dt_in, pad_value=2.5)
    y = run_affine(X, None, np.full(5, 2.0), np.ones(5), mode, dt_out)            # lengths = NULL: every frame is live
    assert same_bits(y, NM.affine(X, np.full(5, 2.0), np.ones(5), mode, None, dt_out))


# ---- the Python functions end to end ------------------------------------------------------------------------------------------
def utterances(name):
    X, L = G[name + "/X"], G[name + "/lengths"]
    return [X[b, :L[b]] for b in range(len(L))]


def close_to_reference(name, mean, var, keys=("mean", "var")):
    """|ours - reference| <= 8 (WORST_RATIO + the reference's ratio) scales on the columns that are not constant."""
    truth = NM.exact(G[name + "/X"], G[name + "/lengths"])
    ref = G[name + "/ref_ratio"]
    for got, key, s, rr in ((mean, keys[0], truth["s_mean"], ref[0]), (var, keys[1], truth["s_var"], ref[1])):
        live = s > 0
        assert (np.abs(got - G[name + "/" + key])[live] <= (8 * (C.WORST_RATIO + rr) * s)[live]).all(), key
    return truth


def float32_close_to_reference(name, mean, var):
    """A float32 corpus: the reference answers in float32.  Both sides round a float64 value that lies within a few of the
    float64 error scales of the truth -- far less than half a float32 ulp -- so they are at most one float32 ulp apart.  Constant
    columns: the reference's variance is not exact there (1.9e-35 for the 0.1 column of the probe); ours is 0."""
    assert mean.dtype == var.dtype == np.float32
    D = len(mean)
    const = np.array([d for k in C.CONSTANT for d in range(k, D, len(C.COLUMNS))], dtype=np.int64)
    other = np.setdiff1d(np.arange(D), const)
    assert (np.abs(mean - G[name + "/mean"]) <= np.spacing(np.abs(G[name + "/mean"]))).all()
    assert (np.abs(var - G[name + "/var"])[other] <= np.spacing(np.abs(G[name + "/var"]))[other]).all()
    assert (var[const] == 0).all()


@pytest.mark.parametrize("name", ["probe64", "blocks64"])
def test_meanvar_meanstd_minmax_against_the_reference(name):
    from nnmnkwii_amd import preprocessing as P
    utts = utterances(name)
    X, L = G[name + "/X"], G[name + "/lengths"]
    results = [P.meanvar(utts, return_last_sample_count=True), P.meanvar(X, L, return_last_sample_count=True),
               P.meanvar(iter(utts), return_last_sample_count=True)]
    for mean, var, count in results:
        assert mean.dtype == var.dtype == np.float64 and count == int(G[name + "/count"]) and isinstance(count, int)
        truth = close_to_reference(name, mean, var)
        assert max(NM.ratios(mean, var, truth)) <= C.BOUND_RATIO
    assert all(same_bits(r[0], results[0][0]) and same_bits(r[1], results[0][1]) for r in results)   # one batch each: the same partition
    mn, mx = P.minmax(utts)
    assert np.array_equal(mn, G[name + "/min"]) and np.array_equal(mx, G[name + "/max"])
    assert all(np.array_equal(u, v) for u, v in zip(P.minmax(X, L), (mn, mx)))
    mean, std = P.meanstd(utts)
    const = [d for k in C.CONSTANT for d in range(k, X.shape[2], len(C.COLUMNS))]
    assert (std[const] == 1.0).all() and same_bits(mean, results[0][0])
    other = np.setdiff1d(np.arange(X.shape[2]), const)
    assert np.array_equal(std[other], np.sqrt(results[0][1])[other])
    # continued from the reference's (mean_, var_, last_sample_count)
    prior = (G[name + "/prior_mean"], G[name + "/prior_var"], int(G[name + "/prior_count"]))
    m3, v3, c3 = P.meanvar(X[2:], L[2:], *prior, return_last_sample_count=True)
    assert c3 == int(G[name + "/streamed_count"])
    truth = close_to_reference(name, m3, v3, keys=("streamed_mean", "streamed_var"))
    # the named tuple of the single pass, streamed through its state
    s1 = P.column_stats(utts[:3])
    s2 = P.column_stats(utts[3:], state=s1.state)
    assert s2.count == int(G[name + "/count"]) and np.array_equal(s2.min, mn) and np.array_equal(s2.max, mx)
    assert max(NM.ratios(s2.mean, s2.var, truth)) <= C.BOUND_RATIO
    with pytest.raises(ValueError, match="no live frame"):
        P.meanvar(X, np.zeros_like(L))


def test_float32_corpus_and_batches_of_bounded_size(monkeypatch):
    from nnmnkwii_amd import preprocessing as P
    for name in ("probe32", "arctic"):
        utts = utterances(name)
        mean, var = P.meanvar(utts)                                       # the reference's rule: the dtype of dataset[0]
        float32_close_to_reference(name, mean, var)
    mn, mx = P.minmax(utts)
    assert mn.dtype == np.float32 and np.array_equal(mn, G[name + "/min"]) and np.array_equal(mx, G[name + "/max"])
    # a bound that holds one utterance per batch: streamed through the state on the device
    monkeypatch.setattr(P.generic, "STATS_BATCH_ELEMS", 113 * 187)
    c0 = _counts()
    s = P.column_stats(utts)
    assert _counts()[39] - c0[39] == 3
    truth = NM.exact(G[name + "/X"], G[name + "/lengths"])
    assert s.count == truth["count"] and max(NM.ratios(s.mean, s.var, truth)) <= C.BOUND_RATIO


@pytest.mark.parametrize("name", ["probe64", "probe32", "arctic"])
def test_scalers_against_the_reference(name):
    from nnmnkwii_amd import preprocessing as P
    x = utterances(name)[1]
    mean, std, mn, mx = (G[name + "/" + k] for k in ("mean", "std", "min", "max"))
    min_, scale_ = G[name + "/min_"], G[name + "/scale_"]
    fr = tuple(float(v) for v in G["feature_range"])
    got = {"scale": P.scale(x, mean, std), "inv_scale": P.inv_scale(x, mean, std),
           "minmax_scale": P.minmax_scale(x, mn, mx, feature_range=fr), "minmax_scale_params": P.minmax_scale(x, scale_=scale_, min_=min_),
           "inv_minmax_scale": P.inv_minmax_scale(x, mn, mx, feature_range=fr),
           "inv_minmax_scale_params": P.inv_minmax_scale(x, scale_=scale_, min_=min_)}
    m2, s2 = P.minmax_scale_params(mn, mx, feature_range=fr)
    assert np.array_equal(m2, min_) and np.array_equal(s2, scale_) and m2.dtype == min_.dtype
    x64 = x.astype(np.float64)
    for key, y in got.items():
        ref = G[name + "/" + key]
        assert y.dtype == ref.dtype and y.shape == ref.shape, key
        if x.dtype == np.float64:
            assert np.array_equal(y, ref), key
        elif key in ("scale", "inv_minmax_scale", "inv_minmax_scale_params"):
            assert (np.abs(y.astype(np.float64) - ref) <= 2 * 2.0 ** -23 * np.abs(ref)).all(), key
        else:
            a = (std if key == "inv_scale" else scale_).astype(np.float64)
            assert (np.abs(y.astype(np.float64) - ref) <= 2.0 ** -23 * (np.abs(a * x64) + np.abs(ref))).all(), key
    # float32 data with float64 statistics promotes, as in numpy
    assert P.scale(x, mean.astype(np.float64), std.astype(np.float64)).dtype == np.float64
    assert np.array_equal(P.scale(x, mean.astype(np.float64), std.astype(np.float64)), (x - mean.astype(np.float64)) / std.astype(np.float64))


def test_tensors_in_place_on_a_column_slice_and_one_launch_per_padded_batch():
    from nnmnkwii_amd import preprocessing as P, util
    dev = torch.device("cuda", torch.cuda.current_device())
    X, L = G["arctic/X"], G["arctic/lengths"]
    utts = utterances("arctic")
    wide = torch.full((3, X.shape[1], 200), 7.0, dtype=torch.float32, device=dev)
    wide[:, :, 5:192] = torch.from_numpy(X).to(dev)
    view = wide[:, :, 5:192]
    mean, std = P.meanstd(view, L)                                   # a CUDA tensor, used where it lies
    assert mean.is_cuda and std.is_cuda and mean.dtype == torch.float32
    m_ref, s_ref = P.meanstd(utts)
    assert np.array_equal(mean.cpu().numpy(), m_ref)
    assert (np.abs(std.cpu().numpy() - s_ref) <= np.spacing(s_ref)).all()      # the square roots: one float32 ulp
    c0 = _counts()
    out = P.scale(view, mean, std, lengths=L, out=view)              # in place
    d = [b - a for a, b in zip(c0, _counts())]
    assert out is view and d[41] == 1 and sum(d) == 1
    host = wide.cpu().numpy()
    assert (host[:, :, :5] == 7).all() and (host[:, :, 192:] == 7).all()
    for b, u in enumerate(utts):
        ref = (u.astype(np.float64) - m_ref) / s_ref
        assert (np.abs(host[b, :len(u), 5:192] - ref) <= 2 * 2.0 ** -23 * np.abs(ref)).all() and (host[b, len(u):, 5:192] == 0).all()
    # the round trip of the training pipeline: x -> scale -> inv_scale, float32
    back = P.inv_scale(view, mean, std, lengths=L).cpu().numpy()
    for b, u in enumerate(utts):
        x64 = u.astype(np.float64)
        assert (np.abs(back[b, :len(u)] - x64) <= 2.0 ** -22 * (np.abs(x64 - m_ref) + np.abs(x64))).all()
    const = [d_ for k in C.CONSTANT for d_ in range(k, 187, len(C.COLUMNS))]
    assert all((back[b, :len(u)][:, const] == u[:, const]).all() for b, u in enumerate(utts))      # constant columns come back exactly
    # util.apply_each2d_padded: one launch for the batch instead of one call per utterance
    c0 = _counts()
    Y = util.apply_each2d_padded(P.scale, X, L, m_ref, s_ref)
    d = [b - a for a, b in zip(c0, _counts())]
    assert d[41] == 1 and sum(d) == 1 and Y.dtype == np.float64 and Y.shape == X.shape
    assert all(np.array_equal(Y[b, :n], P.scale(X[b, :n], m_ref, s_ref).astype(np.float64)) and (Y[b, n:] == 0).all() for b, n in enumerate(L))
    for f, args in ((P.inv_scale, (m_ref, s_ref)), (P.minmax_scale, (G["arctic/min"], G["arctic/max"])),
                    (P.inv_minmax_scale, (G["arctic/min"], G["arctic/max"]))):
        c0 = _counts()
        Y = util.apply_each2d_padded(f, X, L, *args)
        assert _counts()[41] - c0[41] == 1 and np.array_equal(Y[1, :L[1]], f(X[1, :L[1]], *args).astype(np.float64))


def test_statistics_feed_multi_stream_mlpg_on_the_device():
    """The synthesis path: the network's output goes through inv_scale, the corpus variance is the global variance of
    multi_stream_mlpg -- device tensors throughout, no host-memory route (kinds 10, 11) is taken."""
    from nnmnkwii_amd import paramgen, preprocessing as P
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.RandomState(0)
    B, T, sizes, dyn = 3, 80, [9, 3, 1, 3], [True, True, False, True]
    D = sum(sizes)
    L = np.array([80, 33, 64], dtype=np.int32)
    Y = rng.randn(B, T, D) * (0.5 + rng.rand(D)) + rng.randn(D)
    Yd = torch.from_numpy(Y).to(dev)
    Ld = torch.from_numpy(L).to(dev)
    mean, var = P.meanvar(Yd, Ld)
    std = var.sqrt()
    assert mean.is_cuda and var.is_cuda and var.dtype == torch.float64
    Z = P.scale(Yd, mean, std, lengths=Ld)                            # what the network would be trained on
    c0 = _counts()
    gen = paramgen.multi_stream_mlpg(P.inv_scale(Z, mean, std, lengths=Ld), var, WINDOWS, sizes, dyn, lengths=Ld)
    d = [b - a for a, b in zip(c0, _counts())]
    assert gen.is_cuda and d[41] == 1 and d[10] == 0 and d[11] == 0
    mean_h, var_h = P.meanvar(Y, L)
    ref = paramgen.multi_stream_mlpg(Y * (np.arange(T)[None, :, None] < L[:, None, None]), var_h, WINDOWS, sizes, dyn, lengths=L)
    assert np.array_equal(var.cpu().numpy(), var_h)
    assert np.abs(gen.cpu().numpy() - ref).max() <= 1e-9 * np.abs(ref).max()


def test_capturable_into_a_graph_once_the_workspace_exists():
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda", torch.cuda.current_device())
    X, lengths, model = case(5, 65, "float64")
    x = torch.from_numpy(np.nan_to_num(X, nan=0.0)).to(dev)
    Ld = torch.from_numpy(lengths).to(dev)
    ws = torch.empty(_hip.column_stats_workspace(*x.shape) // 8, dtype=torch.float64, device=dev)
    state = torch.empty((5, 65), dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _hip.column_stats(x, Ld, None, state, ws)
        s.synchronize()
        eager = state.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _hip.column_stats(x, Ld, None, state, ws)
            _hip.column_affine(x, state[4], state[1], 0, Ld, y)
        state.zero_()
        g.replay()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(state, eager) and same_bits(state.cpu().numpy(), model)
    st = state.cpu().numpy()
    assert same_bits(y.cpu().numpy(), NM.affine(np.nan_to_num(X, nan=0.0), st[4], st[1], 0, lengths))
