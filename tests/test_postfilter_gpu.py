"""GPU tests (-m gpu) of the Merlin post-filter (csrc/postfilter.hip, nnmnkwii_amd.postfilters) against the literal float64 form
of tools/postfilter_model.py (for float32: evaluated on the float32-rounded input).  Bounds: the project's own for its float64
kernels with transcendental steps (tests/test_modspec_batch_gpu.py): 1e-11 of the reference's maximum in float64, 2e-6 in float32.
The model's frames are independent, so one reference per (D, order, fftlen, dtype) over a pool of 2 tile + 3 frames serves every
frame count and batch shape cut from that pool."""
import os
import sys

import numpy as np
import pytest
import torch

from embed import Embedded, embedded, failed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import postfilter_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
BOUND = {F64: 1e-11, F32: 2e-6}
TORCH_DT = {F32: torch.float32, F64: torch.float64}
DIMS = (1, 2, 3, 4, 5, 25, 60, 63, 64)
SIZES = ((15, 32), (31, 64), (511, 1024))
ALPHAS = (0.58, 0.35, 0.77, -0.42, 0.0)


def _tile():
    from nnmnkwii_amd import _hip
    return _hip.POSTFILTER_FRAME_TILE


def mgc_like(rng, T, D):
    x = rng.randn(T, D) / (1.0 + np.arange(D))
    x[:, 0] += rng.uniform(-8.0, 2.0, T)
    return x


def _err(got, ref):
    return float(np.abs(np.asarray(got, dtype=F64) - ref).max() / np.abs(ref).max())


def _count(kind=None):
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return L.mlpg_hip_launch_count(kind) if kind is not None else [L.mlpg_hip_launch_count(k) for k in range(30)]


@pytest.mark.parametrize("D", DIMS)
def test_parity_grid(D):
    from nnmnkwii_amd import postfilters as PF
    tile = _tile()
    pool_n = 2 * tile + 3
    rng = np.random.RandomState(100 + D)
    dev = torch.device("cuda")
    worst = {F32: 0.0, F64: 0.0}
    for si, (order, fftlen) in enumerate(SIZES):
        if order < D - 1:
            continue
        alpha = ALPHAS[(D + si) % len(ALPHAS)]
        pool = mgc_like(rng, pool_n, D)
        for dt in (F64, F32):
            xin = pool.astype(dt)
            ref = PM.post_filter_literal(xin.astype(F64), alpha, order, fftlen)
            for T in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
                x = torch.from_numpy(xin[:T][None].copy()).to(dev)
                got = PF.merlin_post_filter_batch(x, alpha, order, fftlen).cpu().numpy()
                assert got.dtype == dt and got.shape == (1, T, D)
                e = _err(got[0], ref[:T])
                worst[dt] = max(worst[dt], e)
                assert e <= BOUND[dt], (D, order, fftlen, alpha, dt.__name__, T, e)
            # three utterances cut from the pool (the workgroup's tile does not divide Tmax), with and without lengths
            B, Tmax = 3, (pool_n - 2) // 3
            xb = torch.from_numpy(xin[:B * Tmax].reshape(B, Tmax, D).copy()).to(dev)
            refb = ref[:B * Tmax].reshape(B, Tmax, D)
            got = PF.merlin_post_filter_batch(xb, alpha, order, fftlen).cpu().numpy()
            e = _err(got, refb)
            assert e <= BOUND[dt], (D, order, fftlen, dt.__name__, "batch", e)
            lengths = [Tmax, 7, 0]
            got = PF.merlin_post_filter_batch(xb, alpha, order, fftlen, lengths=lengths).cpu().numpy()
            masked = refb.copy()
            masked[1, 7:] = 0.0
            masked[2] = 0.0
            e = _err(got, masked)
            worst[dt] = max(worst[dt], e)
            assert e <= BOUND[dt], (D, order, fftlen, dt.__name__, "lengths", e)
            assert not got[1, 7:].any() and not got[2].any() and not np.signbit(got[2]).any()
    print("post-filter parity D=%d: float64 %.2e  float32 %.2e" % (D, worst[F64], worst[F32]))


@pytest.mark.parametrize("dt", (F64, F32))
def test_padding_strides_sentinels_in_place_and_repeatability(dt):
    """NaN in the padding frames and in the columns beyond D of a strided input reaches no output; padded rows are exactly 0;
    columns of out beyond D keep a sentinel; in place equals out of place bit for bit; two calls give the same bits."""
    from nnmnkwii_amd import _hip
    tile = _tile()
    rng = np.random.RandomState(7)
    dev = torch.device("cuda")
    B, Tmax, D, ld, col = 3, tile + 9, 25, 40, 6
    alpha, order, fftlen = 0.42, 31, 64
    lens = np.array([Tmax + 5, 11, -3], dtype=np.int32)          # clamped to [0, Tmax]
    eff = np.clip(lens, 0, Tmax)
    clean = np.stack([mgc_like(rng, Tmax, D) for _ in range(B)]).astype(dt)
    wide = np.full((B, Tmax, ld), np.nan, dtype=dt)
    for b in range(B):
        wide[b, :eff[b], col:col + D] = clean[b, :eff[b]]
    ref = PM.post_filter_batch(clean.astype(F64), alpha, order, fftlen, lengths=lens)
    X = torch.from_numpy(wide).to(dev)
    w = torch.from_numpy(PM.default_weight(D)).to(dev)
    G = _hip.postfilter_table(dev, D, alpha, order, fftlen)
    lengths = torch.from_numpy(lens).to(dev)
    sentinel = -777.25
    out = torch.full((B, Tmax, ld + 3), sentinel, dtype=TORCH_DT[dt], device=dev)
    _hip.merlin_post_filter(X[..., col:col + D], alpha, w, G, fftlen, lengths=lengths, out=out[..., 2:2 + D])
    o = out.cpu().numpy()
    assert np.isfinite(o).all()
    assert (o[..., :2] == sentinel).all() and (o[..., 2 + D:] == sentinel).all()
    got = o[..., 2:2 + D]
    assert _err(got, ref) <= BOUND[dt]
    for b in range(B):
        assert not got[b, eff[b]:].any()
    # a second call: the same bits
    out2 = torch.full_like(out, sentinel)
    _hip.merlin_post_filter(X[..., col:col + D], alpha, w, G, fftlen, lengths=lengths, out=out2[..., 2:2 + D])
    assert torch.equal(out, out2)
    # in place on the strided view: the same bits, the NaN around it untouched
    Xi = X.clone()
    view = Xi[..., col:col + D]
    r = _hip.merlin_post_filter(view, alpha, w, G, fftlen, lengths=lengths, out=view)
    assert r.data_ptr() == view.data_ptr()
    xi = Xi.cpu().numpy()
    assert xi[..., col:col + D].tobytes() == np.ascontiguousarray(got).tobytes()
    assert np.isnan(xi[..., :col]).all() and np.isnan(xi[..., col + D:]).all()


def test_column_slice_of_a_wider_tensor_equals_the_contiguous_copy():
    from nnmnkwii_amd import postfilters as PF
    rng = np.random.RandomState(8)
    dev = torch.device("cuda")
    B, Tmax = 2, 70
    Y = torch.from_numpy(rng.randn(B, Tmax, 80)).to(dev)
    Y[..., 10:70] = torch.from_numpy(np.stack([mgc_like(rng, Tmax, 60) for _ in range(B)])).to(dev)
    keep = Y.clone()
    a = PF.merlin_post_filter_batch(Y[..., 10:70], 0.58)
    b = PF.merlin_post_filter_batch(Y[..., 10:70].contiguous(), 0.58)
    assert a.is_contiguous() and torch.equal(a, b) and torch.equal(Y, keep)
    # out = mgc on the slice: the mgc columns are filtered where they lie, the others stay
    r = PF.merlin_post_filter_batch(Y[..., 10:70], 0.58, out=Y[..., 10:70])
    assert torch.equal(r, a) and torch.equal(Y[..., :10], keep[..., :10]) and torch.equal(Y[..., 70:], keep[..., 70:])


@pytest.mark.parametrize("dt", (F64, F32))
def test_buffers_at_element_offsets_between_guard_bands(dt):
    """The C entry itself on buffers of tests/embed.py: every pointer aligned, then every input one element in.  Guards intact,
    inputs unchanged, the two results equal bit for bit and within the bound."""
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    tile = _tile()
    rng = np.random.RandomState(9)
    B, Tmax, D = 2, tile // 2 + 5, 5
    alpha, order, fftlen = 0.35, 15, 32
    x = np.stack([mgc_like(rng, Tmax, D) for _ in range(B)]).astype(dt)
    lens = np.array([Tmax, 9], dtype=np.int32)
    w = PM.default_weight(D)
    G = _hip.postfilter_table_host(D, alpha, order, fftlen)
    ref = PM.post_filter_batch(x.astype(F64), alpha, order, fftlen, lengths=lens)
    res = []
    for off in (0, 1):
        ins = dict(mgc=embedded(x, off), lengths=embedded(lens, off), weight=embedded(w, off), G=embedded(G, off))
        out = Embedded((B, Tmax, D), dt, off, 0xA5)
        rc = L.mlpg_hip_merlin_post_filter(dev.index, _hip._stream(dev), 0 if dt is F32 else 1, ins["mgc"].ptr(), D, ins["lengths"].ptr(),
                                           B, Tmax, D, alpha, ins["weight"].ptr(), ins["G"].ptr(), fftlen, out.ptr(), D)
        torch.cuda.synchronize()
        assert rc == 0, (off, rc, L.mlpg_hip_last_error())
        bad = failed(ins, dict(out=out))
        assert not bad, (off, bad)
        res.append(out.host())
    assert res[0].tobytes() == res[1].tobytes()
    assert _err(res[0], ref) <= BOUND[dt]


def test_counter_29_moves_once_per_launching_call_and_no_other_kind_moves():
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda")
    rng = np.random.RandomState(10)
    x = torch.from_numpy(mgc_like(rng, 10, 5)[None]).to(dev)
    w = torch.from_numpy(PM.default_weight(5)).to(dev)
    G = _hip.postfilter_table(dev, 5, 0.35, 15, 32)
    c0 = _count()
    for _ in range(3):
        _hip.merlin_post_filter(x, 0.35, w, G, 32)
    _hip.merlin_post_filter(x[:, :0], 0.35, w, G, 32)             # Tmax == 0: nothing is launched
    _hip.merlin_post_filter(x[:0], 0.35, w, G, 32)                # B == 0
    torch.cuda.synchronize()
    c1 = _count()
    assert c1[29] == c0[29] + 3
    assert [b - a for k, (a, b) in enumerate(zip(c0, c1)) if k != 29] == [0] * 29
    assert _count(28) == -1 and _count(30) == -1


def test_numpy_cpu_tensor_and_compat_paths():
    from nnmnkwii_amd import compat, postfilters as PF
    rng = np.random.RandomState(11)
    T, D, alpha = 37, 25, 0.42
    x = mgc_like(rng, T, D)
    ref = PM.post_filter_literal(x, alpha, 63, 128)
    y = PF.merlin_post_filter(x, alpha, 63, 128)
    assert isinstance(y, np.ndarray) and y.dtype == F64 and y.shape == (T, D) and _err(y, ref) <= BOUND[F64]
    x32 = x.astype(F32)
    y32 = PF.merlin_post_filter(x32, alpha, 63, 128)
    assert y32.dtype == F32 and _err(y32, PM.post_filter_literal(x32.astype(F64), alpha, 63, 128)) <= BOUND[F32]
    # explicit weight and coef, as the reference takes them
    wgt = 1.0 + rng.rand(D)
    assert _err(PF.merlin_post_filter(x, alpha, 63, 128, weight=wgt), PM.post_filter_literal(x, alpha, 63, 128, weight=wgt)) <= BOUND[F64]
    assert _err(PF.merlin_post_filter(x, alpha, 63, 128, coef=1.2), PM.post_filter_literal(x, alpha, 63, 128, coef=1.2)) <= BOUND[F64]
    # a CPU tensor comes back as a CPU tensor, and is not written
    xt = torch.from_numpy(x.copy())
    yt = PF.merlin_post_filter(xt, alpha, 63, 128)
    assert torch.is_tensor(yt) and yt.device.type == "cpu" and np.array_equal(yt.numpy(), y) and np.array_equal(xt.numpy(), x)
    # a CUDA tensor is filtered in place and returned
    xc = torch.from_numpy(x.copy()).cuda()
    yc = PF.merlin_post_filter(xc, alpha, 63, 128)
    assert yc is xc and np.array_equal(xc.cpu().numpy(), y)
    compat.install()
    try:
        import importlib
        mod = importlib.import_module("nnmnkwii.postfilters")
        assert mod.merlin_post_filter is PF.merlin_post_filter
        from nnmnkwii.postfilters import merlin_post_filter
        assert np.array_equal(merlin_post_filter(x, alpha, 63, 128), y)
    finally:
        compat.uninstall()


def test_apply_each2d_padded_makes_one_launch_and_equals_the_loop():
    from nnmnkwii_amd import postfilters as PF, util
    rng = np.random.RandomState(12)
    B, Tmax, D, alpha = 4, 50, 25, 0.42
    lengths = np.array([50, 31, 1, 17])
    X = np.zeros((B, Tmax, D))
    for b in range(B):
        X[b, :lengths[b]] = mgc_like(rng, lengths[b], D)
    c0 = _count(29)
    Y = util.apply_each2d_padded(PF.merlin_post_filter, X, lengths, alpha, 63, 128)
    assert _count(29) == c0 + 1
    assert Y.dtype == F64 and Y.shape == X.shape
    loop = np.zeros_like(X)
    for b in range(B):
        loop[b, :lengths[b]] = PF.merlin_post_filter(X[b, :lengths[b]], alpha, 63, 128)
    assert np.array_equal(Y, loop)
    c0 = _count(29)
    Yt = util.apply_each2d_trim(PF.merlin_post_filter, X, alpha, 63, 128)
    assert _count(29) == c0 + 1 and np.array_equal(Yt, Y)


def test_larger_case_at_the_defaults():
    """8 x 300 x 60 at the defaults: every 37th frame against the model, and the two properties that need no reference."""
    from nnmnkwii_amd import _hip, postfilters as PF
    rng = np.random.RandomState(13)
    B, Tmax, D, alpha = 8, 300, 60, 0.58
    x = np.stack([mgc_like(rng, Tmax, D) for _ in range(B)])
    xd = torch.from_numpy(x).cuda()
    y = PF.merlin_post_filter_batch(xd, alpha).cpu().numpy()
    flat_x, flat_y = x.reshape(-1, D), y.reshape(-1, D)
    pick = np.arange(0, B * Tmax, 37)
    ref = PM.post_filter_literal(flat_x[pick], alpha)
    e = _err(flat_y[pick], ref)
    print("larger case: %d frames checked, err %.2e" % (len(pick), e))
    assert e <= BOUND[F64]
    # weight = 1 is the identity
    same = PF.merlin_post_filter_batch(xd, alpha, weight=np.ones(D)).cpu().numpy()
    assert _err(same, x) <= BOUND[F64]
    # the frame energy is preserved.  With |out - exact| <= BOUND max|out| per coefficient, L = G c moves by at most
    # max_k sum_d |G[k][d]| times that, and log r0 by at most twice as much.
    G = _hip.postfilter_table_host(D, alpha, 511, 1024)
    r_in, r_out = PM.r0_from_table(flat_x, G, 1024), PM.r0_from_table(flat_y, G, 1024)
    slack = 2.0 * np.abs(G).sum(axis=1).max() * BOUND[F64] * np.abs(y).max()
    drift = np.abs(np.log(r_out / r_in)).max()
    print("larger case: energy drift %.2e (bound %.2e)" % (drift, slack))
    assert drift <= slack
