"""GPU tests (-m gpu): one small guarded cell per device-pointer entry point that tests/test_embed_mlpg_gpu.py and
tests/test_mixture_rows_gpu.py do not reach -- delta features, the trailing-zero trim, the gather along a warping path, the GMM
conversion, fastdtw, the four float64 modulation-spectrum calls on all three routes, and the padded-minibatch spectrum, its
gradient and the fused loss step.

Every cell runs the C entry twice on buffers of tests/embed.py: with every pointer aligned, and with every input one element in.
The outputs sit between guard bands in both calls, the loss workspace is exactly mlpg_hip_modspec_loss_workspace_bytes between
guards.  All guards must be intact, the inputs unchanged, the two results equal bit for bit, and the aligned one within the bound
the entry's own test uses of the reference that test uses.

Left out on purpose: the mlpg_hip_dtw_level_* entries (one lane per pair, on buffers the wrapper sizes itself), the multi-stream
entries (their tests guard columns and shift in_col) and the host-pointer entries (tests/test_literal_calls_gpu.py guards those)."""
import numpy as np
import pytest
import torch

import modspec_batch64 as R
from cases import WINDOW_SETS
from embed import Embedded, Workspace, embedded, failed, ptr
from oracle import dtw as OD
from oracle import mlpg as O
from oracle import modspec as OM
from oracle.mlpg import pack_windows
from test_dtw_costs_cpu import L1 as NP_L1, L2 as NP_L2, SQL2 as NP_SQL2, NP_DISTS, NP_SCALES

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DT_ID = {F32: 0, F64: 1}
EINVAL = -1


def _call():
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda", torch.cuda.current_device())
    return _hip.lib(), dev.index, _hip._stream(dev)


def _twice(call, arrays, out_shapes, work=None, same=None, what=()):
    """Run call(ins, outs, works) with the inputs aligned and one element in; returns the aligned call's outputs (host arrays).
    arrays: name -> ndarray or None; out_shapes: name -> (shape, dtype); work: name -> (bytes, alignment).  `same(a, b)` replaces
    the bitwise comparison of the two results where parts of an output are unspecified."""
    res = []
    for label, off in (("aligned", 0), ("inputs+1", 1)):
        ins = {n: embedded(a, off) for n, a in arrays.items()}
        outs = {n: Embedded(shape, dt, 0, 0xA5) for n, (shape, dt) in out_shapes.items()}
        works = {n: Workspace(nbytes, align) for n, (nbytes, align) in (work or {}).items()}
        rc = call(ins, outs, works)
        torch.cuda.synchronize()
        assert rc == 0, what + (label, rc)
        bad = failed(ins, outs, works)
        assert not bad, what + (label, bad)
        res.append({n: b.host() for n, b in outs.items()})
    a, b = res
    if same is not None:
        same(a, b)
    else:
        for n in a:
            assert a[n].tobytes() == b[n].tobytes(), what + ("%s differs between the aligned and the shifted call" % n,)
    return a


def _close(a, ref, rel, what=""):
    ref = np.asarray(ref, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    err = np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= rel, (what, err)


# ------------------------------------------------------------------------------------------------- delta, trim, gather, convert

@pytest.mark.parametrize("dt", [F32, F64])
def test_delta_features(dt):
    """float64: the bound of tests/test_util_gpu.py.  float32: each output is at most 3 products of float32 inputs with window
    coefficients of size <= 2, summed and rounded once in float32 -- an error below 4 * 2^-24 * sum|c| max|x| < 1e-6 max|out|."""
    L, dev, stream = _call()
    B, T, D = 3, 17, 5
    windows = WINDOW_SETS["std3"]
    wl, wu, wc = pack_windows(windows)
    rng = np.random.RandomState(17)
    x = rng.randn(B, T, D).astype(dt)
    lens = np.array([17, 16, 0], dtype=np.int32)

    def call(ins, outs, works):
        return L.mlpg_hip_delta_features(dev, stream, DT_ID[dt], ins["x"].ptr(), ins["lengths"].ptr(), B, T, D, len(windows),
                                         wl.ctypes.data, wu.ctypes.data, wc.ctypes.data, outs["out"].ptr())
    got = _twice(call, dict(x=x, lengths=lens), dict(out=((B, T, D * 3), dt)), what=("delta_features", dt.__name__))["out"]
    for b, n in enumerate(lens):
        assert not got[b, n:].any()
        if n:
            ref = O.delta_features(x[b, :n].astype(np.float64), windows)
            if dt == F64:
                np.testing.assert_allclose(got[b, :n], ref, rtol=1e-12, atol=1e-14)
            else:
                _close(got[b, :n], ref, 1e-6, b)


@pytest.mark.parametrize("dt", [F32, F64])
def test_trim_lengths(dt):
    L, dev, stream = _call()
    N, T, D = 4, 20, 3
    rng = np.random.RandomState(20)
    X = (rng.rand(N, T, D) + 0.1).astype(dt)
    X[0, 13:] = 0
    X[1, :] = 0                                                  # nothing left
    X[2, 5:9] = 0                                                # zeros inside stay
    X[3, 19] = 1e-9                                              # below eps: trimmed
    X[3, 15:19] = 0

    def call(ins, outs, works):
        return L.mlpg_hip_trim_lengths(dev, stream, DT_ID[dt], ins["X"].ptr(), N, T, D, 1e-7, outs["lengths"].ptr())
    got = _twice(call, dict(X=X), dict(lengths=((N,), np.int32)), what=("trim_lengths", dt.__name__))["lengths"]
    want = [len(OD.trim_zeros_frames(X[n].astype(np.float64))) for n in range(N)]
    assert got.tolist() == want == [13, 0, 20, 15]


@pytest.mark.parametrize("dt", [F32, F64])
def test_gather_path(dt):
    L, dev, stream = _call()
    N, Tsrc, Tout, D, P = 3, 9, 14, 5, 18
    rng = np.random.RandomState(9)
    src = rng.randn(N, Tsrc, D).astype(dt)
    plen = np.array([14, 9, 1], dtype=np.int32)
    path = np.full((N, P), 7, dtype=np.int32)
    for n in range(N):
        path[n, :plen[n]] = np.sort(rng.randint(0, Tsrc, size=plen[n]))

    def call(ins, outs, works):
        return L.mlpg_hip_gather_path(dev, stream, DT_ID[dt], ins["src"].ptr(), ins["path"].ptr(), ins["path_len"].ptr(), N, Tsrc, P,
                                      D, Tout, outs["out"].ptr())
    got = _twice(call, dict(src=src, path=path, path_len=plen), dict(out=((N, Tout, D), dt)), what=("gather_path", dt.__name__))["out"]
    want = np.zeros((N, Tout, D), dtype=dt)
    for n in range(N):
        want[n, :plen[n]] = src[n, path[n, :plen[n]]]
    assert np.array_equal(got, want)                             # a copy: exact


@pytest.mark.parametrize("form", ["posterior", "mixture"])
def test_gmm_convert(form):
    """out[n] = sum_m post[n, m] (mu_y[m] + A[m] (x[n] - mu_x[m])) in float64: the project's 1e-10 float64 bound."""
    L, dev, stream = _call()
    N, D, Dy, M = 70, 3, 3, 4
    rng = np.random.RandomState(70)
    x, mu_x, mu_y, A = rng.randn(N, D), rng.randn(M, D), rng.randn(M, Dy), rng.randn(M, Dy, D)
    post = rng.dirichlet(np.ones(M), size=N) if form == "posterior" else None
    mix = None if form == "posterior" else rng.randint(M, size=N).astype(np.int32)

    def call(ins, outs, works):
        return L.mlpg_hip_gmm_convert(dev, stream, ins["x"].ptr(), ptr(ins["posterior"]), ptr(ins["mixture"]), ins["mu_x"].ptr(),
                                      ins["mu_y"].ptr(), ins["A"].ptr(), N, D, Dy, M, outs["out"].ptr())
    got = _twice(call, dict(x=x, posterior=post, mixture=mix, mu_x=mu_x, mu_y=mu_y, A=A), dict(out=((N, Dy), F64)),
                 what=("gmm_convert", form))["out"]
    per = mu_y[None] + np.einsum("myd,nmd->nmy", A, x[:, None, :] - mu_x[None])                 # (N, M, Dy)
    want = np.einsum("nm,nmy->ny", post, per) if form == "posterior" else per[np.arange(N), mix]
    _close(got, want, 1e-10)


# ------------------------------------------------------------------------------------------------------------------- fastdtw

def _tracks(rng, t, D):
    return np.cumsum(rng.randn(t, D), 0) * 0.1


def _dtw_cell(pairs, radius, tie, check, kind=0, scale=1.0, dist=None):
    """kind / scale: MLPG_HIP_DIST_* and its factor.  dist: the numpy callable of an _NP kind -- the reference is then the literal
    restatement of fastdtw driven by it (a Python call per window cell: small pairs only), else the C oracle."""
    L, dev, stream = _call()
    N, D = len(pairs), pairs[0][0].shape[1]
    Tx, Ty = max(len(x) for x, _ in pairs), max(len(y) for _, y in pairs)
    X, Y = np.zeros((N, Tx, D)), np.zeros((N, Ty, D))
    for n, (x, y) in enumerate(pairs):
        X[n, :len(x)], Y[n, :len(y)] = x, y
    lenx = np.array([len(x) for x, _ in pairs], dtype=np.int32)
    leny = np.array([len(y) for _, y in pairs], dtype=np.int32)

    def call(ins, outs, works):
        return L.mlpg_hip_fastdtw(dev, stream, ins["X"].ptr(), ins["Y"].ptr(), ins["lenx"].ptr(), ins["leny"].ptr(), N, Tx, Ty, D,
                                  radius, kind, scale, tie, outs["path_i"].ptr(), outs["path_j"].ptr(), outs["path_len"].ptr(),
                                  outs["cost"].ptr())

    def same(a, b):
        assert np.array_equal(a["path_len"], b["path_len"]) and a["cost"].tobytes() == b["cost"].tobytes()
        for n in range(N):
            k = a["path_len"][n]
            assert np.array_equal(a["path_i"][n, :k], b["path_i"][n, :k]) and np.array_equal(a["path_j"][n, :k], b["path_j"][n, :k]), n
    got = _twice(call, dict(X=X, Y=Y, lenx=lenx, leny=leny),
                 dict(path_i=((N, Tx + Ty), np.int32), path_j=((N, Tx + Ty), np.int32), path_len=((N,), np.int32), cost=((N,), F64)),
                 same=same, what=("fastdtw", D, radius, tie, N, kind))
    pi, pj, pl, cost = got["path_i"], got["path_j"], got["path_len"], got["cost"]
    assert (pl > 0).all() and (pl <= Tx + Ty).all()
    for n in check:
        x, y = pairs[n]
        if dist is None:
            d, path = OD.fastdtw(x, y, radius, tie=tie)
        else:
            d, path = OD.fastdtw_py(x, y, radius, dist, tie=tie)
            path = np.asarray(path)
        assert pl[n] == len(path), n
        assert np.array_equal(pi[n, :pl[n]], path[:, 0]) and np.array_equal(pj[n, :pl[n]], path[:, 1]), n
        assert abs(cost[n] - d) <= 1e-12 * max(d, 1e-300), n


# D = 13: one full batch of the paired cost, a remainder batch and an odd last element; D = 60: seven full batches and a remainder
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("D", [3, 13, 25, 60])
def test_fastdtw(D, radius, tie):
    rng = np.random.RandomState(100 * D + 10 * radius + tie)
    sizes = [(1, 1), (7, 300), (129, 64), (40, 3)]
    pairs = [(_tracks(rng, tx, D), _tracks(rng, ty, D)) for tx, ty in sizes]
    _dtw_cell(pairs, radius, tie, range(len(pairs)))


@pytest.mark.parametrize("D", [8, 13])
@pytest.mark.parametrize("form", [NP_L2, NP_L1, NP_SQL2])
def test_fastdtw_numpy_order_kinds(form, D):
    """The MLPG_HIP_DIST_SCALED_*_NP kinds (numpy's summation order: D = 8 is one block of eight without a tail, D = 13 a block and a
    tail of five) on the same guarded buffers, against the restatement driven by the numpy expression each kind stands for."""
    rng = np.random.RandomState(1000 * form + D)
    sizes = [(1, 1), (40, 3), (33, 17), (9, 40)]
    pairs = [(_tracks(rng, tx, D), _tracks(rng, ty, D)) for tx, ty in sizes]
    _dtw_cell(pairs, 1, 0, range(len(pairs)), kind=form + 1, scale=NP_SCALES[form], dist=NP_DISTS[form])


def test_fastdtw_two_launch_form():
    """More than 512 pairs: the two-launch form (tests/test_dtw_gpu.py); every 13th pair against the oracle."""
    rng = np.random.RandomState(520)
    pairs = [(_tracks(rng, int(rng.randint(5, 41)), 3), _tracks(rng, int(rng.randint(5, 41)), 3)) for _ in range(520)]
    _dtw_cell(pairs, 1, 0, range(0, 520, 13))


# ------------------------------------------------------------------------------------- float64 modulation spectrum, three routes

def _per_utt(f, *arrs):
    return np.stack([f(*[a[b] for a in arrs]) for b in range(arrs[0].shape[0])])


@pytest.mark.parametrize("route,n", [("fft", 16), ("chirp", 12), ("direct", 12)])
def test_modspec_entries(route, n):
    """mlpg_hip_modspec (phase present and NULL), _inv_modspec, _modspec_smoothing and _modspec_backward at B = 2, T = 10, D = 3 (an
    unpaired last column) against oracle/modspec.py at the bounds of tests/test_modspec_chirp_gpu.py::test_parity_and_route."""
    from nnmnkwii_amd import _hip
    L, dev, stream = _call()
    B, T, D = 2, 10, 3
    nb = n // 2 + 1
    rng = np.random.RandomState(n)
    x = 0.1 * np.cumsum(rng.randn(B, T, D), axis=-2) + rng.rand(B, T, D)
    w = rng.rand(B, nb, D)
    L.mlpg_hip_modspec_set_direct(1 if route == "direct" else 0)
    try:
        assert _hip.modspec_route(n) == {"fft": 0, "direct": 1, "chirp": 2}[route]
        for ortho, norm in ((0, None), (1, "ortho")):
            what = ("modspec", route, n, norm)
            mo = _per_utt(lambda a: OM.modspec(a, n=n, norm=norm), x)
            po = _per_utt(lambda a: OM.modspec(a, n=n, norm=norm, return_phase=True)[1], x)
            for want_phase in (True, False):
                def call(ins, outs, works):
                    return L.mlpg_hip_modspec(dev, stream, ins["x"].ptr(), B, T, D, n, ortho, outs["ms"].ptr(), ptr(outs.get("phase")))
                shapes = dict(ms=((B, nb, D), F64))
                if want_phase:
                    shapes["phase"] = ((B, nb, D, 2), F64)
                got = _twice(call, dict(x=x), shapes, what=what + ("phase" if want_phase else "no phase",))
                _close(got["ms"], mo, 1e-11, what)
                if want_phase:
                    ph = got["phase"][..., 0] + 1j * got["phase"][..., 1]
                    big = mo > 1e-6 * mo.max()                    # the phase of a vanishing bin is noise
                    assert np.abs(ph - po)[big].max() < 1e-8, what

            phase_in = np.ascontiguousarray(np.stack([po.real, po.imag], axis=-1))

            def call(ins, outs, works):
                return L.mlpg_hip_inv_modspec(dev, stream, ins["ms"].ptr(), ins["phase"].ptr(), B, n, D, ortho, outs["out"].ptr())
            got = _twice(call, dict(ms=mo, phase=phase_in), dict(out=((B, n, D), F64)), what=what + ("inverse",))
            _close(got["out"], _per_utt(lambda m, p: OM.inv_modspec(m, p, norm=norm), mo, po), 1e-11, what)

            for log_domain in (1, 0):
                limit_bin = int(n * 25 / 200) + 1

                def call(ins, outs, works):
                    return L.mlpg_hip_modspec_smoothing(dev, stream, ins["x"].ptr(), B, T, D, n, ortho, limit_bin, log_domain,
                                                        outs["out"].ptr())
                got = _twice(call, dict(x=x), dict(out=((B, T, D), F64)), what=what + ("smoothing", log_domain))
                yo = _per_utt(lambda a: OM.modspec_smoothing(a, 200, n=n, norm=norm, cutoff=25, log_domain=bool(log_domain)), x)
                _close(got["out"], yo, 1e-9, what)

            def call(ins, outs, works):
                return L.mlpg_hip_modspec_backward(dev, stream, ins["x"].ptr(), ins["grad_ms"].ptr(), B, T, D, n, ortho,
                                                   outs["grad_x"].ptr())
            got = _twice(call, dict(x=x, grad_ms=w), dict(grad_x=((B, T, D), F64)), what=what + ("backward",))
            _close(got["grad_x"], _per_utt(lambda a, g: OM.modspec_grad(a, g, n, norm), x, w), 1e-10, what)
    finally:
        L.mlpg_hip_modspec_set_direct(0)


# --------------------------------------------------------------------------------------------- padded minibatch and the loss step

TOL_BATCH = {F64: dict(ms=1e-11, grad=1e-10, loss=1e-11), F32: dict(ms=2e-6, grad=5e-6, loss=2e-6)}     # tests/test_modspec_batch_gpu.py


@pytest.mark.parametrize("n", [16, 12])
@pytest.mark.parametrize("dt", [F32, F64])
def test_modspec_batch_entries(dt, n):
    """mlpg_hip_modspec_batch, _batch_backward and _loss_step on a ragged batch (one utterance longer than n, one empty) against
    tests/modspec_batch64.py evaluated in float64 on the inputs as the kernel receives them."""
    L, dev, stream = _call()
    B, T, D = 3, 20, 3
    nb = n // 2 + 1
    tol = TOL_BATCH[dt]
    lens = np.array([20, 7, 0], dtype=np.int32)
    rng = np.random.RandomState(n)
    x = R.make_batch(rng, B, T, D, lens, pad=np.nan).astype(dt)
    g = rng.rand(B, nb, D).astype(dt)
    tgt = (R.modspec(R.make_batch(rng, B, T, D, lens, pad=0.0), n, None, lens) + 0.01).astype(dt)
    x64, g64, tgt64 = x.astype(F64), g.astype(F64), tgt.astype(F64)
    for ortho, norm in ((0, None), (1, "ortho")):
        what = ("modspec_batch", dt.__name__, n, norm)

        def call(ins, outs, works):
            return L.mlpg_hip_modspec_batch(dev, stream, DT_ID[dt], ins["x"].ptr(), ins["lengths"].ptr(), B, T, D, n, ortho,
                                            outs["ms"].ptr())
        got = _twice(call, dict(x=x, lengths=lens), dict(ms=((B, nb, D), dt)), what=what)
        _close(got["ms"], R.modspec(x64, n, norm, lens), tol["ms"], what)

        def call(ins, outs, works):
            return L.mlpg_hip_modspec_batch_backward(dev, stream, DT_ID[dt], ins["x"].ptr(), ins["grad_ms"].ptr(), ins["lengths"].ptr(),
                                                     B, T, D, n, ortho, outs["grad_x"].ptr())
        got = _twice(call, dict(x=x, grad_ms=g, lengths=lens), dict(grad_x=((B, T, D), dt)), what=what + ("backward",))
        live = R.live_frames(lens, B, T, n)
        for b in range(B):
            assert not got["grad_x"][b, live[b]:].any(), what          # every row is written: 0 from min(length, n) on
        _close(got["grad_x"], R.modspec_grad(x64, g64, n, norm, lens), tol["grad"], what)

        ws_bytes = int(L.mlpg_hip_modspec_loss_workspace_bytes(B, D))
        n_elems = float(B * nb * D)
        for log_domain in (1, 0):
            def call(ins, outs, works):
                return L.mlpg_hip_modspec_loss_step(dev, stream, DT_ID[dt], ins["x"].ptr(), ins["target_ms"].ptr(), ins["lengths"].ptr(),
                                                    B, T, D, n, ortho, log_domain, 1e-10, n_elems, outs["grad_x"].ptr(),
                                                    outs["loss"].ptr(), works["ws"].ptr(), ws_bytes)
            shapes = dict(grad_x=((B, T, D), dt), loss=((1,), F64))
            if not L.mlpg_hip_modspec_loss_form(n):
                # a length the fused step does not take: refused, and nothing is touched
                ins = {k: embedded(a, 1) for k, a in dict(x=x, target_ms=tgt, lengths=lens).items()}
                outs = {k: Embedded(s, d, 0, 0xA5) for k, (s, d) in shapes.items()}
                works = dict(ws=Workspace(ws_bytes, 8))
                assert call(ins, outs, works) == EINVAL
                torch.cuda.synchronize()
                assert not failed(ins, outs, works)
                assert all(bool((b.bytes_view() == 0xA5).all()) for b in list(outs.values()) + [works["ws"]])
                continue
            got = _twice(call, dict(x=x, target_ms=tgt, lengths=lens), shapes, work=dict(ws=(ws_bytes, 8)),
                         what=what + ("loss", log_domain))
            want, wgrad = R.loss_and_grad(x64, tgt64, n, norm, lens, bool(log_domain), 1e-10, n_elems)
            _close(got["loss"], np.array([want]), tol["loss"], what + ("loss",))
            _close(got["grad_x"], wgrad, tol["grad"], what + ("loss grad",))
