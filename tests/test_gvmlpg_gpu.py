"""MLPG with the gv likelihood on the device: the kernels of mlpg_hip_gv_ascent and mlpg_hip_gv (csrc/mlpg_gv.hip) against the
numpy specification tools/gvmlpg_model.py through the C entry on guarded buffers at element offsets 0 and 1, then
``paramgen.mlpg_gv`` / ``mlpg_gv_batch`` and ``baseline.gmm.MLPG(gv=...)`` end to end.

Bounds.  Kernel against model on the same y_in: tests/gvmlpg_cases.py ``tolerance`` (8 times the worst distance of the kernel
text from the long-double model, measured by tests/test_gvmlpg_host_cpu.py; half a float32 ulp more for float32 storage).  Pad
frames: exactly 0.  Routes whose maximum-likelihood trajectory comes from different forward kernels, or whose E and D come from
the host on one side and the device on the other: rtol 1e-9, atol 1e-9 max|ref|, the bound of tests/test_gmmtraj_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import gvmlpg_cases as C
import gmm_em64 as R
from embed import Embedded, embedded, failed
from gvmlpg_cases import GV

pytestmark = pytest.mark.gpu

FILL32, FILL64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)
MLPG_KINDS = tuple(range(10))


def _lib():
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts():
    L = _lib()
    return [L.mlpg_hip_launch_count(k) for k in range(40)]


def run_entry(case, off=0, in_place=False, n_iter=100, step=None, init=1, omega_scale=1.0, windows=None, expect_rc=0, Tmax=None):
    """One call of mlpg_hip_gv_ascent on guarded buffers.  Returns (y_out, report, status) as numpy; checks the return code, the
    guards, that the inputs are unchanged, and that exactly one launch of kind 35 (or none, when refused) was counted."""
    from nnmnkwii_amd import _hip
    L = _lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    dt = case["dtype"]
    B, T, sd, D = case["B"], Tmax or case["Tmax"], case["sd"], case["D"]
    win = windows or case["windows"]
    wl, wu, wc = _hip.pack_windows(win)
    mode = GV.var_mode_of(case["var"])
    ins = dict(mean=embedded(case["mean"], off), var=embedded(case["var"], off), gv_mean=embedded(case["gv_mean"], off),
               gv_prec=embedded(case["gv_prec"], off))
    if case["lengths"] is not None:
        ins["lengths"] = embedded(np.asarray(case["lengths"], dtype=np.int32), off)
    y_in = embedded(case["y_in"], off)
    y_out = y_in if in_place else Embedded(case["y_in"].shape, dt, off)
    if not in_place:
        ins["y_in"] = y_in
    rep, st = Embedded((B, sd, 4), np.float64, off), Embedded((B, sd), np.int32, off)
    p = lambda b: None if b is None else ctypes.c_void_p(b.ptr())  # noqa: E731
    c0 = _counts()
    rc = L.mlpg_hip_gv_ascent(dev.index, _hip._stream(dev), int(dt == np.float64), p(ins["mean"]), p(ins["var"]), mode, p(ins.get("lengths")),
                              B, T, D, len(wl), wl.ctypes.data, wu.ctypes.data, wc.ctypes.data, p(y_in), p(y_out), p(ins["gv_mean"]),
                              p(ins["gv_prec"]), omega_scale, n_iter, -1.0 if step is None else step, init, p(rep), p(st))
    torch.cuda.synchronize()
    d = [b - a for a, b in zip(c0, _counts())]
    assert rc == expect_rc, (rc, L.mlpg_hip_last_error())
    assert d[35] == (1 if rc == 0 else 0) and sum(d) == d[35], d
    bad = failed(ins, dict(y_out=y_out, report=rep, status=st))
    assert not bad, bad
    return y_out.host(), rep.host(), st.host()


def check_against_model(case, y, rep, st, **kw):
    y_m, rep_m, st_m = C.model(case, **kw)
    live = GV.live_frames(case["lengths"], case["B"], case["Tmax"])
    pad = np.arange(case["Tmax"])[None, :] >= live[:, None]
    assert y.dtype == case["dtype"] and (y[pad] == 0).all()
    assert np.array_equal(st, st_m), (st, st_m)
    err = float(np.abs(y.astype(np.float64) - y_m).max())
    assert err <= C.tolerance(y_m, case["dtype"]), (err, C.tolerance(y_m, case["dtype"]))
    scale = np.abs(rep_m).max(axis=(0, 1)) + 1e-300
    assert (np.abs(rep - rep_m) <= 64 * C.BOUND_RATIO * C.EPS * scale).all()
    assert (rep[live == 0] == 0).all() and (st[live == 0] == 0).all()
    return err / max(C.tolerance(y_m, case["dtype"]), 1e-300)


LIVE = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257]


@pytest.mark.parametrize("dtype,off,in_place", [(np.float64, 0, False), (np.float32, 1, True)])
def test_every_chunk_size_boundary(dtype, off, in_place):
    case = C.make_case(11, len(LIVE), 257, 3, "std3", GV.VAR_FRAME, dtype, LIVE)
    y, rep, st = run_entry(case, off, in_place)
    print("worst error %.3f of the bound" % check_against_model(case, y, rep, st))
    assert (st == 0).all()


def test_one_system_at_the_longest_length():
    T = _lib().mlpg_hip_gv_max_frames()
    case = C.make_case(12, 1, T, 1, "std3", GV.VAR_FRAME, np.float64, None)
    y, rep, st = run_entry(case, 1)
    print("worst error %.3f of the bound" % check_against_model(case, y, rep, st))


@pytest.mark.parametrize("sd", [1, 3, 4, 5, 24])
def test_static_widths(sd):
    wname, mode = ("std3", "std2", "static")[sd % 3], (GV.VAR_FRAME, GV.VAR_GLOBAL, GV.VAR_UNIT)[sd % 2]
    case = C.make_case(sd, 2, 70, sd, wname, mode, np.float64 if sd % 2 else np.float32, [33, 70])
    for n_iter in (1, 100):
        y, rep, st = run_entry(case, sd % 2, in_place=bool(sd % 2), n_iter=n_iter)
        check_against_model(case, y, rep, st, n_iter=n_iter)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", [GV.VAR_FRAME, GV.VAR_GLOBAL, GV.VAR_UNIT])
@pytest.mark.parametrize("wname", ["std2", "std3", "static"])
def test_windows_variances_and_dtypes_on_a_ragged_batch(wname, mode, dtype):
    case = C.make_case(20 + mode, 5, 70, 2, wname, mode, dtype, [70, 0, 1, 69, 33])
    for off, in_place in ((0, True), (1, False)):
        y, rep, st = run_entry(case, off, in_place)
        check_against_model(case, y, rep, st)


@pytest.mark.parametrize("n_iter", [0, 1, 100])
@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("step", [None, 0.2])
def test_iterations_starts_and_steps(n_iter, init, step):
    case = C.make_case(31, 5, 70, 2, "std3", GV.VAR_FRAME, np.float64, [70, 0, 1, 69, 33])
    y, rep, st = run_entry(case, 1, n_iter=n_iter, step=step, init=init, omega_scale=1.0 if step is None else 1.5)
    check_against_model(case, y, rep, st, n_iter=n_iter, step=step, init=init, omega_scale=1.0 if step is None else 1.5)
    if n_iter == 0 and init == 0:
        assert y.tobytes() == case["y_in"].tobytes()           # pad frames of y_in are 0 already


def test_a_step_far_too_large_is_reported_and_raised():
    from nnmnkwii_amd import paramgen
    case = C.make_case(32, 2, 70, 2, "std3", GV.VAR_FRAME, np.float64, [70, 33])
    y, rep, st = run_entry(case, 0, step=1e7)
    assert np.isin(st, (1, 2)).all()
    assert np.array_equal(st, C.model(case, step=1e7)[2])
    with pytest.raises(ValueError, match="utterance 0, dim 0"):
        paramgen.mlpg_gv_batch(case["mean"], case["var"], case["windows"], case["gv_mean"], 1.0 / case["gv_prec"], case["lengths"], step=1e7)
    out = paramgen.mlpg_gv_batch(case["mean"], case["var"], case["windows"], case["gv_mean"], 1.0 / case["gv_prec"], case["lengths"],
                                 step=1e7, check=False, return_report=True)
    assert np.isin(out[2], (1, 2)).all()


def test_bits_do_not_depend_on_the_batch_or_the_call():
    lengths = [70, 0, 1, 69, 33]
    case = C.make_case(33, 5, 70, 3, "std3", GV.VAR_FRAME, np.float64, lengths)
    y, rep, st = run_entry(case)
    y2, rep2, st2 = run_entry(case)
    assert y.tobytes() == y2.tobytes() and rep.tobytes() == rep2.tobytes() and st.tobytes() == st2.tobytes()
    # the same utterances in another order, in a longer padded batch
    perm = [3, 0, 4, 2, 1]
    wide = lambda a: np.concatenate([a[perm], np.full((5, 13) + a.shape[2:], 3.25, dtype=a.dtype)], axis=1)  # noqa: E731
    other = dict(case, mean=wide(case["mean"]), var=wide(case["var"]), y_in=wide(case["y_in"]), lengths=[lengths[i] for i in perm], Tmax=83)
    yo, repo, _ = run_entry(other)
    for k, i in enumerate(perm):
        assert yo[k, :70].tobytes() == y[i].tobytes() and repo[k].tobytes() == rep[i].tobytes(), (k, i)
    # one utterance alone, cut to its own length
    sub = dict(case, mean=case["mean"][3:4, :69].copy(), var=case["var"][3:4, :69].copy(), y_in=case["y_in"][3:4, :69].copy(), lengths=None,
               B=1, Tmax=69)
    ys, reps, _ = run_entry(sub)
    assert ys[0].tobytes() == y[3, :69].tobytes() and reps[0].tobytes() == rep[3].tobytes()


def test_refused_shapes_launch_nothing_and_leave_the_output_alone():
    case = C.make_case(34, 1, 20, 2, "std2", GV.VAR_FRAME, np.float64, None)
    five_tap = [(0, 0, np.array([1.0])), (2, 2, np.array([0.1, -0.4, 0.0, 0.4, -0.1]))]
    for kw in (dict(windows=five_tap), dict(Tmax=_lib().mlpg_hip_gv_max_frames() + 1)):
        y, rep, st = run_entry(case, expect_rc=-1, **kw)       # run_entry asserts that no counter moved
        assert _lib().mlpg_hip_last_error().startswith(b"gv_ascent:")
        assert (y.view(np.uint64) == FILL64).all() and (rep.view(np.uint64) == FILL64).all() and (st.view(np.uint32) == FILL32).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_gv_of_a_column_slice(dtype):
    from nnmnkwii_amd import _hip, paramgen
    rng = np.random.RandomState(3)
    B, T, D = 4, 131, 5
    lengths = [131, 0, 1, 77]
    xw = (rng.randn(B, T, D + 3) * np.linspace(0.5, 4, D + 3) + 2.0).astype(dtype)
    xd, Ld = torch.from_numpy(xw).cuda(), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    c0 = _counts()
    g = _hip.gv(xd[:, :, :D], Ld)
    d = [b - a for a, b in zip(c0, _counts())]
    assert d[37] == 1 and sum(d) == 1
    ref = GV.gv_padded(xw[:, :, :D], lengths)
    gh = g.cpu().numpy()
    assert gh.dtype == np.float64 and (gh[1] == 0).all() and (gh[2] == 0).all()
    assert np.abs(gh - ref).max() <= 4 * T * C.EPS * float(np.abs(xw).max()) ** 2
    # the public forms: numpy and tensors, a single utterance, the statistics
    x = np.ascontiguousarray(xw[:, :, :D])
    assert np.array_equal(paramgen.gv(x, lengths), gh) and np.array_equal(paramgen.gv(xd[:, :, :D], Ld).cpu().numpy(), gh)
    assert np.array_equal(paramgen.gv(x[3, :77]), gh[3])
    mu, var = paramgen.gv_stats(x, lengths)
    assert np.array_equal(mu, gh[[0, 2, 3]].mean(axis=0)) and np.array_equal(var, gh[[0, 2, 3]].var(axis=0))


def close(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_paramgen_routes_agree_with_each_other_and_the_model(dtype):
    from nnmnkwii_amd import paramgen
    lengths = [70, 0, 1, 69, 33]
    case = C.make_case(41, 5, 70, 3, "std3", GV.VAR_FRAME, dtype, lengths)
    gm, gvar = case["gv_mean"], 1.0 / case["gv_prec"]
    md, vd = torch.from_numpy(case["mean"]).cuda(), torch.from_numpy(case["var"]).cuda()
    # the model on the trajectory the same forward route gives
    y0 = paramgen.mlpg_batch(md, vd, case["windows"], lengths)
    ref = C.model(dict(case, y_in=y0.cpu().numpy()), 30)
    c0 = _counts()
    yt, rep, st = paramgen.mlpg_gv_batch(md, vd, case["windows"], gm, gvar, lengths, n_iter=30, return_report=True)
    d = [b - a for a, b in zip(c0, _counts())]
    assert d[35] == 1 and sum(d[k] for k in MLPG_KINDS) == 1 and d[37] == 0
    assert torch.is_tensor(yt) and yt.is_cuda and yt.dtype == md.dtype and rep.shape == (5, 3, 4) and st.shape == (5, 3)
    yh = yt.cpu().numpy()
    assert np.abs(yh.astype(np.float64) - ref[0]).max() <= C.tolerance(ref[0], dtype) and np.array_equal(st.cpu().numpy(), ref[2])
    yn = paramgen.mlpg_gv_batch(case["mean"], case["var"], case["windows"], gm, gvar, lengths, n_iter=30)
    assert isinstance(yn, np.ndarray) and yn.tobytes() == yh.tobytes()
    for b in (0, 3, 4):                                         # one utterance at a time: another forward route, maybe
        n = lengths[b]
        y1 = paramgen.mlpg_gv(case["mean"][b, :n], case["var"][b, :n], case["windows"], gm, gvar, n_iter=30)
        assert y1.dtype == dtype and y1.shape == (n, 3)
        if dtype == np.float64:
            close(y1, yh[b, :n])
        else:
            np.testing.assert_allclose(y1, yh[b, :n], rtol=1e-5, atol=1e-6 * np.abs(yh).max())
    # global variances through the (T, D) form
    cg = C.make_case(42, 1, 50, 2, "std2", GV.VAR_GLOBAL, dtype, None)
    y1 = paramgen.mlpg_gv(cg["mean"][0], cg["var"], cg["windows"], cg["gv_mean"], 1.0 / cg["gv_prec"], n_iter=10)
    y0 = paramgen.mlpg_batch(torch.from_numpy(cg["mean"]).cuda(), torch.from_numpy(cg["var"]).cuda(), cg["windows"])
    ref = C.model(dict(cg, y_in=y0.cpu().numpy()), 10)[0]
    assert np.abs(y1.astype(np.float64) - ref[0]).max() <= C.tolerance(ref, dtype)


_models = {}


def joint_model():
    """The D = 6, K = 4 model of tests/test_gmmtraj_gpu.py."""
    from sklearn.mixture import GaussianMixture
    if not _models:
        import warnings
        D, K, n = 6, 4, 600
        rng = np.random.RandomState(3)
        src = R.synthetic(n, D, K, seed=3)
        tgt = src @ (np.eye(D) + 0.2 * rng.randn(D, D)) + 0.3 * rng.randn(n, D)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _models[0] = GaussianMixture(n_components=K, covariance_type="full", random_state=0, max_iter=100).fit(np.hstack([src, tgt])), src
    return _models[0]


LENS = [40, 1, 119, 0, 64]


@pytest.mark.parametrize("posterior", ["sklearn", "device"])
def test_gmm_conversion_with_gv(posterior):
    from nnmnkwii_amd import paramgen
    from nnmnkwii_amd.baseline.gmm import MLPG
    gmm, src = joint_model()
    windows = C.WINDOWS["std2"]
    plain = MLPG(gmm, windows=windows, posterior=posterior)
    sd = plain.static_dim
    offs = np.concatenate([[0], np.cumsum(LENS)])
    utts = [src[a:b] for a, b in zip(offs[:-1], offs[1:])]
    wlp = np.sort(plain.px._estimate_weighted_log_prob(np.concatenate(utts)), axis=1)
    assert (wlp[:, -1] - wlp[:, -2] > 1e-6).all()               # arg-max labels well apart: both routes pick the same mixtures
    y_plain = [plain.transform(u) if len(u) else np.zeros((0, sd)) for u in utts]
    # gv statistics above the gv of the plain conversion: it is over-smoothed
    g_plain = np.array([y.var(axis=0) for y, n in zip(y_plain, LENS) if n > 1])
    gv_mean = 1.8 * g_plain.mean(axis=0)
    gv_var = (0.2 * gv_mean) ** 2
    g = MLPG(gmm, windows=windows, posterior=posterior, gv=(gv_mean, gv_var), gv_options=dict(n_iter=50))
    # the model applied to the existing route's E, D and trajectory
    dg = lambda a: np.diagonal(a, axis1=1, axis2=2)  # noqa: E731
    Dm = dg(plain.covarYY) - dg(plain.covarYX) / dg(plain.covarXX) * dg(plain.covarXY)
    ref = []
    for u, y0 in zip(utts, y_plain):
        if not len(u):
            ref.append(np.zeros((0, sd)))
            continue
        E, mix = plain._convert_device(u, hard=True) if posterior == "device" else (None, plain.px.predict(u))
        if E is None:
            E = plain._convert(u, mix=mix)
        ref.append(GV.gv_ascent_padded(E[None], np.ascontiguousarray(Dm[mix])[None], windows, None, y0[None], gv_mean, 1.0 / gv_var,
                                       n_iter=50)[0][0])
    one = [g.transform(u) if len(u) else np.zeros((0, sd)) for u in utts]
    c0 = _counts()
    got = g.transform_batch(utts)
    d = [b - a for a, b in zip(c0, _counts())]
    assert d[35] == 1 and d[33] == 1 and d[22] == (1 if posterior == "device" else 0) and sum(d[k] for k in MLPG_KINDS) == 1
    assert sum(d[k] for k in MLPG_KINDS + (22, 33, 35)) == (4 if posterior == "device" else 3)
    Tmax = max(LENS)
    X = np.zeros((len(utts), Tmax, 6))
    for i, u in enumerate(utts):
        X[i, :len(u)] = u
    Y = g.transform_padded(torch.from_numpy(X).cuda(), torch.tensor(LENS, dtype=torch.int32, device="cuda"))
    assert torch.is_tensor(Y) and Y.dtype == torch.float64 and Y.shape == (len(utts), Tmax, sd)
    Yh = Y.cpu().numpy()
    for i, n in enumerate(LENS):
        assert (Yh[i, n:] == 0).all() and Yh[i, :n].tobytes() == got[i].tobytes() and got[i].shape == one[i].shape == (n, sd)
        if n:
            close(got[i], ref[i])
            close(one[i], ref[i])
        if n > 1:
            assert (np.abs(got[i].var(axis=0) - gv_mean) < np.abs(y_plain[i].var(axis=0) - gv_mean)).all(), i
    # gv=None is today's conversion, bit for bit
    again = MLPG(gmm, windows=windows, posterior=posterior, gv=None)
    for a, b in zip(again.transform_batch(utts), plain.transform_batch(utts)):
        assert a.tobytes() == b.tobytes()
    for a, u in zip(y_plain, utts):
        if len(u):
            assert again.transform(u).tobytes() == a.tobytes()
    assert paramgen.gv(got[2]).shape == (sd,)
