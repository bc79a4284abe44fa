"""GPU tests (-m gpu): mlpg_hip_backward_var and the batched autograd MLPG (autograd.mlpg_batch / MLPGBatch) that rests on it,
against tests/vargrad64.py (float64, numpy only; pinned by tests/test_vargrad64_cpu.py to complex-step derivatives).

The route matrix: the solve families (natural-order, wave, strip, constant-coefficient, chunked) and AUTO x float32 / float64 x
per-frame / global variances x the window sets of tests/golden/cases.py x utterance lengths 1 .. 4100 x no lengths / ragged
lengths down to 0 x 1, 5 and 70 static dims (1 and 16 beyond 1000 frames).  An accepted cell moves its family's counter and the
variance-gradient kernel's (kind 13) by one each, returns status 0, gives a grad_mean bit-identical to mlpg_hip_backward by the
same algo and a grad_var within 1e-10 (float64) / 3e-6 (float32) of the utterance's largest |grad_var|, with exact zeros at
padding rows and masked entries.  Float32: grad_var = -grad_mean tau (mu - W y) is evaluated in float64 from three float32
roundings -- grad_mean (relative 2^-24), y (|W y| off by at most 2^-24 sum|c| max|y|, sum|c| <= 5.4 for these windows) and the
output (2^-24) -- so with O(1) residuals mu - W y the error is a few 1e-7 of the largest entry; 3e-6 holds with room.
A refused cell gets EINVAL naming the algo and moves no counter (kind 13 included).  Then padding, masked entries, a failing
system, the scale invariant, gradcheck, the autograd surface, streams and graphs."""
import numpy as np
import pytest

import vargrad64
from cases import WINDOW_SETS
from test_backward_routes_gpu import ALGO_NAMES, FAMILIES, _ragged, _sds, _warm_fir, supported

pytestmark = pytest.mark.gpu

SOLVE_FAMILIES = ("generic", "wave", "strip", "const", "chunk")
KINDS = {kind: fam for fam, (_, kind) in FAMILIES.items()}
VARGRAD_KIND = 13
TS = [1, 2, 3, 5, 17, 65, 257, 1000, 2049, 4100]
WNAMES = ["std3", "std2", "asym2", "wide3", "zero2", "static"]


def _counts():
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return {k: L.mlpg_hip_launch_count(k) for k in list(KINDS) + [VARGRAD_KIND]}


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _masked(windows, lengths, T, sd):
    """Boolean (B, T, D): entries whose precision the edge mask (or the [-0:] rule) removes, within the live rows."""
    nw = len(windows)
    mw = max(max(l, u) for l, u, _ in windows)
    t = np.arange(T)[None, :]
    L = np.asarray(lengths)[:, None]
    live = t < L
    dyn = live & ((t < mw) | (t >= L - mw)) if mw > 0 else live
    out = np.zeros((len(lengths), T, nw * sd), dtype=bool)
    for w in range(1, nw):
        out[:, :, w * sd:(w + 1) * sd] = dyn[:, :, None]
    return out


def _terms(M, V, y, gm, windows):
    """Per utterance, the largest |grad_mean tau| (|mu| + |W y|) -- the size of the terms whose difference is grad_var."""
    S = max(float(np.abs(np.asarray(c, dtype=np.float64)).sum()) for _, _, c in windows)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(V != 0, (V.dtype.type(1) / V).astype(np.float64), 0.0)
    ymax = np.abs(y).max(axis=(1, 2))[:, None, None]
    return (np.abs(gm) * np.abs(tau) * (np.abs(M.astype(np.float64)) + S * ymax)).max(axis=(1, 2))


def _check_var_grad(gv, ref, lengths, masked, tol, what, terms):
    """Padding rows and masked entries exactly 0; |gv - ref| <= tol * the utterance's largest |ref|.  Where grad_var cancels
    (static-only or fully masked window sets: y = mu, grad_var is 0 up to rounding) that bar is taken against 1/20 of the size
    of its terms instead -- with O(1) residuals the largest |grad_var| is above that, and the bar is the plain one."""
    gv = gv.astype(np.float64)
    B, T, _ = gv.shape
    pad = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
    assert not gv[pad].any(), (what, "padding rows not zero")
    assert not gv[masked].any(), (what, "masked entries not zero")
    err = np.abs(gv - ref).max(axis=(1, 2))
    scale = np.maximum(np.abs(ref).max(axis=(1, 2)), 0.05 * terms)
    assert (err <= tol * scale).all(), (what, (err / np.where(scale > 0, scale, 1)).tolist())


def _cell(fam, m, v, y, g, windows, L, dt, mode, T, has_l):
    """One route cell: (family taken, grad_mean, grad_var) as numpy, or None when refused (after checking the refusal)."""
    import torch
    from nnmnkwii_amd import _hip
    algo = 0 if fam == "auto" else FAMILIES[fam][0]
    c0 = _counts()
    if fam != "auto" and not supported(fam, windows, mode, dt, dt, T, has_l):
        with pytest.raises(_hip.HipExtensionError) as ei:
            _hip.backward_var(m, v, y, g, windows, L, algo=algo)
        assert "failed (-1)" in str(ei.value) and "MLPG_HIP_ALGO_%s" % ALGO_NAMES[algo] in str(ei.value), str(ei.value)
        assert _counts() == c0, (fam, "a refused cell ran a kernel")
        return None
    gm, gv, st = _hip.backward_var(m, v, y, g, windows, L, algo=algo)
    torch.cuda.synchronize()
    moved = {k: n - c0[k] for k, n in _counts().items() if n != c0[k]}
    assert moved.pop(VARGRAD_KIND, None) == 1, (fam, "variance-gradient kernel", moved)
    assert len(moved) == 1 and list(moved.values()) == [1], (fam, moved)
    took = KINDS[next(iter(moved))]
    if fam != "auto":
        assert took == fam, (fam, took)
    assert int(st.abs().max()) == 0, (fam, "status")
    gm_ref, _ = _hip.backward(v, g, windows, m.shape[2], L, out_dtype=m.dtype, algo=algo)
    assert torch.equal(gm, gm_ref), (fam, "grad_mean differs from mlpg_hip_backward")
    return took, gm.cpu().numpy(), gv.cpu().numpy()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("wname", WNAMES)
def test_backward_var_route_matrix(wname, T):
    import torch
    from nnmnkwii_amd import _hip
    windows = WINDOW_SETS[wname]
    nw = len(windows)
    _warm_fir(windows)
    for sd in _sds(T):
        D = nw * sd
        rng = np.random.RandomState(T * 1000 + sd * 10 + nw)
        # 7 utterances: 2 without lengths, 5 with ragged ones
        M = rng.randn(7, T, D)
        V = rng.rand(7, T, D) + 0.1
        vg = rng.rand(D) + 0.1
        go = rng.randn(7, T, sd)
        rag = _ragged(T)
        lens7 = np.concatenate([[T, T], rag])
        for dt in (np.float32, np.float64):
            tol = 1e-10 if dt == np.float64 else 3e-6
            # one reference call for both modes (global restated as per-frame arrays of the same values: per-frame contributions)
            Mall = np.concatenate([M, M]).astype(dt)
            Vall = np.concatenate([V, np.broadcast_to(vg, V.shape)]).astype(dt)
            goall = np.concatenate([go, go]).astype(dt)
            y_ref_all, gm_ref_all, gv_ref_all = vargrad64.mlpg_var_grad64(Mall, Vall, goall, windows, np.tile(lens7, 2))
            terms_all = _terms(Mall, Vall, y_ref_all, gm_ref_all, windows)
            for mi, mode in enumerate(("frame", "global")):
                for lk, sl in (("none", slice(0, 2)), ("ragged", slice(2, 7))):
                    has_l = lk == "ragged"
                    lens = lens7[sl]
                    m, g = _dev(M[sl].astype(dt)), _dev(go[sl].astype(dt))
                    v = _dev(V[sl].astype(dt)) if mode == "frame" else _dev(vg.astype(dt))
                    L = _dev(rag) if has_l else None
                    y, _ = _hip.forward(m, v, windows, L)
                    ref = gv_ref_all[7 * mi:7 * mi + 7][sl]
                    masked = _masked(windows, lens, T, sd)
                    for fam in SOLVE_FAMILIES + ("auto",):
                        res = _cell(fam, m, v, y, g, windows, L, dt, mode, T, has_l)
                        if res is None:
                            continue
                        took, gm, gv = res
                        what = (wname, T, sd, dt.__name__, mode, lk, fam, took)
                        _check_var_grad(gv, ref, lens, masked, tol, what, terms_all[7 * mi:7 * mi + 7][sl])
                        gmr = gm_ref_all[7 * mi:7 * mi + 7][sl]
                        err = np.abs(gm.astype(np.float64) - gmr).max()
                        assert err <= tol * max(np.abs(gmr).max(), 1e-300), what + ("grad_mean",)
                    del y
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- padding, masks, status

def _problem(wname, B, T, sd, dt, seed, lens=None):
    windows = WINDOW_SETS[wname]
    D = len(windows) * sd
    rng = np.random.RandomState(seed)
    if lens is None:
        lens = np.concatenate([_ragged(T), rng.randint(0, T + 1, size=B - 5)]).astype(np.int32)
    live = (np.arange(T)[None, :] < lens[:, None])[:, :, None]
    M = (rng.randn(B, T, D) * live).astype(dt)
    V = ((rng.rand(B, T, D) + 0.1) * live).astype(dt)
    go = (rng.randn(B, T, sd) * live).astype(dt)
    return windows, M, V, go, lens


def _run(M, V, go, windows, lens, algo=0, y=None):
    import torch
    from nnmnkwii_amd import _hip
    m, v, g, L = _dev(M), _dev(V), _dev(go), _dev(lens)
    if y is None:
        y, _ = _hip.forward(m, v, windows, L)
    else:
        y = _dev(y)
    gm, gv, st = _hip.backward_var(m, v, y, g, windows, L, algo=algo)
    torch.cuda.synchronize()
    return y.cpu().numpy(), gm.cpu().numpy(), gv.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("wname", ["std3", "wide3", "asym2"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_padding_is_never_read(wname, dt):
    """NaN, 0 or -1 in the padding rows of mean, var, y and grad_out: every live row of both gradients bit-identical."""
    for B, T, sd in ((5, 200, 5), (5, 200, 70), (16, 130, 5)):
        windows, M, V, go, lens = _problem(wname, B, T, sd, dt, B * T + sd)
        pad = np.arange(T)[None, :] >= lens[:, None]
        for mode in ("frame", "global"):
            for fam in SOLVE_FAMILIES + ("auto",):
                algo = 0 if fam == "auto" else FAMILIES[fam][0]
                if fam != "auto" and not supported(fam, windows, mode, dt, dt, T, True):
                    continue
                res = []
                for dirty in (False, True):
                    Mx, Vx, gx = M.copy(), V.copy(), go.copy()
                    vv = Vx if mode == "frame" else V[0, 0].copy()
                    y0 = _run(M, vv, go, windows, lens, algo)[0]
                    if dirty:
                        junk = np.array([np.nan, 0.0, -1.0], dtype=dt)
                        for b, L in enumerate(lens):
                            n = T - L
                            Vx[b, L:] = junk[np.arange(n) % 3][:, None]
                            Mx[b, L:] = junk[(np.arange(n) + 1) % 3][:, None]
                            gx[b, L:] = np.nan
                            y0[b, L:] = junk[(np.arange(n) + 2) % 3][:, None]
                        vv = Vx if mode == "frame" else vv
                    res.append(_run(Mx, vv, gx, windows, lens, algo, y=y0))
                (_, gm0, gv0, s0), (_, gm1, gv1, s1) = res
                what = (wname, dt.__name__, B, T, sd, mode, fam)
                assert np.array_equal(s0, s1) and not s0.any(), what
                for a0, a1 in ((gm0, gm1), (gv0, gv1)):
                    assert not a0[pad].any() and not a1[pad].any(), what + ("padding",)
                    assert np.array_equal(a0[~pad], a1[~pad]), what + ("live rows differ",)


@pytest.mark.parametrize("wname", ["std3", "wide3", "asym2", "zero2"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_masked_variance_entries_are_never_read(wname, dt):
    """Masked entries of per-frame variances filled with 0, -1 and NaN: grad_var exactly 0 there, every other live entry of
    both gradients bit-identical, on every family that takes per-frame variances -- except the strip family, which is left out
    of this one check by name: its backward solve reads masked entries (a 0 there fails the factorisation, status -2), a
    finding about the existing kernel that this change does not touch."""
    B, T, sd = 6, 150, 5
    windows, M, V, go, lens = _problem(wname, B, T, sd, dt, 77)
    masked = _masked(windows, lens, T, sd)
    pad = np.arange(T)[None, :] >= lens[:, None]
    keep = ~masked & ~pad[:, :, None]
    for fam in ("generic", "wave", "chunk", "auto"):
        algo = 0 if fam == "auto" else FAMILIES[fam][0]
        if fam != "auto" and not supported(fam, windows, "frame", dt, dt, T, True):
            continue
        y = _run(M, V, go, windows, lens, algo)[0]
        base = _run(M, V, go, windows, lens, algo, y=y)
        for fill in (0.0, -1.0, np.nan):
            Vx = V.copy()
            Vx[masked] = fill
            _, gm, gv, st = _run(M, Vx, go, windows, lens, algo, y=y)
            what = (wname, dt.__name__, fam, fill)
            assert not st.any() and not base[3].any(), what
            assert not gv[masked].any(), what + ("masked grad_var",)
            assert np.array_equal(gv[keep], base[2][keep]), what + ("grad_var",)
            assert np.array_equal(gm, base[1]), what + ("grad_mean",)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_failing_system(dt):
    """A negative variance in one system: its status is reported, its grad_var columns are 0, every other system is
    bit-identical to a run where that system is healthy."""
    B, T, sd = 5, 120, 5
    windows, M, V, go, lens = _problem("std3", B, T, sd, dt, 5, lens=np.array([120, 119, 60, 1, 90], dtype=np.int32))
    bad_b, bad_d = 2, 3
    Vb = V.copy()
    Vb[bad_b, 10:20, bad_d] = -1e-3
    for fam in ("generic", "wave", "strip", "chunk", "auto"):
        algo = 0 if fam == "auto" else FAMILIES[fam][0]
        _, gm0, gv0, s0 = _run(M, V, go, windows, lens, algo)
        _, gm1, gv1, s1 = _run(M, Vb, go, windows, lens, algo)
        st = s1.reshape(B, sd)
        assert st[bad_b, bad_d] != 0 and not s0.any(), fam
        st[bad_b, bad_d] = 0
        assert not st.any(), fam
        cols = [w * sd + bad_d for w in range(3)]
        assert not gv1[bad_b][:, cols].any(), fam
        other = np.ones((B, 3 * sd), dtype=bool)
        other[bad_b, cols] = False
        for a0, a1 in ((gv0, gv1), (gm0, gm1)):
            assert np.array_equal(a0.transpose(0, 2, 1)[other], a1.transpose(0, 2, 1)[other]), fam


def test_scale_invariant_on_gpu():
    """sum_{w,t} var grad_var = 0 per system (y does not change when a system's variances are scaled alike), float64."""
    for wname in WNAMES:
        B, T, sd = 6, 300, 7
        windows, M, V, go, lens = _problem(wname, B, T, sd, np.float64, 3)
        nw = len(windows)
        _, _, gv, st = _run(M, V, go, windows, lens)
        assert not st.any()
        prod = (V.astype(np.float64) * gv).reshape(B, T, nw, sd)
        s = prod.sum(axis=(1, 2))
        mag = np.abs(prod).sum(axis=(1, 2))
        floor = 1e-14 * np.abs(go).sum(axis=1) * np.abs(M).max()      # static-only / fully masked sets: grad_var is noise
        assert (np.abs(s) <= 1e-9 * mag + floor).all(), (wname, (np.abs(s) / np.maximum(mag, 1e-300)).max())


# ---------------------------------------------------------------------------------------------------- autograd

@pytest.mark.parametrize("wname", WNAMES)
def test_gradcheck(wname):
    """torch.autograd.gradcheck, float64, B = 2, ragged lengths, per-frame and global variances, both inputs requiring grad.
    Its finite differences use only the forward kernels: independent of both backward kernels."""
    import torch
    from nnmnkwii_amd import autograd as AF
    windows = WINDOW_SETS[wname]
    D = 2 * len(windows)
    for T in (1, 3, 9, 33):
        rng = np.random.RandomState(T)
        lengths = [T, max(T // 2, 1) if T > 1 else 0]
        m = torch.from_numpy(rng.randn(2, T, D)).cuda().requires_grad_()
        for v_np in (rng.rand(2, T, D) + 0.5, rng.rand(D) + 0.5):
            v = torch.from_numpy(v_np).cuda().requires_grad_()
            assert torch.autograd.gradcheck(lambda a, b: AF.mlpg_batch(a, b, windows, lengths), (m, v), eps=1e-6, atol=1e-6,
                                            rtol=1e-4), (wname, T, v_np.ndim)


def _ab(B=3, T=40, sd=4, dt=np.float64, wname="std3", seed=0):
    import torch
    windows = WINDOW_SETS[wname]
    D = len(windows) * sd
    rng = np.random.RandomState(seed)
    m = torch.from_numpy(rng.randn(B, T, D).astype(dt))
    v = torch.from_numpy((rng.rand(B, T, D) + 0.1).astype(dt))
    vg = torch.from_numpy((rng.rand(D) + 0.1).astype(dt))
    go = torch.from_numpy(rng.randn(B, T, sd).astype(dt))
    return windows, m, v, vg, go


def _grads(fn, m, v, go):
    m = m.detach().clone().requires_grad_()
    v = v.detach().clone().requires_grad_()
    y = fn(m, v)
    (y * go.to(y.device)).sum().backward()
    return y.detach(), m.grad, v.grad


def test_autograd_values_shapes_and_lengths_forms():
    import torch
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab()
    lens = np.array([40, 17, 0], dtype=np.int32)
    for dt in (torch.float64, torch.float32):
        mc, vc, vgc, goc = (t.to(dt).cuda() for t in (m, v, vg, go))
        for var in (vc, vgc):
            ref_y, ref_gm, ref_gv = vargrad64.mlpg_var_grad64(mc.cpu().numpy(), var.cpu().numpy(), goc.cpu().numpy(), windows, lens)
            outs = []
            for L in (lens, lens.tolist(), tuple(lens.tolist()), torch.from_numpy(lens), torch.from_numpy(lens).cuda(),
                      torch.from_numpy(lens.astype(np.int64))):
                y, gm, gv = _grads(lambda a, b: AF.mlpg_batch(a, b, windows, L), mc, var, goc)
                assert y.dtype == dt and y.device == mc.device and y.shape == (3, 40, 4)
                assert gm.shape == mc.shape and gv.shape == var.shape and gv.dtype == dt
                assert not y[1, 17:].any() and not y[2].any()
                outs.append((y, gm, gv))
            for o in outs[1:]:
                assert all(torch.equal(a, b) for a, b in zip(outs[0], o))
            y, gm, gv = outs[0]
            tol = 1e-10 if dt == torch.float64 else 3e-6
            for got, ref in ((y, ref_y), (gm, ref_gm), (gv, ref_gv)):
                got = got.double().cpu().numpy()
                assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), (dt, var.dim())
            # same values as the C ABI entry points
            yk, _ = _hip.forward(mc, var, windows, _dev(lens))
            assert torch.equal(y, yk)
    # 2-D inputs: the (T, D) form, no lengths and a one-element lengths
    y2, gm2, gv2 = _grads(lambda a, b: AF.mlpg_batch(a, b, windows), m[0].cuda(), v[0].cuda(), go[0])
    y3, gm3, gv3 = _grads(lambda a, b: AF.mlpg_batch(a, b, windows), m[:1].cuda(), v[:1].cuda(), go[:1])
    assert y2.shape == (40, 4) and torch.equal(y2, y3[0]) and torch.equal(gm2, gm3[0]) and torch.equal(gv2, gv3[0])
    y4, _, _ = _grads(lambda a, b: AF.mlpg_batch(a, b, windows, [20]), m[0].cuda(), v[0].cuda(), go[0])
    assert not y4[20:].any() and y4[:20].abs().sum() > 0
    with pytest.raises(TypeError):
        AF.mlpg_batch(m.cuda(), v.cuda().float(), windows)
    with pytest.raises(TypeError):
        AF.mlpg_batch(m.cuda().half(), v.cuda().half(), windows)


def test_means_only_and_variances_only():
    import torch
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab(dt=np.float32)
    mc, vc, goc = m.cuda(), v.cuda(), go.cuda()
    _, gm_both, gv_both = _grads(lambda a, b: AF.mlpg_batch(a, b, windows), mc, vc, goc)
    L = _hip.lib()
    # means only: mlpg_hip_backward, the variance-gradient kernel does not run
    mm = mc.clone().requires_grad_()
    y = AF.mlpg_batch(mm, vc, windows)
    torch.cuda.synchronize()
    k0 = L.mlpg_hip_launch_count(VARGRAD_KIND)
    (y * goc).sum().backward()
    torch.cuda.synchronize()
    assert L.mlpg_hip_launch_count(VARGRAD_KIND) == k0
    assert torch.equal(mm.grad, gm_both)
    # variances only
    vv = vc.clone().requires_grad_()
    y = AF.mlpg_batch(mc, vv, windows)
    (y * goc).sum().backward()
    torch.cuda.synchronize()
    assert L.mlpg_hip_launch_count(VARGRAD_KIND) == k0 + 1
    assert torch.equal(vv.grad, gv_both)


def test_global_variance_gradient():
    """(D,) variances: the gradient has shape (D,) and is the sum over utterances and live frames (the padding counts nothing)."""
    import torch
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab(B=4, T=50, sd=3)
    lens = np.array([50, 31, 7, 0], dtype=np.int32)
    _, gm, gv = _grads(lambda a, b: AF.mlpg_batch(a, b, windows, lens), m.cuda(), vg.cuda(), go.cuda())
    assert gv.shape == vg.shape
    _, ref_gm, ref_gv = vargrad64.mlpg_var_grad64(m.numpy(), vg.numpy(), go.numpy(), windows, lens)
    assert np.abs(gv.cpu().numpy() - ref_gv).max() <= 1e-10 * np.abs(ref_gv).max()
    assert np.abs(gm.cpu().numpy() - ref_gm).max() <= 1e-10 * np.abs(ref_gm).max()
    # the padding frames of a batch hold nothing: the same utterances one by one sum to the same gradient
    parts = []
    for b in range(4):
        if lens[b] == 0:
            continue
        _, _, g = _grads(lambda a, c: AF.mlpg_batch(a, c, windows), m[b, :lens[b]].cuda(), vg.cuda(), go[b, :lens[b]])
        parts.append(g.cpu().numpy())
    assert np.abs(gv.cpu().numpy() - np.sum(parts, axis=0)).max() <= 1e-12 * np.abs(ref_gv).max()


def test_cpu_tensors_match_cuda():
    import torch
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab()
    lens = [40, 12, 33]
    for var in (v, vg):
        yc, gmc, gvc = _grads(lambda a, b: AF.mlpg_batch(a, b, windows, lens), m, var, go)
        yg, gmg, gvg = _grads(lambda a, b: AF.mlpg_batch(a, b, windows, lens), m.cuda(), var.cuda(), go)
        assert yc.device.type == "cpu" and gmc.device.type == "cpu" and gvc.device.type == "cpu"
        assert torch.equal(yc, yg.cpu()) and torch.equal(gmc, gmg.cpu()) and torch.equal(gvc, gvg.cpu())


def test_linalg_error_under_check_status(monkeypatch):
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd.autograd import _mlpg
    windows, m, v, vg, go = _ab()
    vb = v.clone()
    vb[1, 10:20, 2] = -1e-3
    monkeypatch.setattr(_mlpg, "CHECK_STATUS", True)
    with pytest.raises(np.linalg.LinAlgError):
        AF.mlpg_batch(m.cuda(), vb.cuda(), windows)


def test_double_backward_raises():
    import torch
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab()
    mm, vv = m.cuda().requires_grad_(), v.cuda().requires_grad_()
    y = AF.mlpg_batch(mm, vv, windows)
    gm, gv = torch.autograd.grad((y * go.cuda()).sum(), (mm, vv), create_graph=True)
    with pytest.raises(RuntimeError):
        (gm.sum() + gv.sum()).backward()


def test_float32_2d_matches_autograd_mlpg():
    """A 2-D float32 CUDA call: value and means-gradient bit-identical to autograd.mlpg's."""
    import torch
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab(dt=np.float32, T=300, sd=6)
    a = m[0].cuda().requires_grad_()
    b = m[0].cuda().requires_grad_()
    ya = AF.mlpg(a, v[0].cuda(), windows)
    yb = AF.mlpg_batch(b, v[0].cuda(), windows)
    assert torch.equal(ya, yb)
    (ya * go[0].cuda()).sum().backward()
    (yb * go[0].cuda()).sum().backward()
    assert torch.equal(a.grad, b.grad)


# ---------------------------------------------------------------------------------------------------- streams and graphs

def test_non_default_stream_ordering():
    import torch
    from nnmnkwii_amd import autograd as AF
    windows, m, v, vg, go = _ab(B=8, T=1000, sd=60)
    ref = _grads(lambda a, b: AF.mlpg_batch(a, b, windows), m.cuda(), v.cuda(), go.cuda())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        mc, vc, gc = m.cuda(non_blocking=False), v.cuda(), go.cuda()
        out = _grads(lambda a, b: AF.mlpg_batch(a, b, windows), mc, vc, gc)
        res = [t.clone() for t in out]
    s.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ref, res))


def test_graph_capture_and_repeatability(monkeypatch):
    """CHECK_STATUS off: forward + backward capture after one eager step on the capture stream; two replays equal eager; two
    eager backward calls are bitwise repeatable (the global sum included)."""
    import torch
    from nnmnkwii_amd.autograd import _mlpg
    from nnmnkwii_amd import autograd as AF
    monkeypatch.setattr(_mlpg, "CHECK_STATUS", False)
    windows, m, v, vg, go = _ab(B=16, T=500, sd=20)
    lens = torch.from_numpy(np.random.RandomState(1).randint(0, 501, size=16).astype(np.int32)).cuda()
    for var in (v, vg):
        mc = m.cuda().requires_grad_()
        vc = var.cuda().requires_grad_()
        gc = go.cuda()

        def step():
            mc.grad = None
            vc.grad = None
            y = AF.mlpg_batch(mc, vc, windows, lens)
            (y * gc).sum().backward()
            return y

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            y_e = step()
            eager = (y_e.detach().clone(), mc.grad.clone(), vc.grad.clone())
            step()
            again = (mc.grad.clone(), vc.grad.clone())
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert torch.equal(eager[1], again[0]) and torch.equal(eager[2], again[1]), var.dim()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            y_g = step()
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(y_g, eager[0]) and torch.equal(mc.grad, eager[1]) and torch.equal(vc.grad, eager[2]), var.dim()
