"""GPU tests (-m gpu): every backward route of mlpg_hip_backward against oracle/grad64.py, the float64 gradient that shares
no code with any kernel (tests/test_grad64_cpu.py pins it to the reference's mlpg_grad and to the oracle's forward pass).

The matrix: kernel families (natural-order, wave, strip, constant-coefficient, chunked, FIR, AUTO) x (input, output) dtype
pairs x per-frame / global / unit variances x the window sets of tests/golden/cases.py x utterance lengths from 1 to 4100
frames x no lengths / ragged lengths down to 0 frames x 1, 5 and 70 static dims.  A cell the library's support predicates
accept runs on its own family's kernel (launch counter + 1), returns status 0, matches the reference to 1e-10 (float64 in
and out) or 3e-6 (a float32 side) of the utterance's largest gradient and leaves its padding rows exactly 0; a cell they
reject is refused with the dispatcher's message and runs nothing.  Then the padding contract in both directions and the
user-facing callers (autograd.mlpg, autograd.unit_variance_mlpg, paramgen.mlpg_grad)."""
import numpy as np
import pytest

from cases import WINDOW_SETS
from oracle.grad64 import mlpg_grad64

pytestmark = pytest.mark.gpu

# family -> (algo, launch counter kind of mlpg_hip_launch_count); AUTO is checked to land on exactly one of them
FAMILIES = {"generic": (1, 0), "wave": (2, 1), "strip": (3, 2), "const": (5, 4), "chunk": (6, 6), "fir": (7, 7)}
KINDS = {kind: fam for fam, (_, kind) in FAMILIES.items()}
ALGO_NAMES = {1: "GENERIC", 2: "WAVE", 3: "STRIP", 5: "CONST", 6: "CHUNK", 7: "FIR"}
DT_PAIRS = [(np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float32), (np.float32, np.float64)]
MODES = ("frame", "global", "unit")
TS = [1, 2, 3, 5, 17, 41, 65, 129, 257, 1000, 2049, 4100]


def _sds(T):
    """Static dims per utterance length: 1, 5 and 70 (two 35-dim groups of the lane-per-dim kernels); 1 and 16 beyond 1000
    frames (16: the strip kernel's threshold for long utterances)."""
    return (1, 5, 70) if T <= 1000 else (1, 16)


def _ragged(T):
    return np.array([T, max(T - 1, 0), T // 2, 1, 0], dtype=np.int32)


def supported(fam, windows, mode, in_dt, out_dt, T, has_lengths):
    """The documented support predicates of csrc/mlpg_*.hip (wave_supported, strip_supported, const_supported,
    chunk_supported, fir_shape_supported) restated for dense problems of these sizes."""
    nw = len(windows)
    ext1 = all(l <= 1 and u <= 1 for l, u, _ in windows)
    mw = max(max(l, u) for l, u, _ in windows)
    if fam == "generic":
        return True
    if fam == "wave":
        return 1 <= T <= 2048 and ext1
    if fam == "strip":
        return (T + 63) // 64 <= 256 and ext1
    if fam == "const":
        return mode in ("global", "unit") and nw in (2, 3) and mw == 1 and ext1
    if fam == "chunk":
        return in_dt == out_dt and 1 <= nw <= 3 and 1 <= mw <= 2
    if fam == "fir":
        l0, u0, c0 = windows[0]
        return (in_dt == np.float32 and out_dt == np.float32 and mode == "unit" and not has_lengths and 1 <= nw <= 3
                and mw <= 2 and l0 == 0 and u0 == 0 and float(np.asarray(c0).ravel()[0]) != 0.0 and T >= 96)
    raise KeyError(fam)


def _counts():
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return {k: L.mlpg_hip_launch_count(k) for k in KINDS}


def _torch_dt(dt):
    import torch
    return torch.float32 if dt == np.float32 else torch.float64


def _to_dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_grad(grad, ref, lengths, tol, what):
    """Per utterance: |grad - ref| <= tol * max|ref of that utterance|; rows at and past its length exactly 0."""
    grad = grad.astype(np.float64)
    B, T, _ = grad.shape
    pad = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
    assert not grad[pad].any(), (what, "padding rows not zero")
    err = np.abs(grad - ref).max(axis=(1, 2))
    scale = np.abs(ref).max(axis=(1, 2))
    assert (err <= tol * scale).all(), (what, (err / np.where(scale > 0, scale, 1)).tolist())


def _warm_fir(windows):
    """The FIR form builds its tap table on first use per (device, window set) with one natural-order solve (csrc/mlpg_fir.hip
    table_for): build it before a cell counts launches."""
    import torch
    from nnmnkwii_amd import _hip
    if supported("fir", windows, "unit", np.float32, np.float32, 96, False):
        _hip.forward(torch.zeros((1, 96, len(windows)), dtype=torch.float32, device="cuda"), None, windows, algo=FAMILIES["fir"][0])
        torch.cuda.synchronize()


def _run_cell(fam, v, g, windows, D, L, in_dt, out_dt, mode, T, has_lengths):
    """One cell: returns the family AUTO took (or fam), the gradient (numpy) or None when refused."""
    import torch
    from nnmnkwii_amd import _hip
    algo = 0 if fam == "auto" else FAMILIES[fam][0]
    c0 = _counts()
    if fam != "auto" and not supported(fam, windows, mode, in_dt, out_dt, T, has_lengths):
        with pytest.raises(_hip.HipExtensionError) as ei:
            _hip.backward(v, g, windows, D, L, out_dtype=_torch_dt(out_dt), algo=algo)
        assert "failed (-1)" in str(ei.value) and "MLPG_HIP_ALGO_%s" % ALGO_NAMES[algo] in str(ei.value), str(ei.value)
        assert _counts() == c0, (fam, "a refused cell ran a kernel")
        return fam, None
    grad, st = _hip.backward(v, g, windows, D, L, out_dtype=_torch_dt(out_dt), algo=algo)
    torch.cuda.synchronize()
    moved = {k: n - c0[k] for k, n in _counts().items() if n != c0[k]}
    assert len(moved) == 1 and list(moved.values()) == [1], (fam, moved)
    took = KINDS[next(iter(moved))]
    if fam != "auto":
        assert took == fam, (fam, took)
    assert int(st.abs().max()) == 0, (fam, "status")
    out = grad.cpu().numpy()
    assert out.dtype == out_dt
    return took, out


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("wname", ["std3", "std2", "asym2", "wide3", "zero2", "static"])
def test_backward_route_matrix(wname, T):
    windows = WINDOW_SETS[wname]
    nw = len(windows)
    _warm_fir(windows)
    for sd in _sds(T):
        D = nw * sd
        rng = np.random.RandomState(T * 1000 + sd * 10 + nw)
        # 7 utterances: 2 without lengths, 5 with ragged ones; the same gradients under every variance mode
        V = rng.rand(7, T, D) + 0.1
        vg = rng.rand(D) + 0.1
        go = rng.randn(7, T, sd)
        rag = _ragged(T)
        lens7 = np.concatenate([[T, T], rag])
        for in_dt in (np.float32, np.float64):
            # one reference call for all three modes (global / unit restated as per-frame arrays of the same values)
            Vall = np.concatenate([V, np.broadcast_to(vg, V.shape), np.ones_like(V)]).astype(in_dt)
            goall = np.concatenate([go] * 3).astype(in_dt)
            ref_all = mlpg_grad64(Vall, goall, windows, np.tile(lens7, 3))
            for mi, mode in enumerate(MODES):
                ref = ref_all[7 * mi:7 * mi + 7]
                for lk, sl in (("none", slice(0, 2)), ("ragged", slice(2, 7))):
                    has_l = lk == "ragged"
                    var = {"frame": V[sl].astype(in_dt), "global": vg.astype(in_dt), "unit": None}[mode]
                    v, g = _to_dev(var), _to_dev(go[sl].astype(in_dt))
                    L = _to_dev(rag) if has_l else None
                    lens = lens7[sl]
                    for in_, out_dt in DT_PAIRS:
                        if in_ != in_dt:
                            continue
                        tol = 1e-10 if (in_dt == np.float64 and out_dt == np.float64) else 3e-6
                        for fam in list(FAMILIES) + ["auto"]:
                            took, out = _run_cell(fam, v, g, windows, D, L, in_dt, out_dt, mode, T, has_l)
                            if out is None:
                                continue
                            _check_grad(out, ref[sl], lens, tol,
                                        (wname, T, sd, in_dt.__name__, out_dt.__name__, mode, lk, fam, took))


# AUTO cells that reach each family (the preference rules of capi.hip route_of and csrc/mlpg_*.hip *_preferred)
AUTO_CELLS = [
    # family, windows, mode, in, out, B, T, sd, lengths
    ("const", "std3", "global", np.float64, np.float64, 192, 100, 40, True),      # const_preferred: >= 192 (utt, group) of >= 32 dims
    ("strip", "std3", "frame", np.float64, np.float32, 2, 1100, 16, True),        # strip_preferred: sd >= 16, T > 1024
    ("strip", "std3", "frame", np.float32, np.float32, 32, 1000, 64, False),      # full lane groups, >= 512 items
    ("chunk", "wide3", "frame", np.float64, np.float64, 4, 64, 16, True),         # chunk_preferred: B*sd >= 64, T >= 64, extent 2
    ("fir", "std3", "unit", np.float32, np.float32, 3, 96, 5, False),             # float32, unit, no lengths, T >= 96
    ("wave", "std3", "frame", np.float64, np.float64, 3, 200, 5, True),
    ("generic", "wide3", "frame", np.float32, np.float32, 3, 50, 5, True),
]


def test_auto_reaches_every_family():
    """AUTO's own cells: each lands on the family its preference rule names and matches the reference."""
    reached = set()
    for fam, wname, mode, in_dt, out_dt, B, T, sd, has_l in AUTO_CELLS:
        windows = WINDOW_SETS[wname]
        _warm_fir(windows)
        D = len(windows) * sd
        rng = np.random.RandomState(B + T + sd)
        V = (rng.rand(B, T, D) + 0.1).astype(in_dt)
        var = {"frame": V, "global": V[0, 0].copy(), "unit": None}[mode]
        go = rng.randn(B, T, sd).astype(in_dt)
        lens = rng.randint(1, T + 1, size=B).astype(np.int32) if has_l else np.full(B, T, dtype=np.int32)
        if has_l:
            lens[:2] = (T, 0) if B > 2 else (T, 1)
        took, out = _run_cell("auto", _to_dev(var), _to_dev(go), windows, D, _to_dev(lens) if has_l else None,
                              in_dt, out_dt, mode, T, has_l)
        assert took == fam, (fam, took)
        tol = 1e-10 if (in_dt == np.float64 and out_dt == np.float64) else 3e-6
        _check_grad(out, mlpg_grad64(var, go, windows, lens), lens, tol, (fam, wname, mode))
        reached.add(took)
    assert reached == set(FAMILIES), reached


# ---------------------------------------------------------------------------------------------------- padding contract

def _dirty(V, M, go, lens):
    """Copies with NaN / 0 / -1 in the per-frame variances' padding, NaN in the means' and grad_out's padding."""
    Vd, Md, god = V.copy(), M.copy(), go.copy()
    junk = np.array([np.nan, 0.0, -1.0], dtype=V.dtype)
    for b, L in enumerate(lens):
        n = V.shape[1] - L
        Vd[b, L:] = junk[np.arange(n) % 3][:, None]
        Md[b, L:] = np.nan
        god[b, L:] = np.nan
    return Vd, Md, god


@pytest.mark.parametrize("wname", ["std3", "wide3", "asym2"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_padding_contract_both_directions(wname, dt):
    """The same live data with clean (zero) and dirty padding: live rows bit-identical, padding rows exactly 0, statuses equal,
    on every route that takes a lengths vector, forward and backward."""
    import torch
    from nnmnkwii_amd import _hip
    windows = WINDOW_SETS[wname]
    nw = len(windows)
    for B, T, sd in ((5, 200, 5), (5, 200, 70), (16, 130, 5)):
        D = nw * sd
        rng = np.random.RandomState(B * T + sd + nw)
        lens = np.concatenate([_ragged(T), rng.randint(0, T + 1, size=B - 5)]).astype(np.int32)
        live = np.arange(T)[None, :] < lens[:, None]
        V = ((rng.rand(B, T, D) + 0.1) * live[:, :, None]).astype(dt)
        M = (rng.randn(B, T, D) * live[:, :, None]).astype(dt)
        go = (rng.randn(B, T, sd) * live[:, :, None]).astype(dt)
        Vd, Md, god = _dirty(V, M, go, lens)
        L = _to_dev(lens)
        for mode in MODES:
            for fam in ("generic", "wave", "strip", "const", "chunk", "auto"):
                algo = 0 if fam == "auto" else FAMILIES[fam][0]
                if fam != "auto" and not supported(fam, windows, mode, dt, dt, T, True):
                    continue
                res = []
                for Vx, Mx, gx in ((V, M, go), (Vd, Md, god)):
                    var = {"frame": _to_dev(Vx), "global": _to_dev(V[0, 0].copy()), "unit": None}[mode]
                    y, sy = _hip.forward(_to_dev(Mx), var, windows, L, algo=algo)
                    gr, sg = _hip.backward(var, _to_dev(gx), windows, D, L, out_dtype=_torch_dt(dt), algo=algo)
                    torch.cuda.synchronize()
                    res.append((y.cpu().numpy(), sy.cpu().numpy(), gr.cpu().numpy(), sg.cpu().numpy()))
                (y0, sy0, g0, sg0), (y1, sy1, g1, sg1) = res
                what = (wname, dt.__name__, B, T, sd, mode, fam)
                assert np.array_equal(sy0, sy1) and np.array_equal(sg0, sg1) and not sy0.any() and not sg0.any(), what
                for a0, a1 in ((y0, y1), (g0, g1)):
                    assert not a0[~live].any() and not a1[~live].any(), what + ("padding",)
                    assert np.array_equal(a0[live], a1[live]), what + ("live rows differ",)
                if mode == "frame":
                    _check_grad(g1, mlpg_grad64(V, go, windows, lens), lens, 1e-10 if dt == np.float64 else 3e-6, what)


# ---------------------------------------------------------------------------------------------------- user-facing callers

def test_autograd_mlpg_float64_cuda_gradient():
    """autograd.mlpg on float64 CUDA tensors takes the float64 -> float32 route: a config-2 utterance (std3) and a wide3 one
    (the natural-order kernel)."""
    import torch
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd import autograd as AF
    for wname, T, sd in (("std3", 1000, 60), ("wide3", 300, 7)):
        windows = WINDOW_SETS[wname]
        D = len(windows) * sd
        rng = np.random.RandomState(T + sd)
        m = torch.from_numpy(rng.randn(T, D)).cuda().requires_grad_()
        v_np = rng.rand(T, D) + 0.1
        G_np = rng.randn(T, sd)
        c0 = _counts()
        y = AF.mlpg(m, torch.from_numpy(v_np).cuda(), windows)
        (y * torch.from_numpy(G_np).cuda().to(y.dtype)).sum().backward()
        c1 = _counts()
        ref = mlpg_grad64(v_np[None], G_np.astype(np.float32)[None], windows)[0]
        g = m.grad.cpu().numpy()
        assert np.abs(g - ref).max() <= 3e-6 * np.abs(ref).max(), (wname, np.abs(g - ref).max() / np.abs(ref).max())
        if wname == "wide3":
            assert c1[0] - c0[0] >= 1          # the natural-order kernel took a pass


def test_autograd_unit_variance_mlpg_backward():
    import torch
    from nnmnkwii_amd import autograd as AF
    from nnmnkwii_amd import paramgen as G
    for wname, B, T, sd in (("std3", 3, 120, 6), ("std2", 2, 40, 3)):
        windows = WINDOW_SETS[wname]
        D = len(windows) * sd
        R = torch.from_numpy(G.unit_variance_mlpg_matrix(windows, T)).cuda()
        rng = np.random.RandomState(B * T)
        means = torch.from_numpy(rng.rand(B, T, D).astype(np.float32)).cuda().requires_grad_()
        go = rng.randn(B, T, sd).astype(np.float32)
        y = AF.unit_variance_mlpg(R, means)
        (y * torch.from_numpy(go).cuda()).sum().backward()
        ref = mlpg_grad64(None, go, windows)
        g = means.grad.cpu().numpy()
        for b in range(B):
            assert np.abs(g[b] - ref[b]).max() <= 3e-6 * np.abs(ref[b]).max(), (wname, b)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_paramgen_mlpg_grad_global_variances(dt):
    """paramgen.mlpg_grad on numpy (mlpg_hip_backward_host) with global (D,) variances."""
    from nnmnkwii_amd import paramgen as G
    windows = WINDOW_SETS["std3"]
    T, sd = 500, 4
    rng = np.random.RandomState(9)
    vg = (rng.rand(3 * sd) + 0.1).astype(dt)
    go = rng.randn(T, sd).astype(dt)
    g = G.mlpg_grad(np.zeros((T, 3 * sd), dtype=dt), vg, windows, go)
    ref = mlpg_grad64(vg, go[None], windows)[0]
    assert g.dtype == np.float32
    assert np.abs(g - ref).max() <= 3e-6 * np.abs(ref).max()
