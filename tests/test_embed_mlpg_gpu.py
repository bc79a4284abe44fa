"""GPU tests (-m gpu): mlpg_hip_forward, mlpg_hip_backward and mlpg_hip_backward_var on pointers that do not come straight from
the allocator.  The kernels choose their staging (16-byte LDS-DMA runs or registers: dma_ok of csrc/mlpg_wave_impl.h) and their
store width (out_pairs_ok) from the shape AND from the pointers; every other test hands them pointers aligned to 256 bytes, so the
pointer clauses never decide.  Here every cell runs with all pointers aligned (the baseline), with each data pointer alone one
element in, with all of them one element in (status and lengths one int32 in), and with all of them at the smallest shift that
restores 16-byte alignment.  Every buffer sits between guard bands (tests/embed.py).

Per call: return code 0, status all zero, the family's launch counter moved (the strip family has two: kinds 2 and 9), guards
intact on every buffer, inputs unchanged, rows at and past each length exactly zero, and the result equal to the baseline's bit
for bit -- staging and store width change no arithmetic.  The baseline meets the reference at the bounds the suite uses for the
entry: oracle.mlpg at 1e-9 / 5e-6 (forward), oracle.grad64 at 1e-10 / 3e-6 (backward), tests/vargrad64.py at 1e-10 / 3e-6
(backward_var).  AUTO runs every family's cells and must land on exactly one family.

Shapes: B = 3, lengths None and [T, T - 1, 0]; per family the smallest that reach its tiers (wave: T 5 / 257 / 1025 with 4, 6 and
5 static dims -- 4 takes the DMA in both dtypes, 6 in float64 only and allows pairs, 5 allows neither)."""
import functools

import numpy as np
import pytest
import torch

import vargrad64
from cases import WINDOW_SETS
from embed import Embedded, embedded, failed, ptr
from oracle import mlpg as O
from oracle.grad64 import mlpg_grad64
from test_backward_routes_gpu import FAMILIES, _check_grad, _warm_fir, supported
from test_strip_gpu import TOL32, TOL64, rel_err
from test_var_grad_gpu import VARGRAD_KIND, _check_var_grad, _masked, _terms

pytestmark = pytest.mark.gpu

B = 3
KINDS = {kind: fam for fam, (_, kind) in FAMILIES.items()}
KINDS[9] = "strip"                    # the strip kernel's transposed form (narrow static dims: the lanes over several utterances)
F32, F64 = np.float32, np.float64
TOL_FWD = {F64: TOL64, F32: TOL32}
MODE_ID = {"frame": 0, "global": 1, "unit": 2}
DT_ID = {F32: 0, F64: 1}

# family -> (window sets, T values, static dims, variance modes, (in, out) dtype pairs, lengths given)
SHAPES = {
    "wave": (("std3",), (5, 257, 1025), (4, 6, 5), ("frame", "global", "unit"), ((F64, F64), (F32, F32), (F64, F32)), (False, True)),
    "strip": (("std3",), (65, 200), (5, 70), ("frame",), ((F64, F64), (F32, F32), (F64, F32)), (False, True)),
    "const": (("std2", "std3"), (65, 300), (5,), ("global", "unit"), ((F64, F64), (F32, F32), (F64, F32)), (False, True)),
    "chunk": (("wide3",), (41, 300), (5,), ("frame",), ((F64, F64), (F32, F32)), (False, True)),
    "fir": (("std3",), (97, 300), (4, 5), ("unit",), ((F32, F32),), (False,)),
    "generic": (("asym2",), (17,), (5,), ("frame",), ((F64, F64), (F32, F32), (F64, F32)), (False, True)),
}
CELLS = [(fam, T) for fam, spec in SHAPES.items() for T in spec[1]]


def _call():
    from nnmnkwii_amd import _hip
    dev = torch.device("cuda", torch.cuda.current_device())
    return _hip.lib(), dev.index, _hip._stream(dev)


def _counts():
    from nnmnkwii_amd import _hip
    L = _hip.lib()
    return {k: L.mlpg_hip_launch_count(k) for k in list(KINDS) + [VARGRAD_KIND]}


def _lens(T, has_l):
    return np.array([T, T - 1, 0], dtype=np.int32) if has_l else None


@functools.lru_cache(maxsize=None)
def _data(wname, T, sd, dt, mode, has_l):
    """(mean, var or None, grad_out, lengths or None, effective lengths) of one cell, in dtype dt."""
    nw = len(WINDOW_SETS[wname])
    D = nw * sd
    rng = np.random.RandomState(1000 * T + 10 * sd + nw)
    M = rng.randn(B, T, D).astype(dt)
    V = (rng.rand(B, T, D) + 0.1).astype(dt)
    vg = (rng.rand(D) + 0.1).astype(dt)
    go = rng.randn(B, T, sd).astype(dt)
    lens = _lens(T, has_l)
    return M, {"frame": V, "global": vg, "unit": None}[mode], go, lens, (np.full(B, T, dtype=np.int32) if lens is None else lens)


def _patterns(names, present, dts):
    """[(label, {buffer name: element offset})]: aligned, each data pointer alone at +1, all at +1 (status and lengths too), all at
    the smallest shift that restores 16-byte alignment (status and lengths still at +1 int32)."""
    data = [n for n in names if present[n]]
    out = [("aligned", {})]
    out += [("%s+1" % n, {n: 1}) for n in data]
    out.append(("all+1", dict({n: 1 for n in data}, status=1, lengths=1)))
    out.append(("all+16 bytes", dict({n: 16 // np.dtype(dts[n]).itemsize for n in data}, status=1, lengths=1)))
    return out


def _moved(c0, fam, what, exactly_one):
    moved = {k: n - c0[k] for k, n in _counts().items() if n != c0[k]}
    moved.pop(VARGRAD_KIND, None)
    assert len(moved) == 1, (what, moved)
    kind, n = next(iter(moved.items()))
    assert n == 1 or (n >= 1 and not exactly_one), (what, moved)
    if fam != "auto":
        assert KINDS[kind] == fam, (what, KINDS[kind])
    return KINDS[kind]


def _settle(ins, outs, what):
    torch.cuda.synchronize()
    bad = failed(ins, outs)
    assert not bad, (what, bad)


def _zero_padding(a, lens, what):
    pad = np.arange(a.shape[1])[None, :] >= np.asarray(lens)[:, None]
    assert not a[pad].any() and not np.isnan(a[pad]).any(), (what, "rows at and past the length are not exactly zero")


def _run_patterns(names, arrays, dts, out_shapes, call, fam, what, lens_eff, exactly_one):
    """Run `call` under every pointer pattern; returns the baseline's outputs as host arrays.  arrays: name -> ndarray or None
    (inputs, "lengths" among them); out_shapes: name -> (shape, dtype) ("status" among them)."""
    present = {n: (arrays[n] is not None if n in arrays else True) for n in names}
    base = None
    for label, offs in _patterns(names, present, dts):
        ins = {n: embedded(a, offs.get(n, 0)) for n, a in arrays.items()}
        outs = {n: Embedded(shape, dt, offs.get(n, 0), 0xA5) for n, (shape, dt) in out_shapes.items()}
        c0 = _counts()
        rc = call(ins, outs)
        assert rc == 0, (what, label, rc)
        _settle(ins, outs, what + (label,))
        _moved(c0, fam, what + (label,), exactly_one)
        got = {n: b.host() for n, b in outs.items()}
        assert not got["status"].any(), (what, label, "status")
        for n, a in got.items():
            if n != "status":
                _zero_padding(a, lens_eff, what + (label, n))
        if base is None:
            base = got
        else:
            for n in got:
                assert got[n].tobytes() == base[n].tobytes(), (what, label, "%s differs from the aligned call" % n)
    return base


def _each(fam, T):
    """The cells of one (family, T): (family whose shapes these are, wname, windows, sd, mode, in_dt, out_dt, has_l)."""
    for shapes_of in (list(SHAPES) if fam == "auto" else [fam]):
        wnames, Ts, sds, modes, pairs, lens_opts = SHAPES[shapes_of]
        if T not in Ts:
            continue
        for wname in wnames:
            windows = WINDOW_SETS[wname]
            _warm_fir(windows)
            for sd in sds:
                for mode in modes:
                    for in_dt, out_dt in pairs:
                        for has_l in lens_opts:
                            if fam != "auto":
                                assert supported(fam, windows, mode, in_dt, out_dt, T, has_l)
                            yield shapes_of, wname, windows, sd, mode, in_dt, out_dt, has_l


AUTO_CELLS = [("auto", T) for T in sorted({T for spec in SHAPES.values() for T in spec[1]})]


@pytest.mark.parametrize("fam,T", CELLS + AUTO_CELLS)
def test_forward_under_pointer_offsets(fam, T):
    from nnmnkwii_amd import _hip
    L, dev, stream = _call()
    algo = 0 if fam == "auto" else FAMILIES[fam][0]
    for _, wname, windows, sd, mode, in_dt, out_dt, has_l in _each(fam, T):
        if in_dt != out_dt:
            continue                                               # one dtype in the forward call
        nw, pl, pu, pc, _keep = _hip._win_args(windows)
        D = nw * sd
        M, var, _, lens, lens_eff = _data(wname, T, sd, in_dt, mode, has_l)
        what = ("forward", fam, wname, T, sd, mode, in_dt.__name__, has_l)

        def call(ins, outs):
            return L.mlpg_hip_forward(dev, stream, DT_ID[in_dt], algo, ins["mean"].ptr(), ptr(ins["var"]), MODE_ID[mode],
                                      ptr(ins["lengths"]), B, T, D, nw, pl, pu, pc, outs["out"].ptr(), outs["status"].ptr())
        base = _run_patterns(("mean", "var", "out"), dict(mean=M, var=var, lengths=lens), dict(mean=in_dt, var=in_dt, out=in_dt),
                             dict(out=((B, T, sd), in_dt), status=((B * sd,), np.int32)), call, fam, what, lens_eff, False)
        ref = _forward_ref(wname, T, sd, in_dt, mode, has_l)
        e = rel_err(base["out"].reshape(-1, sd), ref.reshape(-1, sd))
        assert e <= TOL_FWD[in_dt], (what, e)


@functools.lru_cache(maxsize=None)
def _forward_ref(wname, T, sd, dt, mode, has_l):
    windows = WINDOW_SETS[wname]
    M, var, _, lens, lens_eff = _data(wname, T, sd, dt, mode, has_l)
    v = np.ones(M.shape[2], dtype=dt) if var is None else var
    yo, _, rc = O.mlpg_batch(M, v, windows, np.maximum(lens_eff, 1).astype(np.int32))
    assert rc == 0
    yo[lens_eff == 0] = 0                                          # an empty utterance: all rows are padding
    return yo


@functools.lru_cache(maxsize=None)
def _backward_ref(wname, T, sd, dt, mode, has_l):
    _, var, go, _, lens_eff = _data(wname, T, sd, dt, mode, has_l)
    return mlpg_grad64(var, go, WINDOW_SETS[wname], lens_eff)


@pytest.mark.parametrize("fam,T", CELLS + AUTO_CELLS)
def test_backward_under_pointer_offsets(fam, T):
    from nnmnkwii_amd import _hip
    L, dev, stream = _call()
    algo = 0 if fam == "auto" else FAMILIES[fam][0]
    for _, wname, windows, sd, mode, in_dt, out_dt, has_l in _each(fam, T):
        nw, pl, pu, pc, _keep = _hip._win_args(windows)
        D = nw * sd
        _, var, go, lens, lens_eff = _data(wname, T, sd, in_dt, mode, has_l)
        what = ("backward", fam, wname, T, sd, mode, in_dt.__name__, out_dt.__name__, has_l)

        def call(ins, outs):
            return L.mlpg_hip_backward(dev, stream, DT_ID[in_dt], DT_ID[out_dt], algo, ptr(ins["var"]), MODE_ID[mode],
                                       ins["grad_out"].ptr(), ptr(ins["lengths"]), B, T, D, nw, pl, pu, pc,
                                       outs["grad_mean"].ptr(), outs["status"].ptr())
        base = _run_patterns(("var", "grad_out", "grad_mean"), dict(var=var, grad_out=go, lengths=lens),
                             dict(var=in_dt, grad_out=in_dt, grad_mean=out_dt),
                             dict(grad_mean=((B, T, D), out_dt), status=((B * sd,), np.int32)), call, fam, what, lens_eff, True)
        tol = 1e-10 if (in_dt == F64 and out_dt == F64) else 3e-6
        _check_grad(base["grad_mean"], _backward_ref(wname, T, sd, in_dt, mode, has_l), lens_eff, tol, what)


@functools.lru_cache(maxsize=None)
def _var_ref(wname, T, sd, dt, mode, has_l):
    windows = WINDOW_SETS[wname]
    M, var, go, _, lens_eff = _data(wname, T, sd, dt, mode, has_l)
    V = var if mode == "frame" else np.ascontiguousarray(np.broadcast_to(var, M.shape))     # per-frame contributions
    y, gm, gv = vargrad64.mlpg_var_grad64(M, V, go, windows, lens_eff)
    return gm, gv, _terms(M, V, y, gm, windows), _masked(windows, lens_eff, T, sd)


@pytest.mark.parametrize("fam,T", [c for c in CELLS if c[0] != "fir"] + AUTO_CELLS)
def test_backward_var_under_pointer_offsets(fam, T):
    from nnmnkwii_amd import _hip
    L, dev, stream = _call()
    algo = 0 if fam == "auto" else FAMILIES[fam][0]
    for shapes_of, wname, windows, sd, mode, in_dt, out_dt, has_l in _each(fam, T):
        if in_dt != out_dt or mode == "unit":
            continue                                               # one dtype; unit variances have nothing to differentiate
        nw, pl, pu, pc, _keep = _hip._win_args(windows)
        D = nw * sd
        M, var, go, lens, lens_eff = _data(wname, T, sd, in_dt, mode, has_l)
        dev_t = lambda a: None if a is None else torch.from_numpy(a).cuda()
        y = _hip.forward(dev_t(M), dev_t(var), windows, dev_t(lens))[0].cpu().numpy()
        what = ("backward_var", fam, wname, T, sd, mode, in_dt.__name__, has_l)

        def call(ins, outs):
            c13 = L.mlpg_hip_launch_count(VARGRAD_KIND)
            rc = L.mlpg_hip_backward_var(dev, stream, DT_ID[in_dt], algo, ins["mean"].ptr(), ins["var"].ptr(), MODE_ID[mode],
                                         ins["y"].ptr(), ins["grad_out"].ptr(), ptr(ins["lengths"]), B, T, D, nw, pl, pu, pc,
                                         outs["grad_mean"].ptr(), outs["grad_var"].ptr(), outs["status"].ptr())
            assert L.mlpg_hip_launch_count(VARGRAD_KIND) == c13 + 1, what
            return rc
        names = ("mean", "var", "y", "grad_out", "grad_mean", "grad_var")
        base = _run_patterns(names, dict(mean=M, var=var, y=y, grad_out=go, lengths=lens), {n: in_dt for n in names},
                             dict(grad_mean=((B, T, D), in_dt), grad_var=((B, T, D), in_dt), status=((B * sd,), np.int32)),
                             call, fam, what, lens_eff, True)
        tol = 1e-10 if in_dt == F64 else 3e-6
        gm_r, gv_r, terms, masked = _var_ref(wname, T, sd, in_dt, mode, has_l)
        _check_var_grad(base["grad_var"], gv_r, lens_eff, masked, tol, what, terms)
        err = np.abs(base["grad_mean"].astype(np.float64) - gm_r).max()
        assert err <= tol * max(np.abs(gm_r).max(), 1e-300), what + ("grad_mean", err)
