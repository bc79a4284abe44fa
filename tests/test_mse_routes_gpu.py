"""GPU tests (-m gpu): every route of mlpg_hip_unit_mse_step, the fused unit-variance MLPG + MSE training step, against
oracle/mse64.py (float64, no library code; tests/test_mse64_cpu.py pins it to the dense definition).

The step has two forms (include/mlpg_hip.h): the one-launch kernel (csrc/mlpg_wave_fused.hip: extents <= 1, Tmax <= 1024,
both dtypes, ragged lengths; the last workgroup sums the loss partials in the caller's workspace) and the FIR form
(csrc/mlpg_fir.hip launch_fir_mse: float32, no lengths, Tmax >= 96, 1-3 windows of extent <= 2 whose first is a single
non-zero tap, a window set that passes the decay test, and the larger workspace of mlpg_hip_unit_mse_workspace_bytes_t).
The test calls the C ABI itself with workspaces it owns, so that IT decides which form is allowed: each problem runs once
with the small workspace and once with the larger one.  Every cell predicts its form from the documented conditions,
asks mlpg_hip_unit_mse_form the same, and checks the launch counters, the return code, y / grad / loss / status against
the reference, exact zeros at and past each length, canary bytes after every output and the workspace, bitwise repeatable
results and NaN padding that changes nothing.  Refused cells must touch nothing."""
import time

import numpy as np
import pytest

from cases import WINDOW_SETS
from oracle.mlpg import pack_windows
from oracle.mse64 import unit_mse_step64

pytestmark = pytest.mark.gpu

EINVAL = -1
F32, F64 = 0, 1
NP_DT = {F32: np.float32, F64: np.float64}
K_FUSED, K_FIR = 5, 7                         # mlpg_hip_launch_count kinds of the two forms
NKINDS = 12

SETS = {name: WINDOW_SETS[name] for name in ("static", "std2", "std3", "asym2", "zero2", "wide3")}
SETS["fwd2"] = [(0, 0, np.array([1.0])), (0, 1, np.array([-1.0, 1.0]))]
SETS["std3-s2"] = [(0, 0, np.array([2.0]))] + WINDOW_SETS["std3"][1:]
# P^-1 does not decay to 2^-26 within 24 frames: the FIR form's table test refuses it
SETS["dynamic-x4"] = [(0, 0, np.array([1.0])), (1, 1, 4.0 * np.array([-0.5, 0.0, 0.5])), (1, 1, 4.0 * np.array([1.0, -2.0, 1.0]))]
FIR_DECAYS = {"static", "std2", "std3", "asym2", "zero2", "wide3", "fwd2", "std3-s2"}

TMAX = [1, 2, 3, 5, 17, 63, 64, 65, 95, 96, 97, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2049]
SDS = [1, 3, 4, 5, 8, 63, 64, 65, 70]
BS = [1, 3, 8, 9, 64]
# (dtype, lengths) by cell: a third of the cells can take the FIR form
CYCLE = [(F32, "null"), (F64, "ragged"), (F32, "ragged"), (F64, "null"), (F32, "null"), (F64, "full")]
CANARY = 256                                  # bytes after every output and the workspace
# (y, grad, loss) relative tolerances; y and grad per utterance against its largest reference value
TOL = {(F64, 1): (1e-10, 1e-10, 1e-11), (F32, 1): (3e-6, 3e-6, 1e-6), (F32, 2): (5e-6, 2e-5, 2e-5)}
TOL_FIR_OWN_Y = 1e-6                          # FIR loss against the loss recomputed from the kernel's own y

STATS = {"accepted": 0, "refused": 0, "fir": 0, "fused": 0}


def _lib():
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts():
    L = _lib()
    return [L.mlpg_hip_launch_count(k) for k in range(NKINDS)]


def _moved(c0):
    c1 = _counts()
    return {k: c1[k] - c0[k] for k in range(NKINDS) if c1[k] != c0[k]}


def _ext(windows):
    return max(max(l, u) for l, u, _ in windows)


def predict(name, windows, dt, has_lengths, fir_ws, Tmax):
    """2 the FIR form, 1 the one-launch kernel, 0 refused: the conditions of include/mlpg_hip.h, restated."""
    l0, u0, c0 = windows[0]
    if (dt == F32 and not has_lengths and fir_ws and Tmax >= 96 and 1 <= len(windows) <= 3 and _ext(windows) <= 2
            and l0 == 0 and u0 == 0 and float(np.asarray(c0).ravel()[0]) != 0.0 and name in FIR_DECAYS):
        return 2
    return 1 if _ext(windows) <= 1 and 1 <= Tmax <= 1024 else 0


class Buf:
    """n elements of dt at element offset `off` of a device byte buffer filled with `fill`, CANARY bytes behind them."""

    def __init__(self, n, dt, off, fill):
        import torch
        esz = np.dtype(dt).itemsize
        self.lo, self.hi, self.fill = off * esz, (off + n) * esz, fill
        self.raw = torch.full((self.hi + CANARY,), fill, dtype=torch.uint8, device="cuda")
        tdt = {np.float32: torch.float32, np.float64: torch.float64, np.int32: torch.int32}[np.dtype(dt).type]
        self.view = self.raw[self.lo:self.hi].view(tdt)

    def ptr(self):
        return self.view.data_ptr()

    def put(self, a):
        import torch
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()))

    def reset(self):
        self.raw[self.lo:self.hi] = self.fill

    def host(self):
        return self.view.cpu().numpy()

    def untouched(self):
        return bool((self.raw.cpu().numpy() == self.fill).all())

    def canary_ok(self):
        r = self.raw.cpu().numpy()
        return bool((r[:self.lo] == self.fill).all() and (r[self.hi:] == self.fill).all())


def _workspace(nbytes):
    """Exactly nbytes, zeroed once, 0xA5 canary behind them."""
    import torch
    ws = torch.zeros(nbytes + CANARY, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0xA5
    assert ws.data_ptr() % 128 == 0
    return ws


def _ws_ok(ws, nbytes):
    h = ws.cpu().numpy()
    return bool((h[nbytes:] == 0xA5).all() and not h[:4].any())     # canary kept, arrival counter left at 0


def _win(windows):
    wl, wu, wc = pack_windows(windows)
    return len(windows), wl, wu, wc


def _form_query(dt, has_lengths, B, Tmax, D, win):
    import torch
    nw, wl, wu, wc = win
    return _lib().mlpg_hip_unit_mse_form(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, dt,
                                         1 if has_lengths else 0, B, Tmax, D, nw, wl.ctypes.data, wu.ctypes.data, wc.ctypes.data)


def _step(dt, mean, target, lens, B, Tmax, D, win, n_elems, y, grad, loss, status, ws, ws_bytes, stream=None):
    import torch
    nw, wl, wu, wc = win
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    return _lib().mlpg_hip_unit_mse_step(torch.cuda.current_device(), stream, dt, mean, target, lens, B, Tmax, D, nw,
                                         wl.ctypes.data, wu.ctypes.data, wc.ctypes.data, float(n_elems), y, grad, loss, status,
                                         ws, ws_bytes)


def _p(b):
    return None if b is None else b.ptr()


@pytest.fixture(scope="module", autouse=True)
def _warm_fir_tables():
    """The first query for a window set builds its FIR tap table with one natural-order solve (counter 0): do it before any
    cell counts launches."""
    import torch
    for windows in SETS.values():
        nw = len(windows)
        _form_query(F32, False, 1, 96, nw, _win(windows))
    torch.cuda.synchronize()
    yield
    print("\n[mse routes] cells: %s" % STATS)


# ----------------------------------------------------------------------------------------------------------------- cells

def _ragged(B, Tmax, mw, rng):
    base = [Tmax, 0, 1, 2, 2 * mw, 2 * mw + 1]
    L = [min(x, Tmax) for x in base] + list(rng.randint(0, Tmax + 1, size=B - len(base)))
    return np.array(L[:B], dtype=np.int32)


def _problem(name, Tmax, k, dt=None, lmode=None, sd=None, B=None):
    """The k-th cell of the deterministic rotation over dtype, lengths, sd, B, NULL outputs, n_elems and pointer offsets."""
    windows = SETS[name]
    nw = len(windows)
    mw = _ext(windows)
    cyc_dt, cyc_l = CYCLE[k % len(CYCLE)]
    dt = cyc_dt if dt is None else dt
    lmode = cyc_l if lmode is None else lmode
    sd = SDS[(k * 5 + 1) % len(SDS)] if sd is None else sd
    if B is None:
        B = BS[(k * 3) % len(BS)]
        if lmode == "ragged" and B < 8:
            B = 8 + (k % 2)
        while B * Tmax * sd * (nw + 1) > 3_000_000 and B > (8 if lmode == "ragged" else 1):
            B = max(b for b in BS if b < B)
    rng = np.random.RandomState(k * 131 + Tmax)
    lengths = None
    if lmode == "full":
        lengths = np.full(B, Tmax, dtype=np.int32)
    elif lmode == "ragged":
        lengths = _ragged(B, Tmax, mw, rng)
    m = rng.randn(B, Tmax, nw * sd).astype(NP_DT[dt])
    tg = rng.randn(B, Tmax, sd).astype(NP_DT[dt])
    if lengths is not None:
        pad = np.arange(Tmax)[None, :] >= lengths[:, None]
        m[pad] = 0
        tg[pad] = 0
    live = B * Tmax if lengths is None else int(lengths.sum())
    ne = {"default": float(B * Tmax * sd), "live": float(max(live, 1) * sd), "arbitrary": 1234.5}[("default", "live", "arbitrary")[(k // 4) % 3]]
    y_given, st_given = [(1, 1), (0, 1), (1, 0), (0, 0)][(k // 3) % 4]
    off = (k // 6) % 2
    return dict(name=name, windows=windows, dt=dt, B=B, Tmax=Tmax, sd=sd, D=nw * sd, lengths=lengths, m=m, tg=tg,
                n_elems=ne, y_given=y_given, st_given=st_given, off=off)


class Run:
    """The buffers of one call of a problem: inputs at element offset P['off'] with NaN around them, outputs filled with
    sentinels (0xFF bytes: NaN; status 0x5A5A5A5A), the loss slot NaN."""

    def __init__(self, P, ws_bytes, ws=None):
        import torch
        dt = NP_DT[P["dt"]]
        B, Tmax, sd, D, off = P["B"], P["Tmax"], P["sd"], P["D"], P["off"]
        self.P, self.ws_bytes = P, ws_bytes
        self.mean = Buf(B * Tmax * D, dt, off, 0xFF)
        self.mean.put(P["m"])
        self.target = Buf(B * Tmax * sd, dt, off, 0xFF)
        self.target.put(P["tg"])
        self.lens = None if P["lengths"] is None else torch.from_numpy(P["lengths"]).cuda()
        self.y = Buf(B * Tmax * sd, dt, off, 0xFF) if P["y_given"] else None
        self.grad = Buf(B * Tmax * D, dt, off, 0xFF)
        self.status = Buf(B * sd, np.int32, off, 0x5A) if P["st_given"] else None
        self.loss = Buf(1, np.float64, off, 0xFF)
        self.ws = _workspace(ws_bytes) if ws is None else ws

    def outputs(self):
        return [b for b in (self.y, self.grad, self.status, self.loss) if b is not None]

    def reset(self):
        for b in self.outputs():
            b.reset()

    def call(self, **kw):
        P = self.P
        a = dict(dt=P["dt"], mean=self.mean.ptr(), target=self.target.ptr(),
                 lens=None if self.lens is None else self.lens.data_ptr(), B=P["B"], Tmax=P["Tmax"], D=P["D"],
                 win=_win(P["windows"]), n_elems=P["n_elems"], y=_p(self.y), grad=self.grad.ptr(), loss=self.loss.ptr(),
                 status=_p(self.status), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes)
        a.update(kw)
        return _step(**a)

    def snapshot(self):
        return [None if b is None else b.host().copy() for b in (self.y, self.grad, self.status, self.loss)]


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _diff(got, want):
    """Which of (y, grad, status, loss) differ, and by how much (for the failure message)."""
    out = []
    for name, a, b in zip(("y", "grad", "status", "loss"), got, want):
        if not _same_bits(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            out.append((name, int((a.view(np.uint8) != b.view(np.uint8)).sum()), float(np.nanmax(d)) if d.size else None,
                        int(np.nanargmax(d)) if d.size else None))
    return out


def _check_rows(got, ref, lengths, ok, tol, what):
    """Per utterance: |got - ref| <= tol * max|ref|; rows at and past each length, and the columns of failed systems,
    exactly 0."""
    got = got.astype(np.float64)
    B, T, C = got.shape
    pad = np.arange(T)[None, :] >= lengths[:, None]
    assert not got[pad].any(), (what, "padding rows not zero")
    bad = np.tile(~ok, (1, C // ok.shape[1]))
    assert not got[np.broadcast_to(bad[:, None, :], got.shape)].any(), (what, "columns of a failed system not zero")
    err = np.abs(got - ref).max(axis=(1, 2))
    scale = np.abs(ref).max(axis=(1, 2))
    rel = err / np.where(scale > 0, scale, 1.0)
    assert (rel <= tol).all(), (what, float(rel.max()), int(rel.argmax()))


def _run_accepted(P, ref, form, ws_bytes, what):
    import torch
    y_ref, loss_ref, grad_ref, st_ref = ref
    B, Tmax, sd = P["B"], P["Tmax"], P["sd"]
    lengths = P["lengths"] if P["lengths"] is not None else np.full(B, Tmax, dtype=np.int32)
    ok = st_ref == 0
    r = Run(P, ws_bytes)
    c0 = _counts()
    rc = r.call()
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    moved = _moved(c0)
    assert moved == ({K_FIR: 2} if form == 2 else {K_FUSED: 1}), (what, moved)
    tol_y, tol_g, tol_l = TOL[(P["dt"], form)]
    first = r.snapshot()
    y, grad, st, loss = first
    loss = float(loss[0])
    if st is not None:
        assert np.array_equal(st, st_ref.ravel()), (what, "status")
    if y is not None:
        assert y.dtype == NP_DT[P["dt"]]
        _check_rows(y.reshape(B, Tmax, sd), y_ref, lengths, ok, tol_y, what + " y")
    _check_rows(grad.reshape(B, Tmax, P["D"]), grad_ref, lengths, ok, tol_g, what + " grad")
    assert abs(loss - loss_ref) <= tol_l * loss_ref, (what, "loss", loss, loss_ref)
    if form == 2 and y is not None:
        own = float(((y.reshape(P["tg"].shape).astype(np.float64) - P["tg"].astype(np.float64)) ** 2).sum() / P["n_elems"])
        assert abs(loss - own) <= TOL_FIR_OWN_Y * own, (what, "loss vs own y", loss, own)
    for b in r.outputs():
        assert b.canary_ok(), (what, "canary")
    assert _ws_ok(r.ws, ws_bytes), (what, "workspace canary / counter")
    # the same call again (loss slot back to its sentinel): bitwise the same
    r.loss.reset()
    r.grad.reset()
    assert r.call() == 0
    second = r.snapshot()
    assert _same_bits(second[3], first[3]) and _same_bits(second[1], first[1]), (what, "not repeatable", _diff(second, first))
    # NaN in the padding rows of means and target: every output bitwise the same
    if P["lengths"] is not None and (P["lengths"] < Tmax).any():
        pad = np.arange(Tmax)[None, :] >= P["lengths"][:, None]
        m, tg = P["m"].copy(), P["tg"].copy()
        m[pad] = np.nan
        tg[pad] = np.nan
        r.mean.put(m)
        r.target.put(tg)
        r.reset()
        assert r.call() == 0
        third = r.snapshot()
        assert all(_same_bits(a, b) for a, b in zip(third, first)), (what, "NaN padding changed an output", _diff(third, first))
    torch.cuda.synchronize()
    STATS["accepted"] += 1
    STATS["fir" if form == 2 else "fused"] += 1


def _run_refused(P, ws_bytes, what, **kw):
    import torch
    r = Run(P, ws_bytes)
    c0 = _counts()
    rc = r.call(**kw)
    torch.cuda.synchronize()
    assert rc == EINVAL, (what, rc)
    assert _moved(c0) == {}, (what, "a refused call launched")
    for b in r.outputs():
        assert b.untouched(), (what, "a refused call wrote")
    h = r.ws.cpu().numpy()
    assert not h[:ws_bytes].any() and (h[ws_bytes:] == 0xA5).all(), (what, "a refused call touched the workspace")
    STATS["refused"] += 1


def _sizes(P):
    L = _lib()
    nw = len(P["windows"])
    return {"small": int(L.mlpg_hip_unit_mse_workspace_bytes(P["B"], P["D"], nw)),
            "t": int(L.mlpg_hip_unit_mse_workspace_bytes_t(P["B"], P["Tmax"], P["D"], nw))}


def _run_problem(P, tag):
    has_l = P["lengths"] is not None
    form_t = predict(P["name"], P["windows"], P["dt"], has_l, True, P["Tmax"])
    assert _form_query(P["dt"], has_l, P["B"], P["Tmax"], P["D"], _win(P["windows"])) == form_t, (tag, "mlpg_hip_unit_mse_form")
    ref = None
    forms = []
    for kind, nbytes in _sizes(P).items():
        form = predict(P["name"], P["windows"], P["dt"], has_l, kind == "t", P["Tmax"])
        what = "%s ws=%s form=%d" % (tag, kind, form)
        if form == 0:
            _run_refused(P, nbytes, what)
            continue
        if ref is None:
            ref = unit_mse_step64(P["m"], P["tg"], P["windows"], P["lengths"], P["n_elems"])
        _run_accepted(P, ref, form, nbytes, what)
        forms.append(form)
    return forms


def _tag(P):
    return "%s dt=%s B=%d T=%d sd=%d len=%s y=%d st=%d n=%g off=%d" % (
        P["name"], "f32" if P["dt"] == F32 else "f64", P["B"], P["Tmax"], P["sd"],
        "null" if P["lengths"] is None else ("full" if (P["lengths"] == P["Tmax"]).all() else "ragged"),
        P["y_given"], P["st_given"], P["n_elems"], P["off"])


@pytest.mark.parametrize("name", list(SETS))
def test_route_matrix(name):
    t0 = time.time()
    i = list(SETS).index(name)
    seen = set()
    for phase in (0, 3):                     # a phase per set and pass: every Tmax meets every dtype / lengths mode
        for j, Tmax in enumerate(TMAX):
            P = _problem(name, Tmax, i * (len(TMAX) + 1) + j + phase)
            seen.update(_run_problem(P, _tag(P)))
    # every set reaches the one-launch kernel; the sets that decay reach the FIR form too
    assert (1 in seen) == (_ext(SETS[name]) <= 1) and (2 in seen) == (name in FIR_DECAYS), (name, seen)
    print("\n[mse routes] %s: %s, %.1f s" % (name, STATS, time.time() - t0))


@pytest.mark.parametrize("name,Tmax,sd,B,dt,lmode", [
    ("std3", 97, 70, 64, F64, "ragged"),     # 8 x 8 x 18 = 1152 one-launch workgroups feed the final sum
    ("std2", 65, 70, 64, F32, "null"),
    ("std3", 300, 70, 64, F32, "null"),      # the FIR form with two 35-dim groups per utterance
    ("asym2", 1024, 9, 9, F64, "ragged"),
    ("std3", 257, 64, 9, F32, "full"),
    ("wide3", 2049, 65, 3, F32, "null"),
    ("fwd2", 513, 4, 64, F32, "ragged"),
])
def test_route_boundary_cells(name, Tmax, sd, B, dt, lmode):
    for k in range(2):                       # both pointer offsets, NULL outputs and n_elems variants
        P = _problem(name, Tmax, 6 * k + 3, dt=dt, lmode=lmode, sd=sd, B=B)
        _run_problem(P, _tag(P))


@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("windows,lengths", [
    ([(0, 0, [0.0]), (1, 1, [-0.5, 0.0, 0.5])], [0, 1, 2, 2, 1, 0, 2, 1, 2]),
    ([(0, 0, [0.0])], [0, 1, 7, 40, 3, 2, 1, 40, 9]),
])
def test_failing_pivots_in_the_one_launch_form(windows, lengths, dt):
    """A static coefficient of 0: the first pivot is exactly 0 wherever every dynamic row is masked.  status = 1 (the
    oracle's verdict), the system's y and grad columns 0 and no loss term (csrc/mlpg_wave_fused.hip)."""
    lengths = np.asarray(lengths, dtype=np.int32)
    B, Tmax, sd = len(lengths), int(lengths.max()), 5
    nw = len(windows)
    rng = np.random.RandomState(int(lengths.sum()) + dt)
    m = rng.randn(B, Tmax, nw * sd).astype(NP_DT[dt])
    tg = rng.randn(B, Tmax, sd).astype(NP_DT[dt])
    pad = np.arange(Tmax)[None, :] >= lengths[:, None]
    m[pad] = 0
    tg[pad] = 0
    P = dict(name="zero-static", windows=windows, dt=dt, B=B, Tmax=Tmax, sd=sd, D=nw * sd, lengths=lengths, m=m, tg=tg,
             n_elems=float(B * Tmax * sd), y_given=1, st_given=1, off=0)
    ref = unit_mse_step64(m, tg, windows, lengths)
    assert (ref[3] == (lengths > 0)[:, None].astype(np.int32)).all() and ref[1] == 0.0
    assert _form_query(dt, True, B, Tmax, nw * sd, _win(windows)) == 1
    _run_accepted(P, ref, 1, _sizes(P)["small"], "failing pivots")


# --------------------------------------------------------------------------------------------------------- refused calls

def _base(name="std3", Tmax=200, dt=F32, lmode="null", B=3, sd=5, k=0):
    return _problem(name, Tmax, k, dt=dt, lmode=lmode, sd=sd, B=B)


def test_refused_calls_touch_nothing():
    import torch
    L = _lib()
    cases = []
    for lmode, dt in (("full", F32), ("null", F64)):
        P = _base(Tmax=1025, dt=dt, lmode=lmode)
        cases.append((P, _sizes(P)["t"], "Tmax 1025 %s %s" % (lmode, dt), {}))
        P = _base(name="wide3", dt=dt, lmode=lmode)
        cases.append((P, _sizes(P)["t"], "extent 2 %s %s" % (lmode, dt), {}))
    for name, Tmax in (("std3", 1025), ("wide3", 200), ("std2", 2049)):     # FIR-only shapes, small workspace
        P = _base(name=name, Tmax=Tmax)
        cases.append((P, _sizes(P)["small"], "FIR-only %s %d, small workspace" % (name, Tmax), {}))
    P = _base(name="wide3", Tmax=200)                                        # FIR-eligible, one line short: no form left
    cases.append((P, _sizes(P)["t"] - 128, "wide3 one line short of _t", {}))
    for dt in (F32, F64):
        P = _base(dt=dt, lmode="ragged", B=8)
        small = _sizes(P)["small"]
        cases.append((P, small - 128, "workspace one line short", {}))
        cases.append((P, small, "workspace NULL", {"ws": None}))
        for ne in (0.0, -1.0, float("nan")):
            cases.append((P, small, "n_elems %r" % ne, {"n_elems": ne}))
        cases.append((P, small, "D not a multiple of nw", {"D": P["D"] - 1}))
        P9 = dict(P, windows=[(0, 0, [1.0])] * 9, D=9 * P["sd"], m=np.zeros((P["B"], P["Tmax"], 9 * P["sd"]), NP_DT[dt]))
        cases.append((P9, small, "9 windows", {}))
    for P, nbytes, what, kw in cases:
        _run_refused(P, nbytes, what, **kw)
    # misaligned by 64 bytes (inside a buffer with room for the whole workspace)
    P = _base(dt=F64)
    small = _sizes(P)["small"]
    r = Run(P, small, ws=_workspace(small + 64))
    c0 = _counts()
    assert r.call(ws=r.ws.data_ptr() + 64) == EINVAL
    torch.cuda.synchronize()
    assert _moved(c0) == {} and all(b.untouched() for b in r.outputs()) and not r.ws[:small + 64].cpu().numpy().any()
    # NULL loss pointer
    r = Run(P, small)
    assert r.call(loss=None) == EINVAL
    torch.cuda.synchronize()
    assert _moved(c0) == {} and all(b.untouched() for b in r.outputs())
    assert L.mlpg_hip_unit_mse_form(torch.cuda.current_device(), None, F32, 0, 3, 200, 16, 3, *[a.ctypes.data for a in _win(SETS["std3"])[1:]]) == EINVAL


def test_fir_eligible_call_one_line_short_takes_the_one_launch_form():
    P = _base(name="std3", Tmax=200, dt=F32, lmode="null", B=9, sd=65, k=3)
    assert predict("std3", P["windows"], F32, False, True, 200) == 2
    ref = unit_mse_step64(P["m"], P["tg"], P["windows"], None, P["n_elems"])
    _run_accepted(P, ref, 1, _sizes(P)["t"] - 128, "std3 one line short of _t")


def test_empty_batches_write_a_zero_loss_and_launch_nothing():
    import torch
    win = _win(SETS["std3"])
    for B, Tmax, D in ((0, 50, 9), (2, 0, 9), (2, 50, 0)):
        loss = Buf(1, np.float64, 0, 0xFF)
        c0 = _counts()
        rc = _step(F32, None, None, None, B, Tmax, D, win, 1.0, None, None, loss.ptr(), None, None, 0)
        torch.cuda.synchronize()
        assert rc == 0 and _moved(c0) == {} and loss.host()[0] == 0.0 and loss.canary_ok(), (B, Tmax, D)


# ------------------------------------------------------------------------------------------------- workspace and streams

def _shape_list():
    """About a dozen calls of changing B, sd, Tmax, dtype and form."""
    out = []
    spec = [("std3", 100, F32, "null", 3, 5), ("std3", 700, F64, "ragged", 9, 70), ("wide3", 1500, F32, "null", 2, 8),
            ("std2", 33, F32, "ragged", 8, 3), ("asym2", 1024, F32, "null", 8, 64), ("static", 5, F64, "full", 1, 1),
            ("std3-s2", 257, F32, "null", 64, 4), ("fwd2", 96, F64, "null", 3, 65), ("dynamic-x4", 512, F32, "null", 9, 8),
            ("zero2", 129, F32, "null", 3, 63), ("std3", 1000, F32, "ragged", 9, 70), ("wide3", 96, F32, "null", 1, 1)]
    for k, (name, Tmax, dt, lmode, B, sd) in enumerate(spec):
        P = _problem(name, Tmax, k, dt=dt, lmode=lmode, sd=sd, B=B)
        P["y_given"], P["st_given"], P["off"] = 1, 1, 0
        out.append(P)
    return out


def test_one_workspace_serves_calls_of_every_shape_and_form():
    import torch
    Ps = _shape_list()
    big = max(max(_sizes(P).values()) for P in Ps)
    shared = _workspace(big)
    forms = set()
    for P in Ps:
        forms.add(predict(P["name"], P["windows"], P["dt"], P["lengths"] is not None, True, P["Tmax"]))
        fresh = Run(P, _sizes(P)["t"])
        assert fresh.call() == 0
        reuse = Run(P, big, ws=shared)
        assert reuse.call() == 0
        torch.cuda.synchronize()
        got, want = reuse.snapshot(), fresh.snapshot()
        assert all(_same_bits(a, b) for a, b in zip(got, want)), (_tag(P), _diff(got, want))
        assert _ws_ok(shared, big), _tag(P)
    assert forms == {1, 2}


def test_two_streams_with_their_own_workspaces_run_concurrently():
    import torch
    Ps = _shape_list()
    pairs = [(Ps[0], Ps[1]), (Ps[2], Ps[3]), (Ps[6], Ps[10])]
    seq = []
    for a, b in pairs:
        for P in (a, b):
            r = Run(P, _sizes(P)["t"])
            assert r.call() == 0
            torch.cuda.synchronize()
            seq.append(r.snapshot())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    runs = [Run(P, _sizes(P)["t"]) for ab in pairs for P in ab]
    torch.cuda.synchronize()
    for ra, rb in zip(runs[0::2], runs[1::2]):
        for _ in range(2):
            assert ra.call(stream=s1.cuda_stream) == 0
            assert rb.call(stream=s2.cuda_stream) == 0
    torch.cuda.synchronize()
    for r, want in zip(runs, seq):
        got = r.snapshot()
        assert all(_same_bits(x, y) for x, y in zip(got, want)), (_tag(r.P), _diff(got, want))


@pytest.mark.parametrize("case", ["one-launch", "fir"])
def test_graph_replay_matches_eager_calls(case):
    import torch
    if case == "one-launch":
        P = _problem("std3", 300, 5, dt=F64, lmode="ragged", sd=7, B=9)
        form = 1
    else:
        P = _problem("std3", 300, 5, dt=F32, lmode="null", sd=7, B=9)
        form = 2
    P["y_given"], P["st_given"], P["off"] = 1, 1, 0
    nbytes = _sizes(P)["t"]
    assert predict("std3", P["windows"], P["dt"], P["lengths"] is not None, True, 300) == form
    r = Run(P, nbytes)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert r.call(stream=side.cuda_stream) == 0          # warm: the FIR tap table exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        assert r.call(stream=side.cuda_stream) == 0
    torch.cuda.synchronize()
    rng = np.random.RandomState(99)
    for rep in range(3):
        m = rng.randn(*P["m"].shape).astype(NP_DT[P["dt"]])
        tg = rng.randn(*P["tg"].shape).astype(NP_DT[P["dt"]])
        if P["lengths"] is not None:
            pad = np.arange(P["Tmax"])[None, :] >= P["lengths"][:, None]
            m[pad] = 0
            tg[pad] = 0
        r.mean.put(m)
        r.target.put(tg)
        r.reset()
        c0 = _counts()
        g.replay()
        torch.cuda.synchronize()
        assert _moved(c0) == {}                              # a replay goes past the launch counters
        got = r.snapshot()
        Q = dict(P, m=m, tg=tg)
        e = Run(Q, nbytes)
        c0 = _counts()
        assert e.call() == 0
        torch.cuda.synchronize()
        assert _moved(c0) == ({K_FIR: 2} if form == 2 else {K_FUSED: 1})
        want = e.snapshot()
        assert all(_same_bits(a, b) for a, b in zip(got, want)), (case, rep, _diff(got, want))
        assert _ws_ok(r.ws, nbytes)


def test_wrapper_passes_lengths_and_n_elems_through():
    import torch
    from nnmnkwii_amd import _hip
    P = _problem("std3", 150, 2, dt=F64, lmode="ragged", sd=6, B=9)
    y_ref, loss_ref, grad_ref, st_ref = unit_mse_step64(P["m"], P["tg"], P["windows"], P["lengths"], 777.0)
    loss, grad, y, st = _hip.unit_mse_step(torch.from_numpy(P["m"]).cuda(), torch.from_numpy(P["tg"]).cuda(), P["windows"],
                                           lengths=torch.from_numpy(P["lengths"]).cuda(), n_elems=777.0, want_y=True,
                                           want_status=True)
    ok = st_ref == 0
    _check_rows(y.cpu().numpy(), y_ref, P["lengths"], ok, 1e-10, "wrapper y")
    _check_rows(grad.cpu().numpy(), grad_ref, P["lengths"], ok, 1e-10, "wrapper grad")
    assert abs(float(loss) - loss_ref) <= 1e-11 * loss_ref and not st.cpu().numpy().any()
