"""The texts of csrc/mlpg_vargrad.hip and csrc/mlpg_streams_bwd.hip (shared body csrc/vargrad_element.h) run on the CPU
(-m "not gpu"): compiled for the host against the shim tests/gmm_host/common.h plus tests/vargrad_host/extras.h into a
stand-alone program under the address and undefined-behaviour sanitizers, run as a child process, and compared with
tests/vargrad64.py and tests/streamgrad64.py within the bounds of tests/test_var_grad_gpu.py (its rule, restated in `bar`) and
TOL of tests/test_backward_streams_gpu.py.  The kernels are the epilogue behind the backward solve: they get the reference's y
and grad_mean, rounded to the input dtype, and give grad_var.  Each element reads neighbours t - l .. t + u of y: every array is
an exact-size heap block, rows at and past lengths[b] hold NaN in every input, so do the variances the edge mask removes, and --
for the stream table -- the columns that belong to no member; outputs are pre-filled with -7.  The kernels have no LDS (no
``extern __shared__``) and no workspace.  Nothing is loaded into Python under a sanitizer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import streamgrad64  # noqa: E402
import vargrad64  # noqa: E402
from cases import WINDOW_SETS  # noqa: E402

F32, F64 = np.float32, np.float64
TOL = {F64: 1e-10, F32: 3e-6}
SENTINEL = -7
PASS = 3
WORST = {F32: 0.0, F64: 0.0}


def test_the_bounds_are_the_gpu_tests():
    text = open(os.path.join(ROOT, "tests", "test_backward_streams_gpu.py")).read()
    assert eval(re.search(r"^TOL = (\{.*\})$", text, re.M).group(1), {"f32": F32, "f64": F64}) == TOL
    text = open(os.path.join(ROOT, "tests", "test_var_grad_gpu.py")).read()
    assert text.count("tol = 1e-10 if dt == np.float64 else 3e-6") == 1 and (TOL[F64], TOL[F32]) == (1e-10, 3e-6)
    assert text.count("scale = np.maximum(np.abs(ref).max(axis=(1, 2)), 0.05 * terms)") == 1        # the rule `bar` restates


def build(d, edit=None):
    """The host program of the kernel texts in directory d; `edit` (file, old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    csrc = os.path.join(ROOT, "nnmnkwii_amd", "csrc")
    names = ("mlpg_vargrad.hip", "mlpg_streams_bwd.hip", "vargrad_element.h")
    text = {name: open(os.path.join(csrc, name)).read() for name in names}
    assert all(text[name].count("extern __shared__") == 0 for name in names)
    if edit is not None:
        assert text[edit[0]].count(edit[1]) == 1, edit[1]
        text[edit[0]] = text[edit[0]].replace(edit[1], edit[2])
    os.makedirs(d / "csrc" / "x")
    for name in names:
        (d / "csrc" / "x" / (name if name.endswith(".h") else name.replace(".hip", "_host.inc"))).write_text(text[name])
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/vargrad_host", "extras.h"), ("tests/vargrad_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "vargrad_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("vargrad_host"))


def host_call(program, op, dt, mode, B, Tmax, sd, ld_in, ld_out, ld_status, members, windows, lengths, status, arrays, has_gvar=True,
              has_status=True, check=True):
    """(grad_mean (B, Tmax, ld_in), grad_var or None, status (B, ld_status)) after the call.  arrays: grad_out (op 1), var, mean,
    y, grad_mean, grad_var (if has_gvar), of dt."""
    d, exe = program
    var = arrays[1 if op == 1 else 0]
    L = np.zeros(B, dtype=np.int32) if lengths is None else np.asarray(lengths, dtype=np.int32)
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([op, dt == F64, mode, B, Tmax, sd, ld_in, ld_out, ld_status, len(members), len(windows), lengths is not None,
                          has_gvar, has_status, var.size], dtype=np.int64).tobytes())
        f.write(np.array(members, dtype=np.int32).reshape(-1, 5).T.tobytes())
        f.write(np.array([l for l, _, _ in windows], dtype=np.int32).tobytes())
        f.write(np.array([u for _, u, _ in windows], dtype=np.int32).tobytes())
        f.write(np.concatenate([np.asarray(c, dtype=F64) for _, _, c in windows] + [np.zeros(0)]).tobytes())
        f.write(L.tobytes())
        f.write(np.ascontiguousarray(status, dtype=np.int32).tobytes())
        for a in arrays:
            assert a.dtype == dt
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(d / "out.bin", "rb").read()
    n = B * Tmax * ld_in
    k = n * np.dtype(dt).itemsize
    gm = np.frombuffer(raw[:k], dtype=dt).reshape(B, Tmax, ld_in)
    gv = np.frombuffer(raw[k:2 * k], dtype=dt).reshape(B, Tmax, ld_in) if has_gvar else None
    return gm, gv, np.frombuffer(raw[(2 * k if has_gvar else k):], dtype=np.int32).reshape(B, ld_status)


def masked_entries(windows, lengths, T, sd):
    """Boolean (B, T, nw sd): live entries whose precision the edge mask (or the [-0:] rule) removes."""
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


def bar(M, V, y, gm, gv_ref, windows):
    """Per utterance, what tests/test_var_grad_gpu.py measures the error against: the largest |grad_var|, or 1/20 of the largest
    |grad_mean tau| (|mu| + sum|c| max|y|) where grad_var cancels."""
    S = max(float(np.abs(np.asarray(c, dtype=F64)).sum()) for _, _, c in windows)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = np.where(V != 0, (V.dtype.type(1) / V).astype(F64), 0.0)
    ymax = np.abs(y).max(axis=(1, 2))[:, None, None]
    terms = (np.abs(gm) * np.abs(tau) * (np.abs(M.astype(F64)) + S * ymax)).max(axis=(1, 2))
    return np.maximum(np.abs(gv_ref).max(axis=(1, 2)), 0.05 * terms)


def problem(seed, windows, T, sd, lengths, dt, global_var):
    """Inputs of dt and the float64 reference: M, V (per-frame values either way), y, grad_mean, grad_var, and the poisoned copies
    the kernel gets: NaN in the rows at and past each length and in the variances the edge mask removes."""
    rng = np.random.RandomState(seed)
    B, D = len(lengths), len(windows) * sd
    M = rng.randn(B, T, D).astype(dt)
    vg = (rng.rand(D) + 0.1).astype(dt)
    V = np.ascontiguousarray(np.broadcast_to(vg, (B, T, D))) if global_var else (rng.rand(B, T, D) + 0.1).astype(dt)
    go = rng.randn(B, T, sd).astype(dt)
    y, gm, gv = vargrad64.mlpg_var_grad64(M, V, go, windows, lengths)
    pad = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
    dirty = {"M": M.copy(), "V": V.copy(), "y": y.astype(dt), "gm": gm.astype(dt), "go": go.copy()}
    for a in dirty.values():
        a[pad] = np.nan
    if not global_var:
        dirty["V"][masked_entries(windows, lengths, T, sd)] = np.nan
    return M, V, vg, y, gm, gv, dirty


def judge(gv, ref, lengths, masked, scale, dt):
    """None if grad_var is right, else what is wrong with it."""
    gv = gv.astype(F64)
    pad = np.arange(gv.shape[1])[None, :] >= np.asarray(lengths)[:, None]
    if gv[pad].any() or np.isnan(gv[pad]).any():
        return "padding rows not zero"
    if gv[masked].any() or np.isnan(gv[masked]).any():
        return "masked entries not zero"
    if not np.isfinite(gv).all():
        return "not finite"
    err = np.abs(gv - ref).max(axis=(1, 2))
    if (scale > 0).any():
        WORST[dt] = max(WORST[dt], float((err[scale > 0] / scale[scale > 0]).max() / TOL[dt]))
    return None if (err <= TOL[dt] * scale).all() else "error above the bound: %r" % (err / np.where(scale > 0, scale, 1)).tolist()


def lengths_for(T):
    return [T, 1, 0] + ([T - 1] if T > 2 else [])


@pytest.mark.parametrize("T", [1, 2, 3, 5, 65])
@pytest.mark.parametrize("wname", sorted(WINDOW_SETS))
def test_var_grad_kernel_text_on_the_host(program, wname, T):
    windows = WINDOW_SETS[wname]
    sd = 3 if T < 65 else 5                                       # (T = 65, sd = 5: a second workgroup)
    lengths = lengths_for(T)
    B, D = len(lengths), len(windows) * sd
    for dt in (F32, F64):
        for global_var in (False, True):
            M, V, vg, y, gm, gv_ref, dirty = problem(T * 10 + len(wname), windows, T, sd, lengths, dt, global_var)
            status = np.zeros((B, sd), dtype=np.int32)
            prefill = np.full((B, T, D), SENTINEL, dtype=dt)
            _, gv, _ = host_call(program, 0, dt, int(global_var), B, T, sd, D, sd, sd, [], windows, lengths, status,
                                 [vg if global_var else dirty["V"], dirty["M"], dirty["y"], dirty["gm"], prefill])
            what = judge(gv, gv_ref, lengths, masked_entries(windows, lengths, T, sd), bar(M, V, y, gm, gv_ref, windows), dt)
            assert what is None, (wname, T, dt.__name__, global_var, what)
    print("var_grad %s T=%d: worst error / bound so far: float32 %.3g, float64 %.3g" % (wname, T, WORST[F32], WORST[F64]))


def test_var_grad_without_lengths_and_a_failed_system(program):
    """lengths = NULL: every row is live.  A system whose status is not 0 gets zeros in every window's column, whatever it holds."""
    windows, T, sd = WINDOW_SETS["std3"], 5, 2
    M, V, vg, y, gm, gv_ref, dirty = problem(3, windows, T, sd, [T, T], F64, False)
    status = np.array([[0, 0], [7, 0]], dtype=np.int32)
    for k in ("M", "V", "y", "gm"):
        dirty[k][1, :, 0::sd] = np.nan                           # system (1, 0) failed: nothing of it is read
    _, gv, _ = host_call(program, 0, F64, 0, 2, T, sd, 3 * sd, sd, sd, [], windows, None, status,
                         [dirty["V"], dirty["M"], dirty["y"], dirty["gm"], np.full((2, T, 3 * sd), SENTINEL, dtype=F64)])
    assert not gv[1, :, 0::sd].any()
    gv_ref = gv_ref.copy()
    gv_ref[1, :, 0::sd] = 0.0
    assert judge(gv, gv_ref, [T, T], masked_entries(windows, [T, T], T, sd), bar(M, V, y, gm, gv_ref, windows), F64) is None


# ---- the stream table ----------------------------------------------------------------------------------------------------------------

def stream_layout(windows):
    """Two dynamic members of one window list with a pass-through member and gaps between them, ld_in above their sum: input
    column 0, the columns between the members and the last two belong to nobody.  (streams, ld_in, ld_out)"""
    nw = len(windows)
    a = {"in_col": 1, "out_col": 1, "static_dim": 3, "windows": windows}
    p = {"in_col": 1 + 3 * nw + 2, "out_col": 5, "static_dim": 2, "windows": None}
    c = {"in_col": p["in_col"] + 2 + 1, "out_col": 8, "static_dim": 1, "windows": windows}
    return [a, p, c], c["in_col"] + nw + 2, 10


@pytest.mark.parametrize("T", [1, 2, 3, 5, 65])
@pytest.mark.parametrize("wname", sorted(WINDOW_SETS))
def test_streams_bwd_kernel_text_on_the_host(program, wname, T):
    """One launch for the two dynamic members, one for the pass-through member, on the same arrays: grad_var against
    tests/streamgrad64.py, grad_mean of the pass-through member exact, every column of no member untouched."""
    windows = WINDOW_SETS[wname]
    streams, ld_in, ld_out = stream_layout(windows)
    lengths = lengths_for(T)
    B = len(lengths)
    oi, oo = streamgrad64.owned(streams, ld_in, ld_out)
    pad = np.arange(T)[None, :] >= np.asarray(lengths)[:, None]
    dyn = [s for s in streams if s["windows"]]
    for dt in (F32, F64):
        for global_var in (False, True):
            rng = np.random.RandomState(T * 100 + len(wname) + global_var)
            M = rng.randn(B, T, ld_in).astype(dt)
            vg = (rng.rand(ld_in) + 0.1).astype(dt)
            V = np.ascontiguousarray(np.broadcast_to(vg, M.shape)) if global_var else (rng.rand(B, T, ld_in) + 0.1).astype(dt)
            go = rng.randn(B, T, ld_out).astype(dt)
            y, gm, gv_ref = streamgrad64.multi_stream_grad64(M, V, go, streams, lengths)
            # what the kernel gets: NaN in the columns of no member, in the padding rows, in the masked variances, and in the
            # variances of the pass-through member
            Mk, Vk, yk, gmk, gok = M.copy(), V.copy(), y.astype(dt), gm.astype(dt), go.copy()
            vgk = vg.copy()
            for a in (Mk, Vk, gmk):
                a[:, :, ~oi] = np.nan
                a[pad] = np.nan
            for a in (yk, gok):
                a[:, :, ~oo] = np.nan
                a[pad] = np.nan
            vgk[~oi] = np.nan
            p = streams[1]
            Vk[:, :, p["in_col"]:p["in_col"] + 2] = np.nan
            vgk[p["in_col"]:p["in_col"] + 2] = np.nan
            gmk[:, :, p["in_col"]:p["in_col"] + 2] = SENTINEL       # the pass-through launch writes it
            masks = {}
            for s in dyn:
                cols = streamgrad64.stream_cols(s)
                masks[s["in_col"]] = masked_entries(windows, lengths, T, s["static_dim"])
                if not global_var:
                    blk = Vk[:, :, cols]
                    blk[masks[s["in_col"]]] = np.nan
                    Vk[:, :, cols] = blk
            gvk = np.full((B, T, ld_in), SENTINEL, dtype=dt)
            status = np.full((B, ld_out), 5, dtype=np.int32)        # (status columns follow the output columns)
            for s in dyn:
                status[:, s["out_col"]:s["out_col"] + s["static_dim"]] = 0
            members = [[0, dyn[0]["in_col"], dyn[0]["out_col"], 3, dyn[0]["out_col"]], [3, dyn[1]["in_col"], dyn[1]["out_col"], 1, dyn[1]["out_col"]]]
            gm1, gv1, st1 = host_call(program, 1, dt, int(global_var), B, T, 0, ld_in, ld_out, ld_out, members, windows, lengths, status,
                                      [gok, vgk if global_var else Vk, Mk, yk, gmk, gvk])
            assert gm1.tobytes() == gmk.tobytes() and st1.tobytes() == status.tobytes()       # the dynamic launch writes grad_var alone
            gm2, gv2, st2 = host_call(program, 1, dt, PASS, B, T, 0, ld_in, ld_out, ld_out, [[0, p["in_col"], p["out_col"], 2, p["out_col"]]],
                                      windows, lengths, status, [gok, vgk if global_var else Vk, Mk, yk, gm1, gv1])
            # columns of no member: untouched in both outputs
            assert (gv2[:, :, ~oi] == SENTINEL).all() and np.isnan(gm2[:, :, ~oi]).all()
            # the pass-through member: grad_mean = grad_out on live rows, 0 on padding; grad_var 0; status 0
            pc = slice(p["in_col"], p["in_col"] + 2)
            assert np.array_equal(gm2[:, :, pc], np.where(pad[:, :, None], 0, go[:, :, p["out_col"]:p["out_col"] + 2]).astype(dt))
            assert not gv2[:, :, pc].any() and not st2[:, p["out_col"]:p["out_col"] + 2].any()
            assert (st2[:, [0, 4, 7, 9]] == 5).all()
            for s in dyn:
                cols = streamgrad64.stream_cols(s)
                oc = slice(s["out_col"], s["out_col"] + s["static_dim"])
                scale = bar(M[:, :, cols], V[:, :, cols], y[:, :, oc], gm[:, :, cols], gv_ref[:, :, cols], windows)
                what = judge(gv2[:, :, cols], gv_ref[:, :, cols], lengths, masks[s["in_col"]], scale, dt)
                assert what is None, (wname, T, dt.__name__, global_var, s["in_col"], what)
            assert gm2[:, :, oi & ~np.isin(np.arange(ld_in), np.arange(pc.start, pc.stop))].tobytes() == \
                gmk[:, :, oi & ~np.isin(np.arange(ld_in), np.arange(pc.start, pc.stop))].tobytes()
    print("streams_bwd %s T=%d: worst error / bound so far: float32 %.3g, float64 %.3g" % (wname, T, WORST[F32], WORST[F64]))


def test_pass_through_without_grad_var_and_status(program):
    streams, ld_in, ld_out = stream_layout(WINDOW_SETS["std2"])
    p = streams[1]
    rng = np.random.RandomState(1)
    go = rng.randn(2, 3, ld_out)
    gm = np.full((2, 3, ld_in), float(SENTINEL))
    nan = np.full((2, 3, ld_in), np.nan)
    got, _, st = host_call(program, 1, F64, PASS, 2, 3, 0, ld_in, ld_out, ld_out, [[0, p["in_col"], p["out_col"], 2, p["out_col"]]],
                           WINDOW_SETS["std2"], [3, 1], np.full((2, ld_out), 5), [go, nan, nan, np.full((2, 3, ld_out), np.nan), gm],
                           has_gvar=False, has_status=False)
    want = gm.copy()
    want[:, :, p["in_col"]:p["in_col"] + 2] = go[:, :, p["out_col"]:p["out_col"] + 2]
    want[1, 1:, p["in_col"]:p["in_col"] + 2] = 0
    assert np.array_equal(got, want) and (st == 5).all()


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit, T=5, lengths=(5, 3)):
    """The dense kernel on the text with `edit`: "sanitizer", or judge's answer."""
    prog = build(tmp_path, edit)
    windows, sd = WINDOW_SETS["std3"], 2
    lengths = list(lengths)
    M, V, vg, y, gm, gv_ref, dirty = problem(11, windows, T, sd, lengths, F64, False)
    B, D = len(lengths), 3 * sd
    got = host_call(prog, 0, F64, 0, B, T, sd, D, sd, sd, [], windows, lengths, np.zeros((B, sd), dtype=np.int32),
                    [dirty["V"], dirty["M"], dirty["y"], dirty["gm"], np.full((B, T, D), SENTINEL, dtype=F64)], check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    return judge(got[1], gv_ref, lengths, masked_entries(windows, lengths, T, sd), bar(M, V, y, gm, gv_ref, windows), F64)


def test_planted_stencil_one_row_past_the_length(tmp_path):
    """The y stencil takes row `len`: behind the last utterance's last row the read leaves the heap block.  (Inside the block
    the extra tap cannot show: it reaches only row len - 1, where the edge mask has removed every window that has a tap at +1.)"""
    edit = ("vargrad_element.h", "tt >= 0 && tt < len)", "tt >= 0 && tt <= len)")
    assert planted(tmp_path / "a", edit, lengths=(3, 5)) == "sanitizer"


def test_planted_edge_mask_one_row_short(tmp_path):
    """The mask lets the last masked row through: its variance (NaN, never to be read) reaches grad_var."""
    edit = ("vargrad_element.h", "t >= len - ws.mw);", "t > len - ws.mw);")
    assert planted(tmp_path / "a", edit) == "masked entries not zero"


def test_planted_store_one_element_past_the_batch(tmp_path):
    """One thread more than elements: it stores behind grad_var's last element."""
    edit = ("mlpg_vargrad.hip", "if (e >= total) return;", "if (e > total) return;")
    assert planted(tmp_path / "a", edit) == "sanitizer"
