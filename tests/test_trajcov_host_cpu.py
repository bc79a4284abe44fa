"""The text of csrc/mlpg_trajcov.hip (with csrc/assemble.h and csrc/device_prims.h) run on the CPU (-m "not gpu"): compiled for
the host against the shim tests/gmm_host/common.h plus tests/trajcov_host/extras.h into a stand-alone program (its own main)
under the address and undefined-behaviour sanitizers, run as a child process, and compared with tools/trajcov_model.py: the band,
the status, the likelihood (given the program's own logdet) and both gradients BIT FOR BIT -- they are made of + - x / alone --
and logdet within (T + 4) 2^-53 sum_t |log D_t| (the sequential sum plus log's last place).  Every array is an exact-size heap
block: strided arrays end behind their last row's last column; rows at or past an utterance's length hold NaN; the outputs are
pre-filled with -7 and their foreign columns must still hold it.  Nothing is loaded into Python under a sanitizer.

Two planted defects show that the harness bites: see test_planted_*."""
import os
import subprocess

import numpy as np
import pytest

import trajcov_cases as C
from trajcov_cases import TM

ROOT = C.ROOT
SENTINEL = -7


def build(d, edit=None):
    """The host program of the kernel text in directory d; `edit` (old, new) plants a defect: old must occur exactly once."""
    from nnmnkwii_amd.csrc import build as hip_build
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "mlpg_trajcov.hip")).read()
    if edit is not None:
        assert src.count(edit[0]) == 1, edit[0]
        src = src.replace(edit[0], edit[1])
    os.makedirs(d / "csrc" / "x")
    os.makedirs(d / "include")
    (d / "csrc" / "x" / "mlpg_trajcov_host.inc").write_text(src)
    (d / "include" / "nnmnkwii_trajectory.h").write_text(open(os.path.join(ROOT, "include", "nnmnkwii_trajectory.h")).read())
    for sub, name, to in (("tests/gmm_host", "common.h", "common.h"), ("tests/gvmlpg_host", "extras.h", "gvmlpg_extras.h"),
                          ("tests/trajcov_host", "extras.h", "extras.h"), ("tests/trajcov_host", "main.cpp", "main.cpp"),
                          ("nnmnkwii_amd/csrc", "assemble.h", "assemble.h"), ("nnmnkwii_amd/csrc", "device_prims.h", "device_prims.h")):
        (d / to).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "trajcov_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("trajcov_host"))


def strided(a, ld, fill=np.nan):
    """(rows, width) -> the exact-size flat block of rows with stride ld, the foreign columns holding `fill`."""
    rows, width = a.shape
    if rows == 0 or width == 0:
        return np.zeros(0, dtype=a.dtype)
    flat = np.full((rows - 1) * ld + width, fill, dtype=a.dtype)
    for r in range(rows):
        flat[r * ld:r * ld + width] = a[r]
    return flat


def unstrided(flat, rows, ld, width):
    out = np.zeros((rows, width), dtype=flat.dtype)
    foreign = np.ones(flat.shape, dtype=bool)
    for r in range(rows):
        out[r] = flat[r * ld:r * ld + width]
        foreign[r * ld:r * ld + width] = False
    return out, flat[foreign]


def make_case(seed, B, Tmax, sd, wname, mode, dtype, lengths, pad=2):
    win = C.WINDOWS[wname]
    nw = len(win)
    D = nw * sd
    live = TM.live_frames(lengths, B, Tmax)
    var = C.variances(seed, B, Tmax, sd, wname, mode, dtype)
    mean = C.features(seed + 1, B, Tmax, D, dtype)
    target = C.features(seed + 2, B, Tmax, sd, dtype)
    cbar = np.zeros((B, Tmax, sd), dtype=dtype)
    for b in range(B):
        T = int(live[b])
        v = None if mode == TM.VAR_UNIT else (var if mode == TM.VAR_GLOBAL else var[b])
        cbar[b, :T] = TM.mean_trajectory(mean[b], v, win, T, sd).astype(dtype)
        for a in (mean, target, cbar) + ((var,) if mode == TM.VAR_FRAME else ()):
            a[b, T:] = np.nan                                   # no row at or past T is read
    return dict(B=B, Tmax=Tmax, sd=sd, D=D, windows=win, wname=wname, mode=mode, dtype=dtype, lengths=lengths, var=var, mean=mean,
                target=target, cbar=cbar, ld_in=D + pad, ld_band=sd + pad, ld_cbar=sd + pad + 1, ld_target=sd + pad)


def run_host(program, case, want_band=True, do_nll=True, want_gm=True, want_gv=True, check=True):
    d, exe = program
    B, Tmax, sd, D, win, mode, dt = (case[k] for k in ("B", "Tmax", "sd", "D", "windows", "mode", "dtype"))
    Q = TM.window_set(win)[1]
    want_gv = want_gv and mode != TM.VAR_UNIT
    L = case["lengths"]
    head = [B, Tmax, sd, len(win), int(dt == np.float64), mode, L is not None, want_band, do_nll, want_gm, want_gv, case["ld_in"],
            case["ld_band"], case["ld_cbar"], case["ld_target"], Q]
    rows = B * Tmax
    with open(d / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        f.write(np.asarray(L if L is not None else [0] * B, dtype=np.int32).tobytes())
        f.write(np.array([w[0] for w in win], dtype=np.int32).tobytes())
        f.write(np.array([w[1] for w in win], dtype=np.int32).tobytes())
        f.write(np.concatenate([w[2] for w in win]).astype(np.float64).tobytes())
        if mode == TM.VAR_FRAME:
            f.write(strided(case["var"].reshape(rows, D), case["ld_in"]).tobytes())
        elif mode == TM.VAR_GLOBAL:
            f.write(case["var"].tobytes())
        if do_nll:
            f.write(strided(case["mean"].reshape(rows, D), case["ld_in"]).tobytes())
            f.write(strided(case["cbar"].reshape(rows, sd), case["ld_cbar"]).tobytes())
            f.write(strided(case["target"].reshape(rows, sd), case["ld_target"]).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    if not check and r.returncode != 0:
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(d / "out.bin", "rb").read()
    res, o = {}, 0
    if want_band:
        nrow = (Q + 1) * rows
        n = ((nrow - 1) * case["ld_band"] + sd) if nrow and sd else 0
        band, foreign = unstrided(np.frombuffer(raw[:8 * n]), nrow, case["ld_band"], sd)
        assert (foreign == SENTINEL).all()
        res["band"] = band.reshape(Q + 1, B, Tmax, sd)
        o = 8 * n
    res["logdet"] = np.frombuffer(raw[o:o + 8 * B * sd]).reshape(B, sd)
    o += 8 * B * sd
    res["status"] = np.frombuffer(raw[o:o + 4 * B * sd], dtype=np.int32).reshape(B, sd)
    o += 4 * B * sd
    if do_nll:
        res["nll"] = np.frombuffer(raw[o:o + 8 * B * sd]).reshape(B, sd)
        o += 8 * B * sd
        isz = np.dtype(dt).itemsize
        if want_gm:
            res["gm"] = np.frombuffer(raw[o:o + isz * rows * D], dtype=dt).reshape(B, Tmax, D)
            o += isz * rows * D
        if want_gv:
            n = rows * D if mode == TM.VAR_FRAME else D
            res["gv"] = np.frombuffer(raw[o:o + isz * n], dtype=dt).reshape((B, Tmax, D) if mode == TM.VAR_FRAME else (D,))
            o += isz * n
    assert o == len(raw)
    return res


def check_case(program, case):
    B, Tmax, sd, win, mode = (case[k] for k in ("B", "Tmax", "sd", "windows", "mode"))
    got = run_host(program, case)
    band, logdet, status = TM.covariance_batch(case["var"], win, case["lengths"], B, Tmax, sd)
    assert np.array_equal(got["status"], status) and not status.any()
    assert C.same_bits(got["band"], band)
    live = TM.live_frames(case["lengths"], B, Tmax)
    for b in range(B):
        v = None if mode == TM.VAR_UNIT else (case["var"] if mode == TM.VAR_GLOBAL else case["var"][b])
        bound = C.logdet_bound(v, case["wname"], int(live[b]), sd)
        assert (np.abs(got["logdet"][b] - logdet[b]) <= bound).all(), (b, np.abs(got["logdet"][b] - logdet[b]).max(), bound.min())
    # the forward sweep alone: the same logdet bits, no band
    alone = run_host(program, case, want_band=False, do_nll=False)
    assert C.same_bits(alone["logdet"], got["logdet"]) and np.array_equal(alone["status"], status)
    # the likelihood from the program's own logdet
    clean = {k: np.nan_to_num(case[k]) for k in ("mean", "cbar", "target")}
    var = case["var"] if mode != TM.VAR_FRAME else np.where(np.isnan(case["var"]), 1.0, case["var"]).astype(case["dtype"])
    nll, gm, gv = TM.nll_batch(clean["mean"], var, win, clean["cbar"], clean["target"], case["lengths"], band, got["logdet"])
    assert C.same_bits(got["nll"], nll)
    assert C.same_bits(got["gm"], gm)
    if mode != TM.VAR_UNIT:
        assert C.same_bits(got["gv"], gv)
    return got


SHAPES = [(1, 1, 1, None), (1, 2, 3, None), (3, 5, 3, [5, 0, 3]), (2, 17, 65, [4, 17]), (1, 66, 2, None), (2, 9, 130, [9, 8])]


@pytest.mark.parametrize("B,Tmax,sd,lengths", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kernel_text_on_the_host(program, B, Tmax, sd, lengths, dtype):
    for i, wname in enumerate(C.WINDOWS):
        mode = C.MODES[(i + Tmax + sd) % 3]
        check_case(program, make_case(B + Tmax + sd + i, B, Tmax, sd, wname, mode, dtype, lengths))


def test_every_variance_mode_and_window_set(program):
    for wname in C.WINDOWS:
        for mode in C.MODES:
            check_case(program, make_case(7, 2, 8, 3, wname, mode, np.float64, [8, 5]))


def test_tight_dynamic_variances(program):
    case = make_case(3, 2, 17, 2, "std3", TM.VAR_FRAME, np.float64, [17, 6])
    case["var"][..., 2:] *= 0.01
    live = TM.live_frames(case["lengths"], 2, 17)
    for b in range(2):
        case["cbar"][b, :live[b]] = TM.mean_trajectory(case["mean"][b], case["var"][b], case["windows"], int(live[b]), 2)
    check_case(program, case)


def test_non_positive_pivot(program):
    case = make_case(5, 2, 9, 3, "std3", TM.VAR_FRAME, np.float64, [9, 6])
    case["var"][0, 5, 1] = -1e-3
    got = run_host(program, case, do_nll=False)
    band, logdet, status = TM.covariance_batch(case["var"], case["windows"], case["lengths"], 2, 9, 3)
    assert np.array_equal(got["status"], status) and status[0, 1] == 6 and status.sum() == 6
    assert np.isnan(got["band"][:, 0, :, 1]).all() and np.isnan(got["logdet"][0, 1])
    assert C.same_bits(got["band"], band)                         # the neighbours untouched, the pad rows zero


# ---- the harness bites ------------------------------------------------------------------------------------------------------------

def planted(tmp_path, edit):
    prog = build(tmp_path, edit)
    case = make_case(5, 2, 9, 3, "std3", TM.VAR_FRAME, np.float64, [9, 6], pad=0)
    case.update(ld_cbar=3)
    got = run_host(prog, case, check=False)
    if isinstance(got, subprocess.CompletedProcess):
        assert "Sanitizer" in got.stderr or "runtime error" in got.stderr, got.stderr[-2000:]
        return "sanitizer"
    band = TM.covariance_batch(case["var"], case["windows"], case["lengths"], 2, 9, 3)[0]
    return "passed" if C.same_bits(got["band"], band) else "mismatch"


def test_planted_dropped_j2_term(tmp_path):
    edit = ("      for (int j = 2; j <= Q; ++j) acc += m[j] * s[j];\n", "      for (int j = 2; j < Q; ++j) acc += m[j] * s[j];\n")
    assert planted(tmp_path / "a", edit) == "mismatch"
    assert planted(tmp_path / "ok", None) == "passed"


def test_planted_factor_row_read_below_the_first(tmp_path):
    """The backward sweep's read-ahead without its bound: row -1 .. -4 of the last utterance's first plane lie in front of the
    heap block when the utterance is the first."""
    edit = ("fr[kTcAhead - 1][k] = t - kTcAhead >= 0 ? ", "fr[kTcAhead - 1][k] = t - kTcAhead >= -4 ? ")
    assert planted(tmp_path / "a", edit) == "sanitizer"
