"""The text of csrc/mlpg_gv.hip (with csrc/assemble.h and csrc/device_prims.h) run on the CPU (-m "not gpu"): compiled for the
host against the shim tests/gmm_host/common.h plus tests/gvmlpg_host/extras.h (the cross-lane moves) into a stand-alone program
under the address and undefined-behaviour sanitizers, run as a child process, and compared with tools/gvmlpg_model.py.  This
checks the chunk layout, the halo, the masking of pad frames, the report and status and every bound of an array (LDS is an
exact-size heap block); it cannot check the hardware's cross-lane moves (tests/test_gvmlpg_gpu.py does).  Nothing is loaded into
Python under a sanitizer.

The tolerance of kernel against model (tests/gvmlpg_cases.py) comes from here: the worst |y - y_ref| / (eps max|y|) against the
model run in long double at n_iter = 100 on these shapes is printed, and asserted to be at most the recorded WORST_RATIO."""
import os
import subprocess

import numpy as np
import pytest

import gvmlpg_cases as C
from gvmlpg_cases import GV

ROOT = C.ROOT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from nnmnkwii_amd.csrc import build as hip_build
    d = tmp_path_factory.mktemp("gvmlpg_host")
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "mlpg_gv.hip")).read()
    marker = "extern __shared__ double lds[];"
    assert src.count(marker) == 1
    (d / "mlpg_gv_host.inc").write_text(src.replace(marker, "double *lds = g_dyn_lds;"))
    for sub, name in (("tests/gmm_host", "common.h"), ("tests/gvmlpg_host", "extras.h"), ("tests/gvmlpg_host", "main.cpp"),
                      ("nnmnkwii_amd/csrc", "assemble.h"), ("nnmnkwii_amd/csrc", "device_prims.h")):
        (d / name).write_text(open(os.path.join(ROOT, sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "gvmlpg_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_host(program, case, n_iter, step=None, init=1, in_place=False, omega_scale=1.0):
    d, exe = program
    dt = case["dtype"]
    B, Tmax, sd, D = case["B"], case["Tmax"], case["sd"], case["D"]
    win = case["windows"]
    mode = GV.var_mode_of(case["var"])
    L = case["lengths"]
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([B, Tmax, D, len(win), int(dt == np.float64), mode, L is not None, n_iter, init, in_place],
                         dtype=np.int64).tobytes())
        f.write(np.array([omega_scale, -1.0 if step is None else step]).tobytes())
        f.write(np.asarray(L if L is not None else [0] * B, dtype=np.int32).tobytes())
        f.write(np.array([w[0] for w in win], dtype=np.int32).tobytes())
        f.write(np.array([w[1] for w in win], dtype=np.int32).tobytes())
        f.write(np.concatenate([w[2] for w in win]).astype(np.float64).tobytes())
        f.write(np.ascontiguousarray(case["mean"], dtype=dt).tobytes())
        if case["var"] is not None:
            f.write(np.ascontiguousarray(case["var"], dtype=dt).tobytes())
        f.write(np.ascontiguousarray(case["y_in"], dtype=dt).tobytes())
        f.write(case["gv_mean"].astype(np.float64).tobytes())
        f.write(case["gv_prec"].astype(np.float64).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    raw = open(d / "out.bin", "rb").read()
    ny = B * Tmax * sd * np.dtype(dt).itemsize
    y = np.frombuffer(raw[:ny], dtype=dt).reshape(B, Tmax, sd)
    o = ny
    rep = np.frombuffer(raw[o:o + B * sd * 32]).reshape(B, sd, 4)
    o += B * sd * 32
    st = np.frombuffer(raw[o:o + B * sd * 4], dtype=np.int32).reshape(B, sd)
    o += B * sd * 4
    return y, rep, st, np.frombuffer(raw[o:]).reshape(B, sd)


SHAPES = [(1, 1, 1, None), (1, 2, 1, None), (1, 65, 3, None), (3, 130, 5, [130, 0, 64]), (2, 257, 4, None)]


@pytest.mark.parametrize("B,Tmax,sd,lengths", SHAPES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_iter", [0, 1, 100])
def test_kernel_text_on_the_host(program, B, Tmax, sd, lengths, dtype, n_iter):
    wname = ("std3", "std2", "static")[(B + Tmax) % 3]
    mode = (GV.VAR_FRAME, GV.VAR_GLOBAL, GV.VAR_UNIT)[(Tmax + sd) % 3]
    case = C.make_case(B + Tmax + sd, B, Tmax, sd, wname, mode, dtype, lengths)
    y, rep, st, gv = run_host(program, case, n_iter, in_place=bool(Tmax % 2))
    y_m, rep_m, st_m = C.model(case, n_iter)
    live = GV.live_frames(lengths, B, Tmax)
    pad = np.arange(Tmax)[None, :] >= live[:, None]
    assert (y[pad] == 0).all()
    assert np.array_equal(st, st_m) and (st == 0).all()
    assert (rep[live == 0] == 0).all()
    tol = C.tolerance(y_m, dtype)
    print("kernel text against the float64 model: %.3g of the bound" % (np.abs(y.astype(np.float64) - y_m).max() / max(tol, 1e-300)))
    assert np.abs(y.astype(np.float64) - y_m).max() <= tol
    scale = np.abs(rep_m).max(axis=(0, 1)) + 1e-300
    assert (np.abs(rep - rep_m) <= 64 * C.BOUND_RATIO * C.EPS * scale).all()
    assert np.abs(gv - GV.gv_padded(y, lengths)).max() <= 4 * Tmax * C.EPS * max(np.abs(y).max() ** 2, 1e-300)
    if n_iter == 100 and dtype == np.float64:
        # the measurement behind the tolerance: against the model in long double
        y_ld = C.model(case, n_iter, work=np.longdouble)[0]
        ratio = float(np.abs(y - y_ld).max() / (C.EPS * np.abs(y_ld).max()))
        print("against long double: %.2f eps max|y| (recorded worst %.2f, bound %.0f)" % (ratio, C.WORST_RATIO, C.BOUND_RATIO))
        assert ratio <= C.WORST_RATIO


def test_explicit_step_and_unscaled_start(program):
    case = C.make_case(5, 2, 70, 2, "std2", GV.VAR_FRAME, np.float64, [70, 33])
    for kw in (dict(init=0), dict(step=0.37), dict(init=0, step=0.11, omega_scale=2.5)):
        y, rep, st, _ = run_host(program, case, 7, step=kw.get("step"), init=kw.get("init", 1), omega_scale=kw.get("omega_scale", 1.0))
        y_m, rep_m, st_m = C.model(case, 7, **kw)
        assert np.abs(y - y_m).max() <= C.tolerance(y_m, np.float64) and np.array_equal(st, st_m)
    # a step far too large: no ascent, or overflow
    big = 50 * max(1.0 / (case["gv_prec"].min() * 1e-6), 1e6)
    st = run_host(program, case, 100, step=big)[2]
    assert np.isin(st, (1, 2)).all()
