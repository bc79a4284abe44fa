"""The text of csrc/gmm_traj.hip run on the CPU (-m "not gpu"): the file is compiled for the host against the shim
tests/gmm_host/common.h plus tests/gmmtraj_host/extras.h (the ballot and the first-lane read) into a stand-alone program under
the address and undefined-behaviour sanitizers, run as a child process, and compared with tools/gmmtraj_model.py.  This checks the
index arithmetic, the label loop, the masking of partial tiles, column tails and row strides and every bound of an array; it
cannot check that the hardware's lane maps are the documented ones (tests/test_gmmtraj_gpu.py does).  Nothing is loaded into
Python under a sanitizer.  Bound: 2 (D + 4) eps S per element (the GPU test's)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gmmtraj_model as GM  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from nnmnkwii_amd.csrc import build as hip_build
    d = tmp_path_factory.mktemp("gmmtraj_host")
    src = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "gmm_traj.hip")).read()
    marker = "extern __shared__ double lds[];"
    assert src.count(marker) == 1
    (d / "gmm_traj_host.inc").write_text(src.replace(marker, "double *lds = g_dyn_lds;"))
    for sub, name in (("gmm_host", "common.h"), ("gmmtraj_host", "extras.h"), ("gmmtraj_host", "main.cpp")):
        (d / name).write_text(open(os.path.join(ROOT, "tests", sub, name)).read())
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "gmmtraj_host")
    r = subprocess.run([clang, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-ffp-contract=off", "-pthread", "-Wno-psabi", "-I", str(d), str(d / "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


CASES = [(1, 1, 1, 1, None), (1, 63, 3, 2, None), (1, 65, 17, 5, None), (3, 43, 6, 64, [43, 0, 17]), (3, 43, 6, 64, [0, 42, 1]),
         (2, 70, 128, 3, [70, 5])]


@pytest.mark.parametrize("B,T,D,M,lengths", CASES)
@pytest.mark.parametrize("wide", [False, True])
def test_kernel_text_on_the_host(program, B, T, D, M, lengths, wide):
    d, exe = program
    rng = np.random.RandomState(B + T + D + M)
    ld_x, ld_o = (2 * D, D + 3) if wide else (D, D)
    mu_x, mu_y = rng.randn(M, D), rng.randn(M, D)
    A = rng.randn(M, D, D) / np.sqrt(D)
    cvar = rng.rand(M, D) + 0.1
    xw = rng.randn(B, T, ld_x)
    labels = rng.randint(M, size=(B, T)).astype(np.int32)
    live = np.arange(T)[None] < GM.live_frames(lengths, B, T)[:, None]
    labels[~live] = np.where(rng.rand((~live).sum()) < 0.5, -7, M + 9)     # pad rows' labels are not read
    xw[~live] = np.nan                                                     # nor is their x
    if live.sum() > 3:                                                     # one live row with a bad label
        b, t = np.argwhere(live)[len(np.argwhere(live)) // 2]
        labels[b, t] = M
    with open(d / "in.bin", "wb") as f:
        f.write(np.array([B, T, D, M, ld_x, ld_o, lengths is not None], dtype=np.int64).tobytes())
        f.write(np.asarray(lengths if lengths is not None else [0] * B, dtype=np.int32).tobytes())
        f.write(labels.tobytes())
        for a in (xw, mu_x, mu_y, A, cvar):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.fromfile(d / "out.bin").reshape(2, B, T, ld_o)
    assert (out[:, :, :, D:] == -7.0).all()                                # columns past D are untouched
    mean, var = out[0, :, :, :D], out[1, :, :, :D]
    x = xw[:, :, :D]
    mean_r, var_r = GM.stats_padded(x, lengths, labels, mu_x, mu_y, A, cvar)
    ok = live & (labels >= 0) & (labels < M)
    assert np.array_equal(np.isnan(mean), np.isnan(mean_r)) and np.array_equal(var, var_r, equal_nan=True)
    assert (mean[~live] == 0).all() and (var[~live] == 1).all()
    S = GM.error_scale(x[ok], labels[ok], mu_x, mu_y, A)
    ratio = (np.abs(mean[ok] - mean_r[ok]) / (2 * (D + 4) * EPS * S)).max() if ok.any() else 0.0
    print("means: %.3f of the bound" % ratio)
    assert ratio <= 1.0
