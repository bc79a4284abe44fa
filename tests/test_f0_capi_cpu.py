"""CPU-side checks of the nnmk_f0_* entry points and of nnmnkwii_amd.preprocessing.f0 (-m "not gpu"): the symbols and the
version, the extension header as C99 -pedantic and a C program linked against the library, every refusal answered with fake
pointers before the runtime is touched and with no counter moving, the untouched mlpg_hip_*, nnmk_metrics_* and nnmk_frontend_*
surfaces, the Python layer's errors raised before any device work, no fallback for the device route, and the compat surface."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import f0_model as F0  # noqa: E402

NAMES = ("nnmk_f0_abi_version", "nnmk_f0_interp", "nnmk_f0_launch_count")
fake = ctypes.c_void_p(64)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _f0_hip, _frontend_hip, _metrics_hip
    _metrics_hip.lib()
    _frontend_hip.lib()
    return _f0_hip.lib()


def _counts(L):
    return ([L.mlpg_hip_launch_count(k) for k in range(44)]
            + [L.nnmk_metrics_launch_count(), L.nnmk_frontend_launch_count(), L.nnmk_f0_launch_count()])


def interp(L, device=0, dtype_x=0, x=fake, ld_x=187, lengths=fake, B=2, Tmax=100, C=1, kind=0, dtype_y=0, y=fake, ld_y=187, dtype_vuv=0,
           vuv=fake, ld_vuv=187):
    return L.nnmk_f0_interp(device, None, dtype_x, x, ld_x, lengths, B, Tmax, C, kind, dtype_y, y, ld_y, dtype_vuv, vuv, ld_vuv)


def test_symbols_version_and_the_untouched_surfaces(L):
    from nnmnkwii_amd import _f0_hip as FH, _frontend_hip, _hip, _metrics_hip
    for name in NAMES:
        assert getattr(L, name) is not None and name not in _hip.EXPORTS
    assert FH.NAMES == NAMES and L.nnmk_f0_abi_version() == 1 == FH.ABI_VERSION
    assert FH.KINDS == F0.KINDS == ("slinear", "linear", "previous", "zero", "next", "nearest", "nearest-up") and FH.TILE == F0.TILE
    assert not any(n.startswith("nnmk_") for n in _hip.EXPORTS)
    assert len(_hip.EXPORTS) == 61 and L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert [L.mlpg_hip_launch_count(k) for k in (42, 43)] == [-1, -1] and L.nnmk_f0_launch_count() >= 0
    assert L.nnmk_metrics_abi_version() == 1 == _metrics_hip.ABI_VERSION
    assert L.nnmk_frontend_abi_version() == 1 == _frontend_hip.ABI_VERSION
    main_header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    assert "nnmk_" not in main_header
    for other in ("nnmnkwii_metrics.h", "nnmnkwii_frontend.h"):
        assert "nnmk_f0" not in open(os.path.join(ROOT, "include", other)).read()
    header = open(os.path.join(ROOT, "include", "nnmnkwii_f0.h")).read()
    assert set(re.findall(r"\b(nnmk_f0_\w+)\s*\(", header)) == set(NAMES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+NNMK_F0_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(ABI_VERSION=FH.ABI_VERSION, F32=FH.F32, F64=FH.F64, SLINEAR=0, LINEAR=1, PREVIOUS=2, ZERO=3, NEXT=4, NEAREST=5,
                        NEAREST_UP=6, TILE=FH.TILE)
    assert [FH.KINDS.index(k) for k in ("slinear", "zero", "nearest-up")] == [FH.SLINEAR, FH.ZERO, FH.NEAREST_UP]
    assert [F0.kind_of(k) for k in F0.KINDS] == list(range(7)) == [FH.kind_of(k) for k in FH.KINDS]


def test_header_is_c99_and_a_c_program_links(L, tmp_path):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.csrc import build as hip_build
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "main.c"
    src.write_text('#include "nnmnkwii_f0.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   '  printf("%d %d %lld\\n", nnmk_f0_abi_version(), NNMK_F0_TILE, nnmk_f0_launch_count());\n'
                   "  return nnmk_f0_interp(0, 0, NNMK_F0_F32, 0, 0, 0, 0, 0, 0, 7, NNMK_F0_F32, 0, 0, NNMK_F0_F32, 0, 0) != -1;\n}\n")
    exe = str(tmp_path / "main")
    so_dir = os.path.dirname(_hip.SO_PATH)
    r = subprocess.run([clang, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", so_dir, "-l:libmlpg_hip.so", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "256", "0"], (r.stdout, r.stderr[-2000:])


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(dtype_x=2), dict(dtype_x=-1), dict(dtype_y=2), dict(dtype_y=-1), dict(dtype_vuv=2), dict(dtype_vuv=-1),
             dict(kind=7), dict(kind=-1), dict(B=-1), dict(Tmax=-1), dict(C=-1, ld_x=0), dict(ld_x=0), dict(ld_x=-1), dict(C=3, ld_x=2),
             dict(ld_y=0), dict(C=3, ld_y=2), dict(ld_vuv=0), dict(C=3, ld_vuv=2), dict(x=None), dict(y=None, vuv=None),
             dict(device=16), dict(device=-1)]
    for kw in cases:
        rc = interp(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"f0:"), (kw, rc, L.mlpg_hip_last_error())
    assert interp(L, dtype_vuv=2) == -1 and b"dtype" in L.mlpg_hip_last_error()
    assert interp(L, kind=7) == -1 and b"unknown kind" in L.mlpg_hip_last_error()
    assert interp(L, Tmax=-1) == -1 and b"negative size" in L.mlpg_hip_last_error()
    assert interp(L, ld_y=0) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert interp(L, x=None) == -1 and b"NULL x" in L.mlpg_hip_last_error()
    assert interp(L, y=None, vuv=None) == -1 and b"both NULL" in L.mlpg_hip_last_error()
    assert interp(L, device=16) == -1 and b"device" in L.mlpg_hip_last_error()
    # an array that is not wanted needs no stride
    assert interp(L, y=None, ld_y=0, device=16) == -1 and b"device" in L.mlpg_hip_last_error()
    assert interp(L, vuv=None, ld_vuv=0, device=16) == -1 and b"device" in L.mlpg_hip_last_error()
    # an empty batch is still checked, then launches nothing and returns 0 (the pointers are never looked at)
    assert interp(L, B=0, kind=7) == -1 and interp(L, B=0, device=16) == -1 and interp(L, Tmax=0, y=None, vuv=None) == -1
    for kw in (dict(B=0), dict(Tmax=0), dict(C=0), dict(B=0, x=None, lengths=None)):
        assert interp(L, **kw) == 0, kw
    assert _counts(L) == c0


def test_python_layer_raises_before_any_device_work():
    import torch
    from nnmnkwii_amd import preprocessing as P
    from nnmnkwii_amd.preprocessing import f0 as PF
    assert P.interp1d is PF.interp1d and P.interp1d_batch is PF.interp1d_batch
    x = np.zeros(8)
    for kind in ("quadratic", "cubic", 1, None, "Slinear"):
        with pytest.raises(ValueError, match="kind must be one of"):
            P.interp1d(x, kind)
        with pytest.raises(ValueError, match="kind must be one of"):
            P.interp1d_batch(x.reshape(2, 4), kind=kind)
    for bad in (np.zeros((4, 2)), np.zeros((2, 2, 2)), np.zeros((1, 4)), torch.zeros((4, 2))):
        with pytest.raises(RuntimeError, match="1d array is only supported"):
            P.interp1d(bad)
    X = np.zeros((2, 5, 3))
    for bad in (np.zeros(5), np.zeros((1, 2, 3, 4))):
        with pytest.raises(ValueError, match=r"\(B, Tmax, C\) or \(B, Tmax\)"):
            P.interp1d_batch(bad)
    for lengths in (np.array([2.0, 3.0]), np.array([1, 2, 3]), [[1, 2]], torch.tensor([1.0, 2.0]), torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError, match="one integer per utterance"):
            P.interp1d_batch(X, lengths)
    # out / vuv: shape and dtype alone are looked at (a meta tensor has no memory)
    Xm = torch.empty((2, 5, 3), device="meta")
    for name in ("out", "vuv"):
        for t in (torch.empty((2, 5, 2), device="meta"), torch.empty((2, 5, 3), device="meta", dtype=torch.int32), np.zeros((2, 5, 3))):
            with pytest.raises(ValueError, match="%s must be a float32 / float64 CUDA tensor of X's shape" % name):
                P.interp1d_batch(Xm, **{name: t})
            with pytest.raises(ValueError, match="%s must be" % name):
                P.interp1d_batch(X, **{name: t})
    with pytest.raises(ValueError, match="for CUDA tensors"):
        P.interp1d_batch(X, out=torch.empty((2, 5, 3)))
    with pytest.raises(ValueError, match="for CUDA tensors"):
        P.interp1d_batch(torch.from_numpy(X), vuv=torch.empty((2, 5, 3)))
    assert list(inspect.signature(P.interp1d).parameters) == ["f0", "kind"]
    assert inspect.signature(P.interp1d).parameters["kind"].default == "slinear"
    assert list(inspect.signature(P.interp1d_batch).parameters) == ["X", "lengths", "kind", "out", "vuv", "return_vuv"]


def test_binding_checks_its_tensors_without_a_device():
    import torch
    from nnmnkwii_amd import _f0_hip as FH
    x = torch.zeros((2, 9, 1))
    with pytest.raises(ValueError, match="CUDA"):
        FH.interp(x, None, 0, x, None)


def test_no_fallback_for_the_device_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError, preprocessing as P, util
    x = np.array([0.0, 5.0, 0.0, 6.0, 0.0])
    with pytest.raises(HipExtensionError):
        P.interp1d(x)
    with pytest.raises(HipExtensionError):
        P.interp1d(torch.from_numpy(x)[:, None], "nearest")
    with pytest.raises(HipExtensionError):
        P.interp1d_batch(x[None, :, None], [5], return_vuv=True)
    with pytest.raises(HipExtensionError):
        util.apply_each2d_padded(P.interp1d, x[None, :, None], [5], "linear")


def test_compat_surface_is_additive():
    from nnmnkwii_amd import compat, preprocessing as P
    S = compat._SURFACE
    assert S["nnmnkwii.preprocessing"]["interp1d"] is P.interp1d and S["nnmnkwii.preprocessing.f0"] == {"interp1d": P.interp1d}
    assert set(S["nnmnkwii.preprocessing"]) == {"delta_features", "trim_zeros_frames", "modspec", "modphase", "inv_modspec", "modspec_smoothing",
                                                "interp1d"} | set(compat._NORM)
    compat.install()
    try:
        import nnmnkwii.preprocessing
        import nnmnkwii.preprocessing.f0
        assert nnmnkwii.preprocessing.interp1d is P.interp1d and nnmnkwii.preprocessing.f0.interp1d is P.interp1d
    finally:
        compat.uninstall()
