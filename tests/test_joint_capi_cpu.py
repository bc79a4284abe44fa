"""CPU-side checks of the nnmk_joint_* entry points and of nnmnkwii_amd.preprocessing.frames (-m "not gpu"): the symbols and the
version, the extension header as C99 -pedantic and a C program linked against the library, every refusal answered with fake
pointers before the runtime is touched and with no counter moving, nnmk_joint_workspace_bytes against the model, the untouched
mlpg_hip_* surface and the four other extension headers, the Python layer's errors raised before any device work, no fallback
without a GPU, and the compat routing with uninstall() restoring everything."""
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
import joint_model as JM  # noqa: E402

NAMES = ("nnmk_joint_abi_version", "nnmk_joint_workspace_bytes", "nnmk_joint_count", "nnmk_joint_write", "nnmk_joint_launch_count")
fake = ctypes.c_void_p(64)
WL, WU = np.array([0, 1, 1], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)
WC = np.array([1.0, -0.5, 0.0, 0.5, 1.0, -2.0, 1.0])


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _f0_hip, _frontend_hip, _joint_hip, _metrics_hip, _wave_hip
    for m in (_metrics_hip, _frontend_hip, _f0_hip, _wave_hip):
        m.lib()
    return _joint_hip.lib()


def _counts(L):
    return ([L.mlpg_hip_launch_count(k) for k in range(44)]
            + [L.nnmk_metrics_launch_count(), L.nnmk_frontend_launch_count(), L.nnmk_f0_launch_count(), L.nnmk_joint_launch_count()])


def _src(kw):
    d = dict(device=0, dtype_x=0, x=fake, ld_x=60, len_x=fake, Dx=59, dtype_y=1, y=fake, ld_y=60, len_y=fake, Dy=59, B=2, Tmax=100, nw=3,
             wl=WL, wu=WU, wc=WC)
    d.update({k: v for k, v in kw.items() if k in d})
    p = [None if d[k] is None else d[k].ctypes.data for k in ("wl", "wu", "wc")]
    return [d["device"], None, d["dtype_x"], d["x"], d["ld_x"], d["len_x"], d["Dx"], d["dtype_y"], d["y"], d["ld_y"], d["len_y"], d["Dy"], d["B"],
            d["Tmax"], d["nw"]] + p


def count(L, **kw):
    d = dict(keep=0, eps=1e-7, dtype_out=1, ws=fake, ws_bytes=1 << 20, offsets=fake)
    d.update({k: v for k, v in kw.items() if k in d})
    return L.nnmk_joint_count(*_src(kw), d["keep"], d["eps"], d["dtype_out"], d["ws"], d["ws_bytes"], d["offsets"])


def write(L, **kw):
    d = dict(ws=fake, ws_bytes=1 << 20, dtype_out=1, out=fake, ld_out=354, cap=10)
    d.update({k: v for k, v in kw.items() if k in d})
    return L.nnmk_joint_write(*_src(kw), d["ws"], d["ws_bytes"], d["dtype_out"], d["out"], d["ld_out"], d["cap"])


def test_symbols_version_and_the_untouched_surfaces(L):
    from nnmnkwii_amd import _f0_hip, _frontend_hip, _hip, _joint_hip as JH, _metrics_hip, _wave_hip
    for name in NAMES:
        assert getattr(L, name) is not None and name not in _hip.EXPORTS
    assert JH.NAMES == NAMES and L.nnmk_joint_abi_version() == 1 == JH.ABI_VERSION
    assert (JH.TILE, JH.NONZERO, JH.LIVE, JH.MAX_WINDOWS, JH.MAX_EXTENT) == (JM.TILE, JM.NONZERO, JM.LIVE, JM.MAX_WINDOWS, JM.MAX_EXTENT)
    assert not any(n.startswith("nnmk_") for n in _hip.EXPORTS)
    assert len(_hip.EXPORTS) == 61 and L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert [L.mlpg_hip_launch_count(k) for k in (42, 43)] == [-1, -1] and L.nnmk_joint_launch_count() >= 0
    assert L.nnmk_metrics_abi_version() == 1 == _metrics_hip.ABI_VERSION and L.nnmk_frontend_abi_version() == 1 == _frontend_hip.ABI_VERSION
    assert L.nnmk_f0_abi_version() == 1 == _f0_hip.ABI_VERSION and L.nnmk_wave_abi_version() == _wave_hip.ABI_VERSION == 1
    assert "nnmk_" not in open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for other in ("nnmnkwii_metrics.h", "nnmnkwii_frontend.h", "nnmnkwii_f0.h", "nnmnkwii_wave.h"):
        assert "nnmk_joint" not in open(os.path.join(ROOT, "include", other)).read()
    header = open(os.path.join(ROOT, "include", "nnmnkwii_joint.h")).read()
    assert set(re.findall(r"\b(nnmk_joint_\w+)\s*\(", header)) == set(NAMES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+NNMK_JOINT_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(ABI_VERSION=JH.ABI_VERSION, F32=JH.F32, F64=JH.F64, NONZERO=JH.NONZERO, LIVE=JH.LIVE, TILE=JH.TILE,
                        MAX_WINDOWS=JH.MAX_WINDOWS, MAX_EXTENT=JH.MAX_EXTENT)


def test_header_is_c99_and_a_c_program_links(L, tmp_path):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.csrc import build as hip_build
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "main.c"
    src.write_text('#include "nnmnkwii_joint.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   '  printf("%d %d %lld %lld\\n", nnmk_joint_abi_version(), NNMK_JOINT_TILE, (long long)nnmk_joint_workspace_bytes(3, 131),\n'
                   "         nnmk_joint_launch_count());\n"
                   "  if (nnmk_joint_write(0, 0, NNMK_JOINT_F32, 0, 0, 0, 0, NNMK_JOINT_F32, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, NNMK_JOINT_F64, 0, 0, -1) != -1)\n"
                   "    return 1;\n"
                   "  return nnmk_joint_count(0, 0, NNMK_JOINT_F32, 0, 0, 0, 0, NNMK_JOINT_F32, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0.0, NNMK_JOINT_F64, 0, 0, 0) != -1;\n}\n")
    exe = str(tmp_path / "main")
    so_dir = os.path.dirname(_hip.SO_PATH)
    r = subprocess.run([clang, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", so_dir, "-l:libmlpg_hip.so", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "64", "144", "0"], (r.stdout, r.stderr[-2000:])


def test_workspace_bytes_against_the_model(L):
    for B, Tmax in ((0, 0), (1, 1), (1, 63), (1, 64), (1, 65), (3, 131), (70, 131), (512, 2000), (-1, 5), (5, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert L.nnmk_joint_workspace_bytes(B, Tmax) == JM.workspace_bytes(B, Tmax), (B, Tmax)


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    big = np.array([0, 9, 1], dtype=np.int32)
    neg = np.array([0, -1, 1], dtype=np.int32)
    shared = [dict(dtype_x=2), dict(dtype_x=-1), dict(dtype_y=2), dict(dtype_out=2), dict(dtype_out=-1), dict(B=-1), dict(Tmax=-1), dict(Dx=-1),
              dict(Dy=-1), dict(ld_x=58), dict(ld_y=0), dict(nw=9), dict(nw=-1), dict(wl=big), dict(wu=big), dict(wl=neg), dict(wu=neg),
              dict(wl=None), dict(wc=None), dict(x=None), dict(y=None), dict(ws=None), dict(ws=ctypes.c_void_p(68)), dict(ws_bytes=16 * 2 * 2 - 1),
              dict(device=16), dict(device=-1)]
    for kw in shared + [dict(keep=2), dict(keep=-1), dict(eps=-1e-300), dict(eps=float("nan")), dict(offsets=None)]:
        rc = count(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"joint:"), ("count", kw, rc, L.mlpg_hip_last_error())
    for kw in shared + [dict(cap=-1), dict(ld_out=353), dict(out=None)]:
        rc = write(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"joint:"), ("write", kw, rc, L.mlpg_hip_last_error())
    assert count(L, dtype_y=2) == -1 and b"dtype" in L.mlpg_hip_last_error()
    assert count(L, keep=2) == -1 and b"keep mode" in L.mlpg_hip_last_error()
    assert count(L, Tmax=-1) == -1 and b"negative size" in L.mlpg_hip_last_error()
    assert write(L, ld_out=353) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert count(L, nw=9) == -1 and b"num_windows" in L.mlpg_hip_last_error()
    assert count(L, wu=big) == -1 and b"outside [0, 8]" in L.mlpg_hip_last_error()
    assert count(L, eps=-1.0) == -1 and b"eps" in L.mlpg_hip_last_error()
    assert count(L, ws_bytes=63) == -1 and b"workspace" in L.mlpg_hip_last_error()
    assert write(L, cap=-1) == -1 and b"cap" in L.mlpg_hip_last_error()
    assert count(L, device=16) == -1 and b"device" in L.mlpg_hip_last_error()
    # without a y (Dy == 0) its dtype, pointer, stride and lengths are not looked at
    assert count(L, Dy=0, dtype_y=7, y=None, len_y=None, ld_y=0, device=16) == -1 and b"device" in L.mlpg_hip_last_error()
    # an empty batch is still checked, then launches nothing and returns 0 (the pointers are never looked at)
    assert count(L, B=0, keep=7) == -1 and count(L, B=0, device=16) == -1 and write(L, Tmax=0, cap=-1) == -1
    for kw in (dict(B=0), dict(B=0, x=None, y=None, ws=None, offsets=None, ws_bytes=0)):
        assert count(L, **kw) == 0, kw
    for kw in (dict(B=0), dict(Tmax=0, ws_bytes=0), dict(Dx=0, Dy=0, ld_out=0), dict(cap=0), dict(B=0, x=None, y=None, ws=None, out=None)):
        assert write(L, **kw) == 0, kw
    assert _counts(L) == c0


def test_python_layer_raises_before_any_device_work():
    import torch
    from nnmnkwii_amd import preprocessing as P
    from nnmnkwii_amd.preprocessing import frames as PF
    assert P.remove_zeros_frames is PF.remove_zeros_frames and P.remove_zeros_frames_batch is PF.remove_zeros_frames_batch
    assert P.joint_features_batch is PF.joint_features_batch
    X, Y = np.zeros((2, 5, 3)), np.zeros((2, 5, 4))
    for bad in (np.zeros(5), np.zeros((2, 2, 2)), torch.zeros(3)):
        with pytest.raises(ValueError, match=r"must be \(T, D\)"):
            P.remove_zeros_frames(bad)
    for bad in (np.zeros((4, 2)), np.zeros((1, 2, 3, 4))):
        with pytest.raises(ValueError, match=r"must be \(B, Tmax, D\)"):
            P.remove_zeros_frames_batch(bad)
        with pytest.raises(ValueError, match=r"must be \(B, Tmax, D\)"):
            P.joint_features_batch(X, bad, None)
    with pytest.raises(ValueError, match="share B and Tmax"):
        P.joint_features_batch(X, np.zeros((2, 6, 3)), None)
    with pytest.raises(ValueError, match="both be numpy arrays or both be tensors"):
        P.joint_features_batch(X, torch.zeros((2, 5, 3)), None)
    for lengths in (np.array([2.0, 3.0]), np.array([1, 2, 3]), [[1, 2]], torch.tensor([1.0, 2.0]), (np.array([1, 2]), np.array([1, 2, 3]))):
        with pytest.raises(ValueError, match="one integer per utterance"):
            P.joint_features_batch(X, Y, lengths)
    with pytest.raises(ValueError, match="pair of lengths goes with two sources"):
        P.remove_zeros_frames_batch(X, (np.array([1, 2]), np.array([1, 2])))
    for eps in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="eps must be >= 0"):
            P.joint_features_batch(X, Y, None, eps=eps)
        with pytest.raises(ValueError, match="eps must be >= 0"):
            P.remove_zeros_frames(X[0], eps)
    with pytest.raises(ValueError, match="dtype must be float32 or float64"):
        P.joint_features_batch(X, Y, None, dtype=torch.int32)
    with pytest.raises(ValueError, match="at most 8 windows"):
        P.joint_features_batch(X, Y, None, [np.ones(1)] * 9)
    with pytest.raises(ValueError, match="0 <= l, u <= 8"):
        P.joint_features_batch(X, Y, None, [np.ones(19)])
    with pytest.raises(ValueError, match="for CUDA tensors"):
        P.joint_features_batch(X, Y, None, out=torch.empty((4, 7), dtype=torch.float64))
    with pytest.raises(ValueError, match="for CUDA tensors"):
        P.remove_zeros_frames_batch(torch.from_numpy(X), out=torch.empty((4, 3), dtype=torch.float64))
    Xm = torch.empty((2, 5, 3), device="meta")
    for out in (torch.empty((4, 6), device="meta", dtype=torch.float64), torch.empty((4, 7), device="meta", dtype=torch.float32), np.zeros((4, 7))):
        with pytest.raises(ValueError, match="for CUDA tensors|out must be a"):
            P.joint_features_batch(Xm, torch.empty((2, 5, 4), device="meta"), None, out=out)
    assert list(inspect.signature(P.remove_zeros_frames).parameters) == ["x", "eps"]
    assert inspect.signature(P.remove_zeros_frames).parameters["eps"].default == 1e-7
    assert list(inspect.signature(P.remove_zeros_frames_batch).parameters) == ["X", "lengths", "eps", "out", "return_offsets"]
    sig = inspect.signature(P.joint_features_batch)
    assert list(sig.parameters) == ["X", "Y", "lengths", "windows", "eps", "dtype", "out", "return_offsets"]
    assert sig.parameters["dtype"].default is torch.float64 and sig.parameters["eps"].default == 1e-7
    assert sig.parameters["eps"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["windows"].default is None


def test_binding_checks_its_tensors_without_a_device():
    import torch
    from nnmnkwii_amd import _joint_hip as JH
    x = torch.zeros((2, 9, 1))
    with pytest.raises(ValueError, match="CUDA"):
        JH.Plan(x, None, None, None, [], torch.float64)
    with pytest.raises(ValueError, match="at most 8 windows"):
        JH.pack_windows([(0, 0, np.ones(1))] * 9)


def test_aligner_refuses_mixed_inputs_before_any_device_work():
    import torch
    from nnmnkwii_amd.preprocessing.alignment import DTWAligner
    x = torch.zeros((2, 9, 3))
    with pytest.raises(ValueError, match="CUDA tensors"):
        DTWAligner().transform((x, x))
    with pytest.raises(ValueError, match="CUDA tensors"):
        DTWAligner().transform((x.numpy(), x))


def test_no_fallback_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError, preprocessing as P
    x = np.array([[0.0, 5.0], [0.0, 0.0], [1.0, 0.0]])
    with pytest.raises(HipExtensionError):
        P.remove_zeros_frames(x)
    with pytest.raises(HipExtensionError):
        P.remove_zeros_frames(torch.from_numpy(x))
    with pytest.raises(HipExtensionError):
        P.remove_zeros_frames_batch(x[None], [3], return_offsets=True)
    with pytest.raises(HipExtensionError):
        P.joint_features_batch(x[None], x[None], [3], [np.array([1.0]), np.array([-0.5, 0.0, 0.5])], eps=None)


def test_compat_routing_and_uninstall():
    from nnmnkwii_amd import compat, preprocessing as P
    names = ("nnmnkwii.preprocessing", "nnmnkwii.preprocessing.generic", "nnmnkwii.util")
    assert set(compat._ROUTES) == set(names)
    assert all(compat._ROUTES[m] == {"remove_zeros_frames": P.remove_zeros_frames} for m in names)
    assert "remove_zeros_frames" not in compat._SURFACE["nnmnkwii.preprocessing"]
    assert "remove_zeros_frames" not in compat._SURFACE["nnmnkwii.preprocessing.generic"] and set(compat._REEXPORTS) == {"nnmnkwii.preprocessing"}
    assert "remove_zeros_frames" not in compat._REEXPORTS["nnmnkwii.preprocessing"]
    import importlib
    before = {}
    for m in names:
        try:
            before[m] = getattr(importlib.import_module(m), "remove_zeros_frames", None)
        except Exception:
            before[m] = None
    had = {m: m in sys.modules for m in names}
    compat.install()
    try:
        for m in names:
            assert sys.modules[m].remove_zeros_frames is P.remove_zeros_frames, m
        assert sys.modules["nnmnkwii.preprocessing"].delta_features is P.delta_features
    finally:
        compat.uninstall()
    for m in names:
        if had[m]:
            assert getattr(sys.modules[m], "remove_zeros_frames", None) is before[m], m
        else:
            assert m not in sys.modules or getattr(sys.modules[m], "remove_zeros_frames", None) is not P.remove_zeros_frames, m
    assert not compat._saved and not compat._registered
