"""CPU-side checks of the nnmk_sil_* entry points and of their Python layers (-m "not gpu"): the symbols against the header's
prototypes and #defines, the other headers free of the prefix, the extension header as C99 -pedantic and a C program linked
against the library, every refusal answered with fake pointers before the runtime is touched and with no counter moving, the
Python layers' ValueErrors raised before any device work, and no fallback for the device route."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import silence_cases as SC
from silence_cases import SM

ROOT = SC.ROOT
NAMES = ("nnmk_sil_abi_version", "nnmk_sil_frame_counts", "nnmk_sil_expand", "nnmk_sil_gather", "nnmk_sil_launch_count")
fake = ctypes.c_void_p(64)
fake2 = ctypes.c_void_p(4096)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _frontend_hip, _silence_hip
    _frontend_hip.lib()
    return _silence_hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(44)] + [L.nnmk_frontend_launch_count(), L.nnmk_sil_launch_count()]


def expand(L, device=0, dtype_phone=0, phone=fake, ld_phone=416, dtype_dur=2, durations=fake, num_phones=fake, silence=fake, B=2, Nmax=7, S=5,
           Dl=416, min_frames=0, kind=1, cc=None, scale_=None, min_=None, dtype_out=0, out=fake, ld_out=425, Tcap=100, lengths_out=fake):
    return L.nnmk_sil_expand(device, None, dtype_phone, phone, ld_phone, dtype_dur, durations, num_phones, silence, B, Nmax, S, Dl, min_frames,
                             kind, cc, scale_, min_, dtype_out, out, ld_out, Tcap, lengths_out)


def gather(L, device=0, dtype_dur=2, durations=fake, num_phones=fake, silence=fake, B=2, Nmax=7, S=5, min_frames=0, dtype_src=0, src=fake,
           ld_src=60, len_src=fake, Tmax=120, D=60, dtype_out=0, out=fake2, ld_out=60, Tcap=100, lengths_out=fake):
    return L.nnmk_sil_gather(device, None, dtype_dur, durations, num_phones, silence, B, Nmax, S, min_frames, dtype_src, src, ld_src, len_src,
                             Tmax, D, dtype_out, out, ld_out, Tcap, lengths_out)


def counts(L, device=0, dtype_dur=2, durations=fake, num_phones=fake, silence=fake, B=2, Nmax=7, S=5, min_frames=0, out=fake):
    return L.nnmk_sil_frame_counts(device, None, dtype_dur, durations, num_phones, silence, B, Nmax, S, min_frames, out)


def test_symbols_header_and_the_untouched_surfaces(L):
    from nnmnkwii_amd import _frontend_hip as FH, _hip, _silence_hip as SH
    for name in NAMES:
        assert getattr(L, name) is not None and name not in _hip.EXPORTS
    assert SH.NAMES == NAMES and L.nnmk_sil_abi_version() == 1 == SH.ABI_VERSION
    assert len(_hip.EXPORTS) == 61 and L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION and L.nnmk_frontend_abi_version() == 1
    assert L.nnmk_sil_launch_count() >= 0
    header = open(os.path.join(ROOT, "include", "nnmnkwii_silence.h")).read()
    assert set(re.findall(r"\b(nnmk_sil_\w+)\s*\(", header)) == set(NAMES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+NNMK_SIL_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(ABI_VERSION=SH.ABI_VERSION, BLOCK_ROWS=SH.BLOCK_ROWS) and SH.BLOCK_ROWS == SM.BLOCK_ROWS == FH.BLOCK_ROWS
    # the prototypes' argument counts are the binding's
    for name in NAMES:
        proto = re.search(r"^(?:int|long long) %s\(([^)]*)\);" % name, header, re.M).group(1)
        nargs = 0 if proto.strip() == "void" else proto.count(",") + 1
        assert len(getattr(L, name).argtypes) == nargs, name
    # no other header, and nothing of the main surface, knows the prefix
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "nnmnkwii_silence.h":
            text = open(os.path.join(ROOT, "include", other)).read().lower()
            assert "nnmk_sil" not in text and "nnmnkwii_silence" not in text, other
    assert not any("sil" in n for n in _hip.EXPORTS) and not any("sil" in n for n in FH.NAMES)
    keep = open(os.path.join(ROOT, "nnmnkwii_amd", "csrc", "frame_keep.hip")).read()
    assert '#include "common.h"' in keep and "nnmnkwii_silence.h" in keep and "frame_expand" not in re.sub(r"//[^\n]*", "", keep)


def test_header_is_c99_and_a_c_program_links(L, tmp_path):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.csrc import build as hip_build
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "main.c"
    src.write_text('#include "nnmnkwii_silence.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   '  printf("%d %d %d %lld\\n", nnmk_sil_abi_version(), NNMK_SIL_ABI_VERSION, NNMK_SIL_BLOCK_ROWS, nnmk_sil_launch_count());\n'
                   "  if (nnmk_sil_frame_counts(0, 0, 7, 0, 0, 0, 0, 0, 1, 0, 0) != -1) return 1;\n"
                   "  if (nnmk_sil_gather(0, 0, NNMK_FRONTEND_I32, 0, 0, 0, 0, 0, 1, 0, 5, 0, 0, 0, 0, 0, NNMK_FRONTEND_F32, 0, 0, 0, 0) != -1) return 2;\n"
                   "  return nnmk_sil_expand(0, 0, NNMK_FRONTEND_F32, 0, 0, 7, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, NNMK_FRONTEND_F32, 0, 0, 0, 0) != -1;\n}\n")
    exe = str(tmp_path / "main")
    so_dir = os.path.dirname(_hip.SO_PATH)
    r = subprocess.run([clang, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", so_dir, "-l:libmlpg_hip.so", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "1", "64", "0"], (r.stdout, r.stderr[-2000:])


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    common = [dict(dtype_dur=4), dict(dtype_dur=-1), dict(B=-1), dict(Nmax=-1), dict(min_frames=-1), dict(S=0), dict(S=9), dict(S=-1),
              dict(Nmax=8193, S=1), dict(Nmax=1025, S=8), dict(Nmax=1 << 30, S=8), dict(durations=None), dict(silence=None),
              dict(device=16), dict(device=-1)]
    for kw in common + [dict(out=None), dict(B=1 << 24)]:
        rc = counts(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"silence:"), (kw, rc, L.mlpg_hip_last_error())
    for kw in common + [dict(dtype_phone=2), dict(dtype_phone=-1), dict(dtype_out=2), dict(dtype_out=-1), dict(kind=8), dict(kind=-1),
                        dict(Dl=-1, ld_phone=0), dict(Tcap=-1), dict(ld_phone=415), dict(ld_phone=-1), dict(ld_out=424), dict(ld_out=-1),
                        dict(kind=0, ld_out=415), dict(kind=6, ld_out=420, cc=None), dict(scale_=fake), dict(min_=fake), dict(phone=None),
                        dict(out=None), dict(lengths_out=None), dict(B=1 << 24, Tcap=1), dict(B=1 << 20, Tcap=1 << 20)]:
        rc = expand(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"silence:"), (kw, rc, L.mlpg_hip_last_error())
    for kw in common + [dict(dtype_src=2), dict(dtype_src=-1), dict(dtype_out=3), dict(dtype_out=-1), dict(Tmax=-1), dict(D=-1, ld_src=0, ld_out=0),
                        dict(Tcap=-1), dict(ld_src=59), dict(ld_out=59), dict(ld_src=-1), dict(src=None), dict(out=None), dict(lengths_out=None),
                        dict(out=fake), dict(Tmax=(1 << 31) - 1), dict(B=1 << 24, Tcap=1), dict(B=1 << 20, Tcap=1 << 20)]:
        rc = gather(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"silence:"), (kw, rc, L.mlpg_hip_last_error())
    assert gather(L, out=fake) == -1 and b"out == src" in L.mlpg_hip_last_error()
    assert gather(L, ld_out=59) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert gather(L, B=1 << 24, Tcap=1) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert expand(L, ld_out=424) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert expand(L, S=9) == -1 and b"1 .. 8" in L.mlpg_hip_last_error()
    assert expand(L, kind=8) == -1 and b"unknown kind" in L.mlpg_hip_last_error()
    assert expand(L, kind=6, ld_out=420) == -1 and b"table" in L.mlpg_hip_last_error()
    assert expand(L, scale_=fake) == -1 and b"go together" in L.mlpg_hip_last_error()
    assert expand(L, silence=None) == -1 and b"NULL silence" in L.mlpg_hip_last_error()
    assert expand(L, B=1 << 24, Tcap=1) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert expand(L, Nmax=8193, S=1) == -1 and b"states" in L.mlpg_hip_last_error() and b"8192" in L.mlpg_hip_last_error()
    # the cap itself passes the size checks (the call is then refused for its device, the check behind them)
    assert expand(L, Nmax=8192, S=1, device=16) == -1 and b"states" not in L.mlpg_hip_last_error()
    assert gather(L, Nmax=1024, S=8, device=16) == -1 and b"states" not in L.mlpg_hip_last_error()
    # an empty batch is still checked
    assert expand(L, B=0, kind=8) == -1 and expand(L, B=0, device=16) == -1 and gather(L, B=0, S=0) == -1 and counts(L, B=0, dtype_dur=9) == -1
    assert _counts(L) == c0


def test_python_layers_raise_value_errors_before_any_device_work():
    import torch
    from nnmnkwii_amd import preprocessing as PP
    from nnmnkwii_amd.frontend import merlin as fe
    P, d, sil = np.zeros((4, 6)), np.ones((4, 5), dtype=np.int64), np.array([1, 0, 0, 1], dtype=bool)
    bad = [dict(a=(P, d, sil[:3]), kw={}, match="one bool or integer flag per phone"),
           dict(a=(P, d, sil.astype(np.float64)), kw={}, match="one bool or integer flag per phone"),
           dict(a=(P, d, sil[None]), kw={}, match="one bool or integer flag per phone"),
           dict(a=(P, d, sil), kw=dict(subphone_features="phoneme"), match="Unknown value"),
           dict(a=(P, d[:3], sil), kw={}, match=r"\(N, Dl\) and \(N, S\)"),
           dict(a=(P, np.ones((4, 9)), sil), kw={}, match="1 .. 8"),
           dict(a=(P, d, sil), kw=dict(min_frames=-1), match="min_frames"),
           dict(a=(P, d, sil), kw=dict(scale_=np.ones(15)), match="go together"),
           dict(a=(P, d, sil), kw=dict(dtype=np.int32), match="dtype must be")]
    for case in bad:
        with pytest.raises(ValueError, match=case["match"]):
            fe.kept_frame_features(*case["a"], **case["kw"])
        with pytest.raises(ValueError, match=case["match"].replace(r"\(N, Dl\) and \(N, S\)", "Nmax")):
            fe.kept_frame_features_batch(*(x[None] for x in case["a"]), **case["kw"])
        with pytest.raises(ValueError):
            fe.kept_frame_features(*(torch.from_numpy(x) for x in case["a"]), **case["kw"])
    with pytest.raises(ValueError, match="Tmax = 20 but out has 30"):
        fe.kept_frame_features_batch(P[None], d[None], sil[None], Tmax=20, out=torch.empty((1, 30, 15), device="meta"))
    with pytest.raises(ValueError, match="CUDA"):
        fe.kept_frame_features_batch(P[None], d[None], sil[None], out=torch.empty((1, 30, 15)))
    y = np.zeros((30, 3))
    bad = [dict(a=(y, d, sil[:3]), kw={}, match="one bool or integer flag per phone"),
           dict(a=(y[0], d, sil), kw={}, match=r"\(T, D\) and \(N, S\)"),
           dict(a=(y.astype(np.int32), d, sil), kw={}, match="float32 or float64"),
           dict(a=(y, d.astype(bool), sil), kw={}, match="durations must be"),
           dict(a=(y, np.ones((4, 9)), sil), kw={}, match="1 .. 8"),
           dict(a=(y, np.ones((8193, 1)), np.zeros(8193, bool)), kw={}, match="8192"),
           dict(a=(y, d, sil), kw=dict(min_frames=-1), match="min_frames")]
    for case in bad:
        with pytest.raises(ValueError, match=case["match"]):
            PP.remove_silence_frames(*case["a"], **case["kw"])
        with pytest.raises(ValueError, match=case["match"].replace(r"\(T, D\) and \(N, S\)", "Nmax")):
            PP.remove_silence_frames_batch(*(x[None] for x in case["a"]), **case["kw"])
    Y, D3, S2 = y[None], d[None], sil[None]
    with pytest.raises(ValueError, match="lengths must have one entry per utterance"):
        PP.remove_silence_frames_batch(Y, D3, S2, np.array([3, 3]))
    with pytest.raises(ValueError, match="num_phones must have one entry per utterance"):
        PP.remove_silence_frames_batch(Y, D3, S2, None, np.array([3, 3]))
    with pytest.raises(ValueError, match="Tmax"):
        PP.remove_silence_frames_batch(Y, D3, S2, Tmax=-1)
    with pytest.raises(ValueError, match="dtype must be"):
        PP.remove_silence_frames_batch(Y, D3, S2, dtype=np.int16)
    with pytest.raises(ValueError, match="out has 4 columns, the matrix has 3"):
        PP.remove_silence_frames_batch(Y, D3, S2, out=torch.empty((1, 30, 4), device="meta"))
    with pytest.raises(ValueError, match="Tmax = 20 but out has 30"):
        PP.remove_silence_frames_batch(Y, D3, S2, Tmax=20, out=torch.empty((1, 30, 3), device="meta"))
    with pytest.raises(ValueError, match="CUDA"):
        PP.remove_silence_frames_batch(Y, D3, S2, out=torch.empty((1, 30, 3)))
    Ym = torch.empty((1, 30, 3), device="meta")
    with pytest.raises(ValueError, match="must not be the matrix itself"):
        PP.remove_silence_frames_batch(Ym, D3, S2, out=Ym)
    # the interface
    assert list(inspect.signature(PP.remove_silence_frames_batch).parameters) == ["Y", "durations", "silence", "lengths", "num_phones", "min_frames",
                                                                                  "Tmax", "out", "dtype", "strict"]
    assert list(inspect.signature(PP.remove_silence_frames).parameters) == ["y", "durations", "silence", "min_frames"]
    kinds = {n: p.kind for n, p in inspect.signature(PP.remove_silence_frames_batch).parameters.items()}
    assert all(kinds[n] == inspect.Parameter.KEYWORD_ONLY for n in ("min_frames", "Tmax", "out", "dtype", "strict"))
    assert list(inspect.signature(fe.kept_frame_features_batch).parameters) == ["phone_features", "durations", "silence", "num_phones",
                                                                                 "subphone_features", "min_frames", "scale_", "min_", "Tmax", "out",
                                                                                 "dtype", "strict"]
    assert list(inspect.signature(fe.kept_frame_features).parameters) == ["phone_features", "durations", "silence", "subphone_features", "min_frames",
                                                                           "scale_", "min_", "dtype"]
    for f in (fe.kept_frame_features_batch, fe.kept_frame_features, PP.remove_silence_frames_batch, PP.remove_silence_frames):
        assert "silence_phone_indices(regex)] = True" in f.__doc__
    import nnmnkwii_amd
    assert "nnmnkwii_silence.h" in nnmnkwii_amd.__doc__


def test_binding_checks_its_tensors_without_a_device():
    import torch
    from nnmnkwii_amd import _silence_hip as SH
    d, s = torch.ones((2, 4, 5), dtype=torch.int32), torch.zeros((2, 4), dtype=torch.bool)
    with pytest.raises(ValueError, match="CUDA"):
        SH.frame_counts(d, None, s)
    with pytest.raises(ValueError, match="CUDA"):
        SH.expand(torch.zeros((2, 4, 3)), d, None, s, 1, 0, None, None, None, torch.zeros((2, 9, 12)))
    with pytest.raises(ValueError, match="CUDA"):
        SH.gather(torch.zeros((2, 9, 3)), None, d, None, s, 0, torch.zeros((2, 9, 3)))


def test_no_fallback_for_the_device_route():
    import torch
    if torch.cuda.is_available():
        return                      # (with a device the route runs: tests/test_silence_gpu.py)
    from nnmnkwii_amd import HipExtensionError, preprocessing as PP
    from nnmnkwii_amd.frontend import merlin as fe
    P, d, sil = np.zeros((4, 6)), np.ones((4, 5), dtype=np.int64), np.array([1, 0, 0, 1], dtype=bool)
    with pytest.raises(HipExtensionError):
        fe.kept_frame_features(P, d, sil)
    with pytest.raises(HipExtensionError):
        PP.remove_silence_frames(np.zeros((20, 3)), d, sil)
    with pytest.raises(HipExtensionError):
        PP.remove_silence_frames_batch(torch.zeros((1, 20, 3)), torch.from_numpy(d)[None], torch.from_numpy(sil)[None], Tmax=30, strict=False)
