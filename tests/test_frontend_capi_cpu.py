"""CPU-side checks of the nnmk_frontend_* entry points and of nnmnkwii_amd.frontend.merlin (-m "not gpu"): the symbols, the
version and the feature sizes, the extension header as C99 -pedantic and a C program linked against the library, every refusal
answered with fake pointers before the runtime is touched and with no counter moving, the cap on the states of an utterance, the
untouched mlpg_hip_* and nnmk_metrics_* surfaces, the Python layer's ValueErrors raised before any device work, and no fallback
for the device route."""
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
import frontend_model as FM  # noqa: E402

NAMES = ("nnmk_frontend_abi_version", "nnmk_frontend_feature_size", "nnmk_frontend_frame_counts", "nnmk_frontend_expand",
         "nnmk_frontend_launch_count")
fake = ctypes.c_void_p(64)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _frontend_hip, _metrics_hip
    _metrics_hip.lib()
    return _frontend_hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(44)] + [L.nnmk_metrics_launch_count(), L.nnmk_frontend_launch_count()]


def expand(L, device=0, dtype_phone=0, phone=fake, ld_phone=416, dtype_dur=2, durations=fake, num_phones=fake, B=2, Nmax=7, S=5, Dl=416,
           min_frames=0, kind=1, cc=None, scale_=None, min_=None, dtype_out=0, out=fake, ld_out=425, Tmax=100, lengths_out=fake):
    return L.nnmk_frontend_expand(device, None, dtype_phone, phone, ld_phone, dtype_dur, durations, num_phones, B, Nmax, S, Dl, min_frames, kind,
                                  cc, scale_, min_, dtype_out, out, ld_out, Tmax, lengths_out)


def counts(L, device=0, dtype_dur=2, durations=fake, num_phones=fake, B=2, Nmax=7, S=5, min_frames=0, out=fake):
    return L.nnmk_frontend_frame_counts(device, None, dtype_dur, durations, num_phones, B, Nmax, S, min_frames, out)


def test_symbols_version_sizes_and_the_untouched_surfaces(L):
    from nnmnkwii_amd import _frontend_hip as FH, _hip, _metrics_hip as M
    for name in NAMES:
        assert getattr(L, name) is not None and name not in _hip.EXPORTS
    assert FH.NAMES == NAMES and L.nnmk_frontend_abi_version() == 1 == FH.ABI_VERSION
    assert [L.nnmk_frontend_feature_size(k) for k in range(-1, 9)] == [-1, 0, 9, 2, 1, 1, 2, 4, 3, -1]
    assert FH.SIZES == FM.SIZES == (0, 9, 2, 1, 1, 2, 4, 3) and FH.KINDS == FM.KINDS
    assert not any(n.startswith("nnmk_") for n in _hip.EXPORTS)
    assert len(_hip.EXPORTS) == 61 and L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert [L.mlpg_hip_launch_count(k) for k in (42, 43)] == [-1, -1] and L.nnmk_frontend_launch_count() >= 0
    assert L.nnmk_metrics_abi_version() == 1 == M.ABI_VERSION
    main_header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    metrics_header = open(os.path.join(ROOT, "include", "nnmnkwii_metrics.h")).read()
    assert "nnmk_" not in main_header and "frontend" not in metrics_header.lower()
    header = open(os.path.join(ROOT, "include", "nnmnkwii_frontend.h")).read()
    assert set(re.findall(r"\b(nnmk_frontend_\w+)\s*\(", header)) == set(NAMES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+NNMK_FRONTEND_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(ABI_VERSION=FH.ABI_VERSION, F32=FH.F32, F64=FH.F64, I32=FH.I32, I64=FH.I64, NONE=0, FULL=1, MINIMAL_FRAME=2, STATE_ONLY=3,
                        FRAME_ONLY=4, UNIFORM_STATE=5, COARSE_CODING=6, MINIMAL_PHONEME=7, MAX_S=FH.MAX_S, CC_POINTS=FH.CC_POINTS,
                        BLOCK_ROWS=FH.BLOCK_ROWS, MAX_STATES=FH.MAX_STATES)
    assert (FM.BLOCK_ROWS, FM.MAX_STATES, FM.MAX_S, FM.CC_POINTS) == (FH.BLOCK_ROWS, FH.MAX_STATES, FH.MAX_S, FH.CC_POINTS)
    assert FH.MAX_STATES >= 8192
    assert [FH.KINDS.index(k) for k in (None, "full", "coarse_coding", "minimal_phoneme")] == [FH.NONE, FH.FULL, FH.COARSE_CODING, FH.MINIMAL_PHONEME]


def test_header_is_c99_and_a_c_program_links(L, tmp_path):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.csrc import build as hip_build
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "main.c"
    src.write_text('#include "nnmnkwii_frontend.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   '  printf("%d %d %d %d %lld\\n", nnmk_frontend_abi_version(), nnmk_frontend_feature_size(NNMK_FRONTEND_FULL),\n'
                   "         nnmk_frontend_feature_size(NNMK_FRONTEND_COARSE_CODING), nnmk_frontend_feature_size(8), nnmk_frontend_launch_count());\n"
                   "  return nnmk_frontend_expand(0, 0, NNMK_FRONTEND_F32, 0, 0, 7, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, NNMK_FRONTEND_F32, 0, 0, 0, 0) != -1;\n}\n")
    exe = str(tmp_path / "main")
    so_dir = os.path.dirname(_hip.SO_PATH)
    r = subprocess.run([clang, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", so_dir, "-l:libmlpg_hip.so", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "9", "4", "-1", "0"], (r.stdout, r.stderr[-2000:])


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(dtype_phone=2), dict(dtype_phone=-1), dict(dtype_out=2), dict(dtype_out=-1), dict(dtype_dur=4), dict(dtype_dur=-1),
             dict(kind=8), dict(kind=-1), dict(B=-1), dict(Nmax=-1), dict(Dl=-1, ld_phone=0), dict(Tmax=-1), dict(min_frames=-1),
             dict(S=0), dict(S=9), dict(S=-1), dict(ld_phone=415), dict(ld_phone=-1), dict(ld_out=424), dict(ld_out=-1),
             dict(kind=0, ld_out=415), dict(kind=6, ld_out=420, cc=None), dict(scale_=fake), dict(min_=fake),
             dict(phone=None), dict(durations=None), dict(out=None), dict(lengths_out=None), dict(device=16), dict(device=-1),
             dict(B=1 << 24, Tmax=1), dict(B=1 << 20, Tmax=1 << 20), dict(Nmax=8193, S=1), dict(Nmax=1025, S=8), dict(Nmax=1 << 30, S=8)]
    for kw in cases:
        rc = expand(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"frontend:"), (kw, rc, L.mlpg_hip_last_error())
    assert expand(L, ld_out=424) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert expand(L, S=9) == -1 and b"1 .. 8" in L.mlpg_hip_last_error()
    assert expand(L, kind=8) == -1 and b"unknown kind" in L.mlpg_hip_last_error()
    assert expand(L, kind=6, ld_out=420) == -1 and b"table" in L.mlpg_hip_last_error()
    assert expand(L, scale_=fake) == -1 and b"go together" in L.mlpg_hip_last_error()
    assert expand(L, out=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    assert expand(L, B=1 << 24, Tmax=1) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert expand(L, dtype_dur=4) == -1 and b"dtype_dur" in L.mlpg_hip_last_error()
    # an empty batch is still checked
    assert expand(L, B=0, kind=8) == -1 and expand(L, B=0, device=16) == -1 and expand(L, B=0, S=0) == -1
    for kw in (dict(dtype_dur=4), dict(B=-1), dict(Nmax=-1), dict(S=0), dict(S=9), dict(min_frames=-1), dict(Nmax=8193, S=1), dict(device=16),
               dict(durations=None), dict(out=None), dict(B=1 << 24)):
        rc = counts(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"frontend:"), (kw, rc, L.mlpg_hip_last_error())
    assert _counts(L) == c0


def test_the_cap_and_the_cap_plus_one(L):
    """Nmax * S = NNMK_FRONTEND_MAX_STATES passes the size checks (the call is then refused for its device, the check behind them);
    one state more is refused for its size."""
    from nnmnkwii_amd import _frontend_hip as FH
    c0 = _counts(L)
    for Nmax, S in ((FH.MAX_STATES, 1), (FH.MAX_STATES // 8, 8)):
        assert expand(L, Nmax=Nmax, S=S, device=16) == -1 and b"device" in L.mlpg_hip_last_error() and b"states" not in L.mlpg_hip_last_error()
        assert counts(L, Nmax=Nmax, S=S, device=16) == -1 and b"states" not in L.mlpg_hip_last_error()
    for Nmax, S in ((FH.MAX_STATES + 1, 1), (FH.MAX_STATES // 8 + 1, 8)):
        assert expand(L, Nmax=Nmax, S=S, device=16) == -1 and b"states" in L.mlpg_hip_last_error() and b"8192" in L.mlpg_hip_last_error()
        assert counts(L, Nmax=Nmax, S=S, device=16) == -1 and b"states" in L.mlpg_hip_last_error()
    assert _counts(L) == c0


def test_python_layer_raises_value_errors_before_any_device_work():
    import torch
    from nnmnkwii_amd.frontend import merlin as fe
    assert [fe.get_frame_feature_size(k) for k in FM.KINDS] == list(FM.SIZES) and fe.get_frame_feature_size() == 9
    with pytest.raises(ValueError, match="deprecated"):
        fe.get_frame_feature_size("none")
    with pytest.raises(ValueError, match="Unknown value"):
        fe.get_frame_feature_size("phoneme")
    P, d = np.zeros((4, 6)), np.ones((4, 5), dtype=np.int64)
    bad = [dict(a=(P, d), kw=dict(subphone_features="phoneme"), match="Unknown value"),
           dict(a=(P, d), kw=dict(subphone_features="none"), match="deprecated"),
           dict(a=(P, d[:3]), kw={}, match=r"\(N, Dl\) and \(N, S\)"),
           dict(a=(P[0], d), kw={}, match=r"\(N, Dl\) and \(N, S\)"),
           dict(a=(P, np.ones((4, 9))), kw={}, match="1 .. 8"),
           dict(a=(P, np.ones((4, 0))), kw={}, match="1 .. 8"),
           dict(a=(np.zeros((8193, 2)), np.ones((8193, 1))), kw={}, match="8192"),
           dict(a=(P.astype(np.int64), d), kw={}, match="float32 or float64"),
           dict(a=(P, d.astype(bool)), kw={}, match="durations must be"),
           dict(a=(P, d), kw=dict(min_frames=-1), match="min_frames"),
           dict(a=(P, d), kw=dict(scale_=np.ones(15)), match="go together"),
           dict(a=(P, d), kw=dict(scale_=np.ones(14), min_=np.ones(15)), match="one value per output column"),
           dict(a=(P, d), kw=dict(dtype=np.int32), match="dtype must be")]
    for case in bad:
        with pytest.raises(ValueError, match=case["match"]):
            fe.frame_features(*case["a"], **case["kw"])
        with pytest.raises(ValueError, match=case["match"].replace(r"\(N, Dl\) and \(N, S\)", "Nmax")):
            fe.frame_features_batch(case["a"][0][None], case["a"][1][None], **case["kw"])
        with pytest.raises(ValueError):
            fe.frame_features(torch.from_numpy(case["a"][0]), torch.from_numpy(case["a"][1]), **case["kw"])
    with pytest.raises(ValueError, match="one entry per utterance"):
        fe.frame_features_batch(P[None], d[None], np.array([4, 4]))
    with pytest.raises(ValueError, match="Tmax"):
        fe.frame_features_batch(P[None], d[None], Tmax=-1)
    # out: a tensor of the right width (shape alone is looked at: a meta tensor has no memory)
    with pytest.raises(ValueError, match="out has 14 columns, the features have 15"):
        fe.frame_features_batch(P[None], d[None], out=torch.empty((1, 30, 14), device="meta"))
    with pytest.raises(ValueError, match="Tmax = 20 but out has 30"):
        fe.frame_features_batch(P[None], d[None], Tmax=20, out=torch.empty((1, 30, 15), device="meta"))
    with pytest.raises(ValueError, match="out must be"):
        fe.frame_features_batch(P[None], d[None], out=torch.empty((2, 30, 15), device="meta"))
    with pytest.raises(ValueError, match="CUDA"):
        fe.frame_features_batch(P[None], d[None], out=torch.empty((1, 30, 15)))
    assert list(inspect.signature(fe.frame_features).parameters) == ["phone_features", "durations", "subphone_features", "min_frames", "scale_",
                                                                      "min_", "dtype"]
    assert list(inspect.signature(fe.frame_features_batch).parameters) == ["phone_features", "durations", "num_phones", "subphone_features",
                                                                            "min_frames", "scale_", "min_", "Tmax", "out", "dtype", "strict"]
    kinds = {n: p.kind for n, p in inspect.signature(fe.frame_features_batch).parameters.items()}
    assert all(kinds[n] == inspect.Parameter.KEYWORD_ONLY for n in ("min_frames", "scale_", "min_", "Tmax", "out", "dtype", "strict"))


def test_the_python_table_is_the_model_s():
    from nnmnkwii_amd.frontend import merlin as fe
    cc = fe.coarse_coding_table()
    assert cc.dtype == np.float64 and np.array_equal(cc, FM.coarse_coding_table())
    G = np.load(os.path.join(ROOT, "tests", "golden", "frontend_ref.npz"))
    assert np.array_equal(cc, G["cc"])


def test_binding_checks_its_tensors_without_a_device():
    import torch
    from nnmnkwii_amd import _frontend_hip as FH
    d = torch.ones((2, 4, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        FH.frame_counts(d)
    with pytest.raises(ValueError, match="CUDA"):
        FH.expand(torch.zeros((2, 4, 3)), d, None, FH.FULL, 0, None, None, None, torch.zeros((2, 9, 12)))


def test_no_fallback_for_the_device_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError
    from nnmnkwii_amd.frontend import merlin as fe
    P, d = np.zeros((4, 6)), np.ones((4, 5), dtype=np.int64)
    with pytest.raises(HipExtensionError):
        fe.frame_features(P, d)
    with pytest.raises(HipExtensionError):
        fe.frame_features_batch(torch.from_numpy(P)[None], torch.from_numpy(d)[None], Tmax=30, strict=False)
