"""CPU-side checks of the nnmk_wave_* entry points and of nnmnkwii_amd.preprocessing.wave (-m "not gpu"): the symbols and the
version, the extension header as C99 -pedantic and a C program linked against the library, every refusal answered with fake
pointers before the runtime is touched and with no counter moving, nnmk_wave_plan against the model's plan, the untouched
mlpg_hip_* and other nnmk_* surfaces, the Python layer's errors raised before any device work, no fallback for the device route,
and the compat surface."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import wave_cases as WC
from wave_cases import WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nnmk_wave_abi_version", "nnmk_wave_encode", "nnmk_wave_decode", "nnmk_wave_plan", "nnmk_wave_launch_count")
SIX = ("mulaw", "inv_mulaw", "mulaw_quantize", "inv_mulaw_quantize", "preemphasis", "inv_preemphasis")
fake, fake2 = ctypes.c_void_p(64), ctypes.c_void_p(1 << 20)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _f0_hip, _frontend_hip, _metrics_hip, _wave_hip
    _metrics_hip.lib()
    _frontend_hip.lib()
    _f0_hip.lib()
    return _wave_hip.lib()


def _counts(L):
    return ([L.mlpg_hip_launch_count(k) for k in range(44)]
            + [L.nnmk_metrics_launch_count(), L.nnmk_frontend_launch_count(), L.nnmk_f0_launch_count(), L.nnmk_wave_launch_count()])


def encode(L, device=0, dtype_x=0, x=fake, ld_x=1000, lengths=fake, B=2, Lmax=1000, emphasis=1, coef=0.97, stage=2, mu=256, dtype_y=3, y=fake2,
           ld_y=1000):
    return L.nnmk_wave_encode(device, None, dtype_x, x, ld_x, lengths, B, Lmax, emphasis, coef, stage, mu, dtype_y, y, ld_y)


def decode(L, device=0, dtype_x=3, x=fake, ld_x=1000, lengths=fake, B=2, Lmax=1000, stage=2, mu=256, table=fake, emphasis=1, coef=0.97, segment=0,
           dtype_y=0, y=fake2, ld_y=1000):
    return L.nnmk_wave_decode(device, None, dtype_x, x, ld_x, lengths, B, Lmax, stage, mu, table, emphasis, coef, segment, dtype_y, y, ld_y)


def test_symbols_version_and_the_untouched_surfaces(L):
    from nnmnkwii_amd import _f0_hip, _frontend_hip, _hip, _metrics_hip, _wave_hip as WH
    for name in NAMES:
        assert getattr(L, name) is not None and name not in _hip.EXPORTS
    assert WH.NAMES == NAMES and L.nnmk_wave_abi_version() == 1 == WH.ABI_VERSION
    assert (WH.TILE, WH.TABLE_LDS) == (WM.TILE, WM.TABLE_LDS) == (1024, 4096)
    assert (WH.F32, WH.F64, WH.U8, WH.I16, WH.I32, WH.I64) == (WM.F32, WM.F64, WM.U8, WM.I16, WM.I32, WM.I64)
    assert (WH.PLAIN, WH.MULAW, WH.QUANTIZE) == (WM.PLAIN, WM.MULAW, WM.QUANTIZE)
    assert not any(n.startswith("nnmk_") for n in _hip.EXPORTS)
    assert len(_hip.EXPORTS) == 61 and L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert [L.mlpg_hip_launch_count(k) for k in (42, 43)] == [-1, -1] and L.nnmk_wave_launch_count() >= 0
    assert L.nnmk_metrics_abi_version() == 1 == _metrics_hip.ABI_VERSION
    assert L.nnmk_frontend_abi_version() == 1 == _frontend_hip.ABI_VERSION
    assert L.nnmk_f0_abi_version() == 1 == _f0_hip.ABI_VERSION
    assert "nnmk_" not in open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for other in ("nnmnkwii_metrics.h", "nnmnkwii_frontend.h", "nnmnkwii_f0.h"):
        assert "nnmk_wave" not in open(os.path.join(ROOT, "include", other)).read()
    header = open(os.path.join(ROOT, "include", "nnmnkwii_wave.h")).read()
    assert set(re.findall(r"\b(nnmk_wave_\w+)\s*\(", header)) == set(NAMES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+NNMK_WAVE_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(ABI_VERSION=1, F32=0, F64=1, U8=2, I16=3, I32=4, I64=5, PLAIN=0, MULAW=1, QUANTIZE=2, TILE=1024, TABLE_LDS=4096)


def test_header_is_c99_and_a_c_program_links(L, tmp_path):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.csrc import build as hip_build
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "main.c"
    src.write_text('#include "nnmnkwii_wave.h"\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   "  int64_t S = 0, W = 0, n = 0;\n"
                   "  if (nnmk_wave_plan(160000, 0.97, 0, &S, &W, &n) != 0) return 2;\n"
                   '  printf("%d %d %lld %lld %lld %lld\\n", nnmk_wave_abi_version(), NNMK_WAVE_TILE, nnmk_wave_launch_count(), (long long)S,\n'
                   "         (long long)W, (long long)n);\n"
                   "  if (nnmk_wave_plan(7000, 0.97, 1024, 0, 0, 0) != -1) return 3;\n"
                   "  if (nnmk_wave_decode(0, 0, NNMK_WAVE_F32, 0, 0, 0, 0, 0, 7, 256, 0, 0, 0.0, 0, NNMK_WAVE_F32, 0, 0) != -1) return 4;\n"
                   "  return nnmk_wave_encode(0, 0, NNMK_WAVE_I16, 0, 0, 0, 0, 0, 1, 0.97, NNMK_WAVE_QUANTIZE, 256, NNMK_WAVE_U8, 0, 0) != -1;\n}\n")
    exe = str(tmp_path / "main")
    so_dir = os.path.dirname(_hip.SO_PATH)
    r = subprocess.run([clang, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", so_dir, "-l:libmlpg_hip.so", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "1024", "0", "16384", "2048", "10"], (r.stdout, r.stderr[-2000:])


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    enc = [dict(dtype_x=2), dict(dtype_x=3), dict(dtype_x=5), dict(dtype_x=6), dict(dtype_x=-1), dict(stage=3), dict(stage=-1), dict(dtype_y=0),
           dict(dtype_y=1), dict(dtype_y=6), dict(stage=1, dtype_y=3), dict(stage=0, dtype_y=2), dict(mu=0), dict(mu=-5), dict(mu=256, dtype_y=2),
           dict(mu=40000, dtype_y=3), dict(B=-1), dict(Lmax=-1, ld_x=0, ld_y=0), dict(ld_x=999), dict(ld_y=999), dict(ld_x=0), dict(coef=float("nan")),
           dict(x=None), dict(y=None), dict(y=fake, dtype_y=4), dict(device=16), dict(device=-1),
           dict(emphasis=0, y=fake, dtype_y=3), dict(emphasis=0, y=fake, dtype_x=1, dtype_y=4)]
    for kw in enc:
        rc = encode(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"wave:"), (kw, rc, L.mlpg_hip_last_error())
    dec = [dict(stage=3), dict(stage=-1), dict(dtype_x=0), dict(dtype_x=1), dict(dtype_x=6), dict(stage=1), dict(stage=0), dict(dtype_y=2),
           dict(dtype_y=-1), dict(mu=0), dict(B=-1), dict(Lmax=-1, ld_x=0, ld_y=0), dict(ld_x=999), dict(ld_y=999), dict(coef=float("nan")),
           dict(segment=-1), dict(segment=100), dict(segment=512), dict(Lmax=7000, ld_x=7000, ld_y=7000, segment=1024),
           dict(coef=1.0, Lmax=7000, ld_x=7000, ld_y=7000, segment=2048), dict(coef=-1.5, Lmax=7000, ld_x=7000, ld_y=7000, segment=4096),
           dict(x=None), dict(y=None), dict(table=None), dict(y=fake, dtype_x=4), dict(device=16), dict(device=-1),
           dict(emphasis=0, y=fake, dtype_x=3), dict(emphasis=0, y=fake, dtype_x=4, dtype_y=1)]
    for kw in dec:
        rc = decode(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"wave:"), (kw, rc, L.mlpg_hip_last_error())
    assert encode(L, dtype_x=3) == -1 and b"not integers" in L.mlpg_hip_last_error()
    assert encode(L, mu=256, dtype_y=2) == -1 and b"does not fit uint8" in L.mlpg_hip_last_error()
    assert encode(L, y=fake, dtype_y=4) == -1 and b"y must not be x" in L.mlpg_hip_last_error()
    assert encode(L, emphasis=0, y=fake, dtype_y=3) == -1 and b"element sizes" in L.mlpg_hip_last_error()
    assert decode(L, y=fake, dtype_x=4) == -1 and b"y must not be x" in L.mlpg_hip_last_error()
    assert decode(L, Lmax=7000, ld_x=7000, ld_y=7000, segment=1024) == -1 and b"too short for this coef" in L.mlpg_hip_last_error()
    assert decode(L, segment=100) == -1 and b"no multiple of the tile" in L.mlpg_hip_last_error()
    assert decode(L, table=None) == -1 and b"NULL table" in L.mlpg_hip_last_error()
    assert decode(L, device=16) == -1 and b"device" in L.mlpg_hip_last_error()
    # an empty batch is still checked, then launches nothing and returns 0 (the pointers are never looked at)
    assert encode(L, B=0, stage=3) == -1 and decode(L, B=0, device=16) == -1
    for kw in (dict(B=0), dict(Lmax=0, ld_x=0, ld_y=0), dict(B=0, x=None, y=None, lengths=None)):
        assert encode(L, **kw) == 0 and decode(L, **kw) == 0, kw
    assert _counts(L) == c0


def test_plan_equals_the_model(L):
    from nnmnkwii_amd import _wave_hip as WH
    assert WH.plan(160000, 0.97) == (16384, 2048, 10) == WM.plan(160000, 0.97, 0)
    assert WM.AUTO_SEGMENT == WH.plan(1 << 20, 0.5)[0]
    for Lmax in (0, 1, 1024, 7000, 16384, 16385, 160000, (1 << 31) - 1):
        for coef in (0.97, 0.85, -0.97, 0.5, 0.999, 0.0, 0.9999, float(np.float32(0.97)), 1.0, -1.0, 1.5):
            for segment in (0, 1024, 2048, 4096, 16384, 65536, Lmax, Lmax + 1, 1000):
                try:
                    want = WM.plan(Lmax, coef, segment)
                except ValueError:
                    want = None
                try:
                    got = WH.plan(Lmax, coef, segment)
                except ValueError as e:
                    assert str(e).startswith("wave:")
                    got = None
                assert got == want, (Lmax, coef, segment, got, want)
    assert WH.plan(7000, 0.97, 7000) == (7000, 2048, 1) and WH.plan(7000, 1.0, 7000) == (7000, -1, 1) and WH.plan(7000, 0.5, 2048) == (2048, 1024, 4)
    assert L.nnmk_wave_plan(7000, 0.5, 2048, None, None, None) == 0 and L.nnmk_wave_plan(-1, 0.5, 0, None, None, None) == -1


def test_python_layer_raises_before_any_device_work():
    import torch
    from nnmnkwii_amd import preprocessing as P
    from nnmnkwii_amd.preprocessing import wave as PW
    for name in SIX + ("wave_encode_batch", "wave_decode_batch"):
        assert getattr(P, name) is getattr(PW, name)
    assert [list(inspect.signature(getattr(P, n)).parameters) for n in SIX] == [["x", "mu"], ["y", "mu"], ["x", "mu"], ["y", "mu"], ["x", "coef"],
                                                                               ["x", "coef"]]
    assert all(inspect.signature(getattr(P, n)).parameters["mu"].default == 256 for n in SIX[:4])
    assert all(inspect.signature(getattr(P, n)).parameters["coef"].default == 0.97 for n in SIX[4:])
    assert list(inspect.signature(P.wave_encode_batch).parameters) == ["X", "lengths", "coef", "mu", "quantize", "out", "dtype"]
    assert list(inspect.signature(P.wave_decode_batch).parameters) == ["Y", "lengths", "mu", "coef", "out", "segment"]
    for f in (P.preemphasis, P.inv_preemphasis):
        for ints in (np.arange(5), np.arange(5, dtype=np.int16), torch.arange(5)):
            with pytest.raises(TypeError, match="integer waveforms"):
                f(ints)
        for bad in (np.zeros((4, 2)), np.float64(0.5), torch.zeros((2, 2))):
            with pytest.raises(ValueError, match="1-D input only"):
                f(bad)
    with pytest.raises(TypeError, match="integer waveforms"):
        P.wave_encode_batch(np.zeros((2, 4), dtype=np.int16), coef=0.97)
    with pytest.raises(TypeError, match="classes are integers"):
        P.inv_mulaw_quantize(np.zeros(4))
    for f in (P.mulaw, P.inv_mulaw, P.mulaw_quantize):
        for mu in (0, -1, 255.5, None, "256"):
            with pytest.raises(ValueError, match="mu must be an integer"):
                f(np.zeros(4), mu)
    with pytest.raises(ValueError, match="mu must be an integer"):
        P.inv_mulaw_quantize(np.zeros(4, dtype=np.int64), 0)
    X = np.zeros((2, 5), dtype=np.float32)
    for bad in (np.zeros(5, dtype=np.float32), np.zeros((1, 2, 3), dtype=np.float32)):
        with pytest.raises(ValueError, match=r"\(B, Lmax\) batch"):
            P.wave_encode_batch(bad)
        with pytest.raises(ValueError, match=r"\(B, Lmax\) batch"):
            P.wave_decode_batch(bad)
    for lengths in (np.array([2.0, 3.0]), np.array([1, 2, 3]), [[1, 2]], torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError, match="one integer per utterance"):
            P.wave_encode_batch(X, lengths)
        with pytest.raises(ValueError, match="one integer per utterance"):
            P.wave_decode_batch(X, lengths)
    with pytest.raises(ValueError, match="does not fit"):
        P.wave_encode_batch(X, mu=256, dtype=np.uint8)
    with pytest.raises(ValueError, match="classes are uint8, int16, int32 or int64"):
        P.wave_encode_batch(X, dtype=np.float32)
    with pytest.raises(ValueError, match="float32 or float64"):
        P.wave_encode_batch(X, quantize=False, dtype=np.int16)
    with pytest.raises(ValueError, match="coef is NaN"):
        P.wave_encode_batch(X, coef=float("nan"))
    with pytest.raises(ValueError, match="out= is for CUDA tensors"):
        P.wave_encode_batch(X, out=torch.empty((2, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be a CUDA tensor of X's shape"):
        P.wave_decode_batch(torch.empty((2, 5), device="meta"), out=torch.empty((2, 4), device="meta"))
    with pytest.raises(ValueError, match="too short for this coef"):
        P.wave_decode_batch(np.zeros((1, 7000), dtype=np.float32), mu=None, coef=0.97, segment=1024)
    with pytest.raises(ValueError, match="no multiple of the tile"):
        P.wave_decode_batch(np.zeros((1, 7000), dtype=np.int16), coef=0.5, segment=1000)
    assert WC.same_bits(PW.inv_mulaw_table(256), WM.inv_mulaw_table(256)) and WC.same_bits(PW.inv_mulaw_table(255), WM.inv_mulaw_table(255))


def test_binding_checks_its_tensors_without_a_device():
    import torch
    from nnmnkwii_amd import _wave_hip as WH
    x = torch.zeros((2, 9))
    with pytest.raises(ValueError, match="CUDA"):
        WH.encode(x, None, 0.97, WH.PLAIN, 256, x)
    with pytest.raises(ValueError, match="CUDA"):
        WH.decode(x, None, WH.PLAIN, 256, None, None, 0, x)


def test_no_fallback_for_the_device_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError, preprocessing as P
    x = np.linspace(-1, 1, 9)
    for call in (lambda: P.mulaw(x), lambda: P.inv_mulaw(x), lambda: P.mulaw_quantize(0.5), lambda: P.inv_mulaw_quantize(np.arange(5)),
                 lambda: P.preemphasis(x), lambda: P.inv_preemphasis(torch.from_numpy(x)), lambda: P.wave_encode_batch(x[None], [9], 0.97),
                 lambda: P.wave_decode_batch(np.zeros((1, 9), dtype=np.uint8), mu=255, coef=0.97)):
        with pytest.raises(HipExtensionError):
            call()


def test_compat_surface_is_additive():
    from nnmnkwii_amd import compat, preprocessing as P
    S = compat._SURFACE
    for name in SIX:
        assert S["nnmnkwii.preprocessing.generic"][name] is getattr(P, name) is compat._REEXPORTS["nnmnkwii.preprocessing"][name]
    assert set(compat._REEXPORTS) == {"nnmnkwii.preprocessing"} and set(compat._REEXPORTS["nnmnkwii.preprocessing"]) == set(SIX)
    assert set(S["nnmnkwii.preprocessing"]) == {"delta_features", "trim_zeros_frames", "modspec", "modphase", "inv_modspec", "modspec_smoothing",
                                                "interp1d"} | set(compat._NORM)
    assert set(S["nnmnkwii.preprocessing.generic"]) == {"delta_features", "trim_zeros_frames"} | set(compat._NORM) | set(SIX)
    compat.install()
    try:
        import nnmnkwii.preprocessing
        import nnmnkwii.preprocessing.generic
        for name in SIX:
            assert getattr(nnmnkwii.preprocessing, name) is getattr(P, name) is getattr(nnmnkwii.preprocessing.generic, name)
    finally:
        compat.uninstall()
    assert not compat._saved                                                 # uninstall() put everything back
