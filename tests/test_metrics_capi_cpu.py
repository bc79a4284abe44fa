"""CPU-side checks of the nnmk_metrics_* entry points and of nnmnkwii_amd.metrics (-m "not gpu"): the symbols, the extension
header as C99 -pedantic and a C program linked against the library, every refusal answered with fake pointers before the runtime
is touched and with no counter moving, the workspace function (overflow included), the untouched mlpg_hip_* surface, the Python
layer's ValueErrors, the host path against the reference's values, the compat surface, and no fallback for the device route."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import metrics_cases as C
from metrics_cases import MM

ROOT = C.ROOT
NAMES = ("nnmk_metrics_abi_version", "nnmk_metrics_workspace", "nnmk_metrics_batch", "nnmk_metrics_launch_count")
REFERENCE_NAMES = ("melcd", "mean_squared_error", "lf0_mean_squared_error", "vuv_error")
fake = ctypes.c_void_p(64)
G = C.golden()


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _metrics_hip
    return _metrics_hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(44)] + [L.nnmk_metrics_launch_count()]


def _terms(*ts):
    from nnmnkwii_amd import _metrics_hip as M
    return (M.Term * max(len(ts), 1))(*[M.term(**t) for t in ts])


ONE = dict(kind=0, x_col=1, width=4)


def batch(L, device=0, dtype_x=0, x=fake, ld_x=6, dtype_y=1, y=fake, ld_y=7, lengths=fake, B=2, Tmax=10, terms=(ONE,), nterms=None,
          per_utt=fake, totals=fake, workspace=fake, workspace_bytes=1 << 20):
    arr = None if terms is None else _terms(*terms)
    return L.nnmk_metrics_batch(device, None, dtype_x, x, ld_x, dtype_y, y, ld_y, lengths, B, Tmax, arr,
                                len(terms or ()) if nterms is None else nterms, per_utt, totals, workspace, workspace_bytes)


def test_symbols_version_and_the_untouched_mlpg_surface(L):
    from nnmnkwii_amd import _hip, _metrics_hip as M
    for name in NAMES:
        assert getattr(L, name) is not None and name not in _hip.EXPORTS
    assert M.NAMES == NAMES and L.nnmk_metrics_abi_version() == 1 == M.ABI_VERSION
    assert not any(n.startswith("nnmk_") for n in _hip.EXPORTS)
    assert len(_hip.EXPORTS) == 61 and L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert [L.mlpg_hip_launch_count(k) for k in (42, 43)] == [-1, -1] and L.nnmk_metrics_launch_count() >= 0
    main_header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    assert "nnmk_" not in main_header
    header = open(os.path.join(ROOT, "include", "nnmnkwii_metrics.h")).read()
    assert set(re.findall(r"\b(nnmk_metrics_\w+)\s*\(", header)) == set(NAMES)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+NNMK_METRICS_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(ABI_VERSION=M.ABI_VERSION, F32=0, F64=1, MAX_TERMS=M.MAX_TERMS, BLOCK_ROWS=M.BLOCK_ROWS, MAX_ROW_BYTES=M.MAX_ROW_BYTES,
                        FRAME_L2=M.FRAME_L2, SQUARED=M.SQUARED, VOICED_SQUARED=M.VOICED_SQUARED, MISMATCH=M.MISMATCH, FLAG_EXP=M.FLAG_EXP)
    assert (MM.BLOCK_ROWS, MM.MAX_TERMS, MM.FRAME_L2, MM.SQUARED, MM.VOICED_SQUARED, MM.MISMATCH, MM.FLAG_EXP) == (
        M.BLOCK_ROWS, M.MAX_TERMS, M.FRAME_L2, M.SQUARED, M.VOICED_SQUARED, M.MISMATCH, M.FLAG_EXP)
    assert ctypes.sizeof(M.Term) == 40 == C.term_bytes([MM.term(0, 0)]).itemsize


def test_header_is_c99_and_a_c_program_links(L, tmp_path):
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.csrc import build as hip_build
    hipcc = hip_build._hipcc()
    clang = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang") if os.path.sep in hipcc else ""
    if not os.path.exists(clang):
        clang = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "main.c"
    src.write_text('#include "nnmnkwii_metrics.h"\n#include <stdio.h>\n'
                   "int main(void) {\n  nnmk_metrics_term t = {NNMK_METRICS_FRAME_L2, 1, 1, 59, 0, 0, 0, 0.0};\n"
                   '  printf("%d %d %lld %d\\n", nnmk_metrics_abi_version(), (int)sizeof t, (long long)nnmk_metrics_workspace(3, 257, 4), t.width);\n'
                   "  return 0;\n}\n")
    exe = str(tmp_path / "main")
    so_dir = os.path.dirname(_hip.SO_PATH)
    r = subprocess.run([clang, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                        "-L", so_dir, "-l:libmlpg_hip.so", "-Wl,-rpath," + so_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["1", "40", str(3 * 2 * 4 * 16), "59"], (r.stdout, r.stderr[-2000:])


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    voiced = dict(kind=2, x_col=1, width=1, x_mask_col=2)
    cases = [dict(dtype_x=2), dict(dtype_y=-1), dict(B=-1), dict(Tmax=-1), dict(ld_x=-1), dict(ld_x=4), dict(ld_y=4), dict(nterms=0),
             dict(terms=(ONE,) * 9), dict(terms=None, nterms=1), dict(terms=(dict(ONE, kind=4),)), dict(terms=(dict(ONE, kind=-1),)),
             dict(terms=(dict(ONE, width=0),)), dict(terms=(dict(ONE, x_col=-1),)), dict(terms=(dict(ONE, y_col=4),)),
             dict(terms=(dict(voiced, width=2),)), dict(terms=(dict(voiced, x_mask_col=6),)), dict(terms=(dict(voiced, y_mask_col=7),)),
             dict(terms=(dict(voiced, x_mask_col=-1),)), dict(terms=(dict(voiced, flags=2),)), dict(terms=(dict(ONE, flags=1),)),
             dict(device=16), dict(device=-1), dict(x=None), dict(y=None), dict(totals=None), dict(workspace=None),
             dict(workspace=ctypes.c_void_p(68)), dict(workspace_bytes=31), dict(workspace_bytes=0),
             dict(ld_x=5000, ld_y=5000, terms=(dict(ONE, width=2049),)), dict(B=1 << 30, Tmax=1 << 30, workspace_bytes=(1 << 63) - 1)]
    for kw in cases:
        rc = batch(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"metrics:"), (kw, rc, L.mlpg_hip_last_error())
    assert batch(L, ld_x=4) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert batch(L, nterms=0) == -1 and b"1 .. 8" in L.mlpg_hip_last_error()
    assert batch(L, terms=(dict(ONE, kind=4),)) == -1 and b"unknown kind" in L.mlpg_hip_last_error()
    assert batch(L, terms=(dict(voiced, width=2),)) == -1 and b"width 1" in L.mlpg_hip_last_error()
    assert batch(L, terms=(dict(voiced, x_mask_col=6),)) == -1 and b"mask columns" in L.mlpg_hip_last_error()
    assert batch(L, x=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    assert batch(L, workspace_bytes=31) == -1 and b" 32" in L.mlpg_hip_last_error()
    assert batch(L, workspace=ctypes.c_void_p(68)) == -1 and b"8-byte aligned" in L.mlpg_hip_last_error()
    assert batch(L, B=1 << 30, Tmax=1 << 30, workspace_bytes=(1 << 63) - 1) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert batch(L, ld_x=5000, ld_y=5000, terms=(dict(ONE, width=2049),)) == -1 and b"16000" in L.mlpg_hip_last_error()
    # an empty batch still writes the totals, so they are required; its other arguments are still checked
    assert batch(L, B=0, x=None, y=None, workspace=None, workspace_bytes=0, totals=None) == -1 and b"totals" in L.mlpg_hip_last_error()
    assert batch(L, B=0, dtype_x=2) == -1 and batch(L, B=0, device=16) == -1 and batch(L, B=0, nterms=9) == -1
    assert _counts(L) == c0


def test_workspace_bytes(L):
    from nnmnkwii_amd import _metrics_hip as M
    ws = L.nnmk_metrics_workspace
    blk = M.BLOCK_ROWS
    assert ws(0, 10, 4) == 0 and ws(2, 0, 4) == 0 and ws(2, 10, 0) == 0
    assert ws(1, 1, 1) == 16 and ws(2, 10, 1) == 32 and ws(3, blk, 8) == 3 * 128 and ws(3, blk + 1, 8) == 2 * 3 * 128
    assert ws(512, 2000, 4) == 512 * -(-2000 // blk) * 64
    assert ws(-1, 10, 4) == -1 and ws(2, -1, 4) == -1 and ws(2, 10, -1) == -1
    big = 2 ** 31 - 1
    assert ws(big, big, 8) == big * -(-big // blk) * 128
    assert ws(big, big, big) == -1                       # 2^31 * 2^23 * 2^31 * 16 does not fit 63 bits
    assert M.metrics_workspace(2, 10, 1) == 32
    with pytest.raises(ValueError, match="too large"):
        M.metrics_workspace(big, big, big)


def test_python_layer_raises_value_errors_without_a_device():
    import torch
    from nnmnkwii_amd import _metrics_hip as M, metrics
    x = torch.zeros((2, 5, 3))
    with pytest.raises(ValueError, match="CUDA"):
        M.metrics_batch(x, x, [M.term(M.SQUARED, 0)])
    X = np.zeros((2, 5, 6))
    for bad in ({"a": ("melcd", slice(0, 6, 2))}, {"a": ("melcd", 6)}, {"a": ("rmse", 1)}, {"a": ("lf0_mse", 1)}, {"a": "melcd"}, {},
                {str(i): ("mse", i % 6) for i in range(9)}):
        with pytest.raises(ValueError, match="batch_metrics"):
            metrics.batch_metrics(X, X, None, bad)
    with pytest.raises(ValueError, match="batches of the same"):
        metrics.batch_metrics(X, X[:, :4], None, {"a": ("mse", 0)})
    with pytest.raises(ValueError, match="agree in shape"):
        metrics.mean_squared_error(X, X[:1])
    with pytest.raises(ValueError, match="lf0 and vuv"):
        metrics.vuv_error(X, X)
    with pytest.raises(ValueError, match="lengths for a batch"):
        metrics.mean_squared_error(X, X, [5])
    for name in REFERENCE_NAMES:
        assert callable(getattr(metrics, name))
    assert list(inspect.signature(metrics.melcd).parameters) == ["X", "Y", "lengths"]
    assert list(inspect.signature(metrics.mean_squared_error).parameters) == ["X", "Y", "lengths"]
    assert list(inspect.signature(metrics.lf0_mean_squared_error).parameters) == ["src_f0", "src_vuv", "tgt_f0", "tgt_vuv", "lengths", "linear_domain"]
    assert list(inspect.signature(metrics.vuv_error).parameters) == ["src_vuv", "tgt_vuv", "lengths"]
    assert list(inspect.signature(metrics.batch_metrics).parameters) == ["X", "Y", "lengths", "terms", "per_utterance", "vuv_threshold"]


def _figure_bound(key, B, Tmax, dtype, width):
    kind = {"melcd": MM.FRAME_L2, "mse": MM.SQUARED, "lf0": MM.VOICED_SQUARED, "vuv": MM.MISMATCH}[key.split("/")[0]]
    t = MM.term(kind, 0, width=width, flags=MM.FLAG_EXP if key.endswith("linear") else 0)
    return C.reference_bound(B, Tmax, t, dtype) + 3 * C.U


@pytest.mark.parametrize("name", sorted(C.G_CASES))
@pytest.mark.parametrize("tensors", [False, True])
def test_host_path_equals_the_reference(name, tensors):
    """numpy arrays and CPU tensors: the host path, in float64 from the definitions.  melcd on numpy arrays is the reference's own
    arithmetic: equal.  The others: within the bound for another summation order (float32 inputs: the reference's float32 error)."""
    import torch
    from nnmnkwii_amd import metrics
    X, Y, L = G[name + "/X"], G[name + "/Y"], G[name + "/lengths"]
    if tensors:
        X, Y = torch.from_numpy(X), torch.from_numpy(Y)
    got = C.golden_calls(metrics, X, Y, L)
    for key, value in got.items():
        want = float(G["%s/%s" % (name, key)])
        assert isinstance(value, float)
        if key.startswith("melcd") and not tensors:
            assert value == want, key
        width = {"melcd/lengths": 11, "melcd/utterance": 11, "melcd/frame": 11, "mse/batch": 11}.get(key, 3 if key.startswith("mse") else 1)
        assert C.close(value, want, _figure_bound(key, len(L), X.shape[1], G[name + "/X"].dtype, width)), (key, value, want)
    # the whole evaluation in one call, and per utterance
    terms = {"mcd": ("melcd", C.G_MGC), "bap": ("mse", C.G_BAP), "lf0": ("lf0_mse", C.G_LF0, C.G_VUV), "lf0_hz": ("lf0_mse", C.G_LF0, C.G_VUV, True),
             "vuv": ("vuv_error", C.G_VUV)}
    one = metrics.batch_metrics(X, Y, L, terms)
    for k, key in (("mcd", "melcd/lengths"), ("bap", "mse/lengths"), ("lf0", "lf0/lengths"), ("lf0_hz", "lf0/lengths_linear"), ("vuv", "vuv/lengths")):
        # the same host sums; melcd on numpy arrays is the reference's arithmetic instead (float32 for float32 inputs)
        rel = _figure_bound(key, len(L), X.shape[1], G[name + "/X"].dtype, 11) if k == "mcd" else 4 * C.U
        assert C.close(one[k], got[key], rel), (k, one[k], got[key])
    per = metrics.batch_metrics(X, Y, L, terms, per_utterance=True)
    for k, v in per.items():
        assert v.shape == (len(L),) and v.dtype == np.float64 and np.isnan(v[1]) and np.isfinite(v[[0, 3, 4]]).all()
    assert C.close(per["mcd"][3], got["melcd/utterance"], _figure_bound("melcd/utterance", 1, int(L[3]), G[name + "/X"].dtype, 11))
    assert per["vuv"][3] == got["vuv/utterance"]


def test_thresholds_and_nothing_counted():
    from nnmnkwii_amd import metrics
    x = np.array([[[5.0, 0.9], [5.1, 0.4], [5.2, 0.8]]])
    y = np.array([[[5.5, 0.7], [5.0, 0.6], [5.0, 0.2]]])
    r = metrics.batch_metrics(x, y, None, {"lf0": ("lf0_mse", 0, 1), "vuv": ("vuv_error", 1)}, vuv_threshold=0.5)
    assert r["lf0"] == 0.5 and r["vuv"] == 2.0 / 3.0                      # voiced on both sides: frame 0 alone; flags differ in 1 and 2
    r = metrics.batch_metrics(x, y, None, {"lf0": ("lf0_mse", 0, 1), "vuv": ("vuv_error", 1)})
    assert np.isnan(r["lf0"]) and r["vuv"] == 1.0                          # the reference's rules: no flags sum to 2, all values differ
    assert np.isnan(metrics.mean_squared_error(x, y, [0])) and np.isnan(metrics.vuv_error(x[:, :, 1], y[:, :, 1], [0]))
    assert np.isnan(metrics.lf0_mean_squared_error(x[0, :, 0], x[0, :, 1], y[0, :, 0], y[0, :, 1]))


def test_no_fallback_for_the_device_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError, metrics
    x = torch.zeros((2, 5, 3))
    with pytest.raises(HipExtensionError):
        metrics._device_pairs(x, x, None, [(1, 0, 0, 3, 0, 0, 0, None)])


def test_compat_surface_has_the_reference_names():
    import nnmnkwii_amd.compat as compat
    from nnmnkwii_amd import metrics
    assert set(compat._SURFACE["nnmnkwii.metrics"]) == set(REFERENCE_NAMES)
    for name in REFERENCE_NAMES:
        assert compat._SURFACE["nnmnkwii.metrics"][name] is getattr(metrics, name)
    compat.install()
    try:
        import nnmnkwii.metrics as RM
        assert RM.melcd is metrics.melcd and RM.vuv_error is metrics.vuv_error
    finally:
        compat.uninstall()
