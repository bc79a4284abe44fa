"""CPU-side checks of mlpg_hip_column_stats, mlpg_hip_column_stats_workspace and mlpg_hip_column_affine (-m "not gpu"): exports
and declarations, the ABI version and the launch-counter kinds, every refusal answered with fake pointers before the runtime is
touched and with no counter moving, empty batches, the workspace function (overflow included), the Python layer's ValueErrors
and the compat surface."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mlpg_hip_column_stats", "mlpg_hip_column_stats_workspace", "mlpg_hip_column_affine")
REFERENCE_NAMES = ("meanvar", "meanstd", "minmax", "scale", "inv_scale", "minmax_scale_params", "minmax_scale", "inv_minmax_scale")
fake = ctypes.c_void_p(64)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(44)]


def stats(L, device=0, dtype=1, x=fake, ld_x=6, lengths=fake, B=2, Tmax=10, D=6, state_in=fake, state_out=fake, workspace=fake,
          workspace_bytes=1 << 20):
    return L.mlpg_hip_column_stats(device, None, dtype, x, ld_x, lengths, B, Tmax, D, state_in, state_out, workspace, workspace_bytes)


def affine(L, device=0, in_dtype=1, out_dtype=1, mode=0, x=fake, ld_x=6, y=ctypes.c_void_p(1 << 20), ld_y=6, lengths=fake, B=2, Tmax=10,
           D=6, a=fake, c=fake):
    return L.mlpg_hip_column_affine(device, None, in_dtype, out_dtype, mode, x, ld_x, y, ld_y, lengths, B, Tmax, D, a, c)


def test_exports_declarations_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, header)
    assert len(_hip.EXPORTS) == 61 == len(set(_hip.EXPORTS))
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(39) >= 0 and L.mlpg_hip_launch_count(41) >= 0
    assert [L.mlpg_hip_launch_count(k) for k in (38, 40, 42, 43)] == [-1, -1, -1, -1]
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MLPG_HIP_COLSTATS_(\w+)\s+(\d+)", header, re.M)}
    assert defs == dict(CHUNK_ROWS=_hip.COLSTATS_CHUNK_ROWS, BLOCK_ROWS=_hip.COLSTATS_BLOCK_ROWS)
    # the shapes of the tests (tests/norm_cases.py) follow the model's constants: they are the module's
    import norm_cases
    assert (norm_cases.CHUNK, norm_cases.BLOCK) == (_hip.COLSTATS_CHUNK_ROWS, _hip.COLSTATS_BLOCK_ROWS)


def test_column_stats_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(dtype=2), dict(dtype=-1), dict(B=-1), dict(Tmax=-1), dict(D=-1, ld_x=0), dict(ld_x=5), dict(device=16), dict(device=-1),
             dict(x=None), dict(state_out=None), dict(workspace=None), dict(workspace_bytes=2 * 5 * 6 * 8 - 1), dict(workspace_bytes=0)]
    for kw in cases:
        rc = stats(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"column_stats:"), (kw, rc, L.mlpg_hip_last_error())
    assert stats(L, ld_x=5) == -1 and b"row stride" in L.mlpg_hip_last_error()
    assert stats(L, x=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    assert stats(L, workspace_bytes=479) == -1 and b"480" in L.mlpg_hip_last_error()
    assert stats(L, workspace=ctypes.c_void_p(68)) == -1 and b"8-byte aligned" in L.mlpg_hip_last_error()
    assert stats(L, B=1 << 30, Tmax=1 << 30, D=1 << 30, ld_x=1 << 30, workspace_bytes=(1 << 63) - 1) == -1 and b"too large" in L.mlpg_hip_last_error()
    # D == 0: nothing to do, no pointer is looked at -- but the arguments are still checked
    assert stats(L, D=0, ld_x=0, x=None, lengths=None, state_in=None, state_out=None, workspace=None, workspace_bytes=0) == 0
    assert stats(L, B=0, D=0, ld_x=0, x=None, lengths=None, state_in=None, state_out=None, workspace=None, workspace_bytes=0) == 0
    assert stats(L, D=0, ld_x=0, dtype=2) == -1 and stats(L, D=0, ld_x=0, device=16) == -1 and stats(L, D=0, ld_x=-1) == -1
    # an empty batch with D > 0 still writes state_out: it is required
    assert stats(L, B=0, x=None, workspace=None, workspace_bytes=0, state_out=None) == -1 and b"state_out" in L.mlpg_hip_last_error()
    assert _counts(L) == c0


def test_column_stats_refuses_more_columns_than_the_finish_step_has_threads_for(L):
    """The finish step takes one workgroup of 256 threads per 4 columns, and a grid is 32 bits of threads: 2^24 - 1 workgroups,
    2^26 - 4 columns (the statistics kernel, one workgroup per 64 columns, would take 2^30).  At the bound the call passes the
    check (the next refusal, the device's, answers); four columns more are refused with the limit named.  No counter moves."""
    c0 = _counts(L)
    most = 4 * ((1 << 24) - 1)
    big = dict(B=1, Tmax=1, workspace_bytes=(1 << 62))
    assert stats(L, D=most, ld_x=most, device=16, **big) == -1 and b"bad device" in L.mlpg_hip_last_error()
    assert stats(L, D=most + 1, ld_x=most + 1, device=16, **big) == -1
    assert b"16777215 workgroups of 256 threads" in L.mlpg_hip_last_error()
    assert stats(L, D=most + 1, ld_x=most + 1, device=16, B=0, Tmax=1, workspace_bytes=0) == -1        # an empty batch has a finish step too
    assert b"16777215 workgroups of 256 threads" in L.mlpg_hip_last_error()
    assert _counts(L) == c0


def test_column_affine_refusals_and_empty_batches(L):
    c0 = _counts(L)
    cases = [dict(in_dtype=2), dict(out_dtype=2), dict(out_dtype=-1), dict(mode=2), dict(mode=-1), dict(B=-1), dict(Tmax=-1),
             dict(D=-1, ld_x=0, ld_y=0), dict(ld_x=5), dict(ld_y=5), dict(device=16), dict(device=-1), dict(x=None), dict(y=None),
             dict(a=None), dict(c=None), dict(y=fake, out_dtype=0), dict(y=fake, ld_y=7)]
    for kw in cases:
        rc = affine(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"column_affine:"), (kw, rc, L.mlpg_hip_last_error())
    assert affine(L, mode=2) == -1 and b"mode" in L.mlpg_hip_last_error()
    assert affine(L, y=fake, ld_y=7) == -1 and b"in place" in L.mlpg_hip_last_error()
    null = dict(x=None, y=None, a=None, c=None, lengths=None)
    assert affine(L, B=0, **null) == 0 and affine(L, Tmax=0, **null) == 0 and affine(L, D=0, ld_x=0, ld_y=0, **null) == 0
    assert affine(L, B=0, mode=2) == -1 and affine(L, B=0, device=16) == -1 and affine(L, B=0, ld_x=5) == -1
    assert _counts(L) == c0


def test_workspace_bytes(L):
    from nnmnkwii_amd import _hip
    ws = L.mlpg_hip_column_stats_workspace
    blk = _hip.COLSTATS_BLOCK_ROWS
    assert ws(0, 10, 6) == 0 and ws(2, 0, 6) == 0 and ws(2, 10, 0) == 0
    assert ws(1, 1, 1) == 40 and ws(2, 10, 6) == 2 * 5 * 6 * 8
    assert ws(3, blk, 7) == 3 * 40 * 7 and ws(3, blk + 1, 7) == 2 * 3 * 40 * 7 and ws(512, 2000, 187) == 512 * -(-2000 // blk) * 40 * 187
    assert ws(-1, 10, 6) == -1 and ws(2, -1, 6) == -1 and ws(2, 10, -1) == -1
    big = 2 ** 31 - 1
    assert ws(big, big, big) == -1                       # 2^31 * 2^22 * 2^31 * 40 does not fit 63 bits
    assert ws(big, 1, 1) == big * 40 and ws(big, big, 1) == big * -(-big // blk) * 40
    assert _hip.column_stats_workspace(2, 10, 6) == 480
    with pytest.raises(ValueError, match="too large"):
        _hip.column_stats_workspace(big, big, big)


def test_python_layer_raises_value_errors_without_a_device():
    import torch
    from nnmnkwii_amd import _hip, preprocessing as P
    x = np.zeros((4, 3))
    for f in (P.minmax_scale, P.inv_minmax_scale):
        with pytest.raises(ValueError, match="must be specified"):
            f(x)
        with pytest.raises(ValueError, match="must be specified"):
            f(x, data_min=np.zeros(3))
        with pytest.raises(ValueError, match="must be specified"):
            f(x, scale_=np.ones(3), data_max=np.ones(3))
    with pytest.raises(ValueError, match="dimensions"):
        P.scale(np.zeros(3), 0.0, 1.0)
    with pytest.raises(ValueError, match="out= is for CUDA tensors"):
        P.scale(x, 0.0, 1.0, out=x)
    with pytest.raises(ValueError, match="lengths go with"):
        P.inv_scale(x, 0.0, 1.0, lengths=[4])
    with pytest.raises(ValueError, match="CUDA"):
        _hip.column_stats(torch.zeros((2, 5, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="CUDA"):
        _hip.column_affine(torch.zeros((2, 5, 3)), None, None, 0)
    # host arithmetic only: the reference's formulas, zero range -> 1
    min_, scale_ = P.minmax_scale_params(np.array([0.0, 1.0, 2.0]), np.array([0.0, 3.0, 2.5]), feature_range=(0.1, 0.9))
    assert np.array_equal(scale_, 0.8 / np.array([1.0, 2.0, 0.5])) and np.array_equal(min_, 0.1 - np.array([0.0, 1.0, 2.0]) * scale_)
    std = np.array([0.0, 2.0])
    assert np.array_equal(P.generic._zero_to_one(std), [1.0, 2.0]) and std[0] == 0.0          # on a copy
    for name in REFERENCE_NAMES + ("column_stats",):
        assert callable(getattr(P, name)) and getattr(P, name) is getattr(P.generic, name)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nnmnkwii_amd import HipExtensionError, preprocessing as P
    X = np.zeros((2, 5, 3))
    for call in (lambda: P.meanvar(X), lambda: P.meanstd([X[0], X[1]]), lambda: P.minmax(X), lambda: P.column_stats(X),
                 lambda: P.scale(X[0], np.zeros(3), np.ones(3)), lambda: P.inv_scale(X, np.zeros(3), np.ones(3)),
                 lambda: P.minmax_scale(X[0], np.zeros(3), np.ones(3)), lambda: P.inv_minmax_scale(X[0], np.zeros(3), np.ones(3))):
        with pytest.raises(HipExtensionError):
            call()


def test_compat_surface_has_the_reference_names():
    import nnmnkwii_amd.compat as compat
    from nnmnkwii_amd import preprocessing as P, util
    for name in REFERENCE_NAMES:
        assert compat._SURFACE["nnmnkwii.preprocessing"][name] is getattr(P, name)
        assert compat._SURFACE["nnmnkwii.preprocessing.generic"][name] is getattr(P, name)
    for name in ("delta_features", "trim_zeros_frames"):
        assert compat._SURFACE["nnmnkwii.preprocessing.generic"][name] is getattr(P, name)
    import inspect
    assert list(inspect.signature(P.meanvar).parameters) == ["dataset", "lengths", "mean_", "var_", "last_sample_count", "return_last_sample_count"]
    assert list(inspect.signature(P.minmax_scale).parameters)[:6] == ["x", "data_min", "data_max", "feature_range", "scale_", "min_"]
    assert util._gen.scale is P.scale
