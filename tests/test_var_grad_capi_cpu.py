"""CPU-side checks (-m "not gpu") of mlpg_hip_backward_var: its argument validation answers before any device is touched,
and its launch counter (kind 13) exists while kind 12 still reads -1."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _args():
    wl = np.array([0, 1], dtype=np.int32)
    wu = np.array([0, 1], dtype=np.int32)
    wc = np.array([1.0, -0.5, 0.0, 0.5])
    st = np.zeros(2, dtype=np.int32)
    return wl, wu, wc, st


def _call(L, device=0, dtype=1, var_mode=0, y=64, status=True, B=1, Tmax=4, D=4, nw=2):
    wl, wu, wc, st = _args()
    fake = ctypes.c_void_p(64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return L.mlpg_hip_backward_var(device, None, dtype, 0, fake, fake, var_mode, ctypes.c_void_p(y) if y else None, fake, None,
                                   B, Tmax, D, nw, p(wl), p(wu), p(wc), fake, fake, p(st) if status else None)


def test_backward_var_validates_without_gpu(L):
    assert _call(L, var_mode=2) == -1                      # unit variances: nothing to differentiate
    assert b"MLPG_HIP_VAR_UNIT" in L.mlpg_hip_last_error()
    assert _call(L, status=False) == -1                    # status is required
    assert b"status" in L.mlpg_hip_last_error()
    assert _call(L, y=0) == -1                             # the trajectory is required
    assert b"NULL" in L.mlpg_hip_last_error()
    assert _call(L, dtype=7) == -1                         # bad dtype
    assert b"dtype" in L.mlpg_hip_last_error()
    assert _call(L, D=5) == -1                             # D not a multiple of num_windows
    assert b"multiple" in L.mlpg_hip_last_error()
    assert _call(L, var_mode=5) == -1                      # unknown variance mode
    assert b"var_mode" in L.mlpg_hip_last_error()
    assert _call(L, device=-1) == -1                       # a bad device
    assert b"device" in L.mlpg_hip_last_error()
    assert _call(L, B=0) == 0                              # an empty batch
    assert _call(L, Tmax=0) == 0                           # no frames


def test_launch_counter_kind_13(L):
    assert L.mlpg_hip_launch_count(13) >= 0
    assert L.mlpg_hip_launch_count(12) == -1 and L.mlpg_hip_launch_count(14) == -1


def test_binding_exports_backward_var(L):
    from nnmnkwii_amd import _hip
    assert "mlpg_hip_backward_var" in _hip.EXPORTS and _hip.ABI_VERSION == L.mlpg_hip_abi_version() == 14
    assert callable(_hip.backward_var)
    from nnmnkwii_amd import autograd as AF
    assert AF.MLPGBatch is not None and callable(AF.mlpg_batch)
