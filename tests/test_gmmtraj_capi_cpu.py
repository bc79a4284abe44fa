"""CPU-side checks of mlpg_hip_gmm_trajectory_stats (-m "not gpu"): export and declaration, the ABI version and the
launch-counter kinds, the row tile on both sides, refusals answered with fake pointers before the runtime is touched, empty
batches, and the Python layer's own argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mlpg_hip_gmm_trajectory_stats"
fake = ctypes.c_void_p(64)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(36)]


def ts(L, device=0, x=fake, ld_x=6, lengths=fake, B=2, Tmax=10, D=6, labels=fake, mu_x=fake, mu_y=fake, A=fake, cvar=fake, M=4,
       mean=ctypes.c_void_p(1 << 20), ld_mean=6, var=ctypes.c_void_p(1 << 21), ld_var=6):
    return L.mlpg_hip_gmm_trajectory_stats(device, None, x, ld_x, lengths, B, Tmax, D, labels, mu_x, mu_y, A, cvar, M, mean, ld_mean,
                                           var, ld_var)


def test_export_declaration_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    assert NAME in _hip.EXPORTS and getattr(L, NAME) is not None
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(33) >= 0
    assert L.mlpg_hip_launch_count(32) == -1 and L.mlpg_hip_launch_count(34) == -1
    tile = int(re.search(r"#define\s+MLPG_HIP_GMM_TRAJ_ROW_TILE\s+(\d+)", header).group(1))
    assert tile == _hip.GMM_TRAJ_ROW_TILE and tile % 16 == 0


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(D=0, ld_x=0, ld_mean=0, ld_var=0), dict(D=129, ld_x=129, ld_mean=129, ld_var=129), dict(M=0), dict(M=65537), dict(M=-1),
             dict(ld_x=5), dict(ld_mean=5), dict(ld_var=5), dict(B=-1), dict(Tmax=-1), dict(device=16), dict(device=-1),
             dict(x=None), dict(labels=None), dict(mu_x=None), dict(mu_y=None), dict(A=None), dict(cvar=None), dict(mean=None),
             dict(var=None)]
    for kw in cases:
        rc = ts(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error(), (kw, rc)
    assert ts(L, D=129, ld_x=129, ld_mean=129, ld_var=129) == -1 and b"[1, 128]" in L.mlpg_hip_last_error()
    assert ts(L, M=0) == -1 and b"[1, 65536]" in L.mlpg_hip_last_error()
    assert ts(L, ld_x=5) == -1 and b"row strides" in L.mlpg_hip_last_error()
    assert ts(L, device=16) == -1 and b"gmm_trajectory_stats: bad device" in L.mlpg_hip_last_error()
    assert ts(L, x=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    # empty batches are no-ops: no pointer is looked at, nothing is launched
    null = dict(x=None, lengths=None, labels=None, mu_x=None, mu_y=None, A=None, cvar=None, mean=None, var=None)
    assert ts(L, B=0, **null) == 0
    assert ts(L, Tmax=0, **null) == 0
    # ... but their sizes are still checked
    assert ts(L, B=0, D=129, ld_x=129, ld_mean=129, ld_var=129) == -1
    assert ts(L, B=0, device=16) == -1
    assert _counts(L) == c0


def test_python_layer_checks_its_arguments_without_a_device():
    import torch
    from sklearn.mixture import GaussianMixture
    from nnmnkwii_amd import _hip
    from nnmnkwii_amd.baseline.gmm import MLPG
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    lab = torch.zeros(10, dtype=torch.int32)
    with pytest.raises(ValueError, match="float64 CUDA"):   # wrong dtype
        _hip.gmm_trajectory_stats(torch.zeros((2, 5, 6), dtype=torch.float32), None, lab, z(4, 6), z(4, 6), z(4, 6, 6), z(4, 6))
    with pytest.raises(ValueError, match="float64 CUDA"):   # a host tensor
        _hip.gmm_trajectory_stats(z(2, 5, 6), None, lab, z(4, 6), z(4, 6), z(4, 6, 6), z(4, 6))
    with pytest.raises(ValueError, match="float64 CUDA"):
        _hip.gmm_trajectory_stats(np.zeros((2, 5, 6)), None, lab, z(4, 6), z(4, 6), z(4, 6, 6), z(4, 6))
    rng = np.random.RandomState(0)
    g = GaussianMixture(n_components=2, covariance_type="full", random_state=0).fit(rng.randn(200, 12))
    m = MLPG(g)
    assert m.static_dim == 3
    with pytest.raises(ValueError, match="transform_batch"):     # static-only input
        m.transform_padded(np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="transform_batch"):
        m.transform_padded(torch.zeros((2, 5, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        m.transform_padded(np.zeros((5, 6)))
    with pytest.raises(ValueError):
        m.transform_padded(np.zeros((2, 5, 7)))
    with pytest.raises(ValueError, match="float64 CUDA"):
        m.transform_padded(torch.zeros((2, 5, 6), dtype=torch.float64))
    assert m.transform_batch([]) == []
