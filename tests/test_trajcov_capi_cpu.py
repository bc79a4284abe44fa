"""CPU-side checks of include/nnmnkwii_trajectory.h on the cross-compiled library (-m "not gpu"): the exports, the ABI version,
every refusal answered with fake pointers before the runtime is touched and with no counter moving, the empty shapes, the
workspace sizes, and the Python layer's errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
fake = lambda k=1: ctypes.c_void_p(4096 * k)  # noqa: E731
i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
WL, WU, WC = i32(0, 1, 1), i32(0, 1, 1), np.array([1.0, -0.5, 0.0, 0.5, 1.0, -2.0, 1.0])


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _trajectory_hip
    return _trajectory_hip.lib()


def _p(a):
    return a if a is None or isinstance(a, ctypes.c_void_p) else a.ctypes.data_as(ctypes.c_void_p)


def cov(L, device=0, dtype=1, var=fake(1), var_mode=0, ld_in=6, lengths=fake(2), B=2, Tmax=10, D=6, sd=2, nw=3, wl=WL, wu=WU, wc=WC,
        want_band=1, band=fake(1000), ld_band=2, logdet=fake(3000), status=fake(4000)):
    return L.nnmk_traj_covariance(device, None, dtype, var, var_mode, ld_in, lengths, B, Tmax, D, sd, nw, _p(wl), _p(wu), _p(wc), want_band,
                                  band, ld_band, logdet, status)


def nll(L, device=0, dtype=1, mean=fake(5000), var=fake(1), var_mode=0, ld_in=6, lengths=fake(2), B=2, Tmax=10, D=6, sd=2, nw=3, wl=WL,
        wu=WU, wc=WC, cbar=fake(6000), ld_cbar=2, target=fake(7000), ld_target=2, band=fake(1000), ld_band=2, logdet=fake(3000),
        out=fake(8000), gm=fake(9000), gv=fake(10000), work=None, work_bytes=0):
    return L.nnmk_traj_nll(device, None, dtype, mean, var, var_mode, ld_in, lengths, B, Tmax, D, sd, nw, _p(wl), _p(wu), _p(wc), cbar,
                           ld_cbar, target, ld_target, band, ld_band, logdet, out, gm, gv, work, work_bytes)


def _counts(L):
    return [L.nnmk_traj_launch_count()] + [L.mlpg_hip_launch_count(k) for k in range(42)]


def test_exports_declarations_and_abi(L):
    from nnmnkwii_amd import _hip, _trajectory_hip
    header = open(os.path.join(ROOT, "include", "nnmnkwii_trajectory.h")).read()
    assert "#define NNMK_TRAJ_ABI_VERSION 1" in header
    for name in _trajectory_hip.NAMES:
        assert getattr(L, name) is not None and re.search(r"\b%s\s*\(" % name, header), name
        assert name not in _hip.EXPORTS
    assert L.nnmk_traj_abi_version() == 1 == _trajectory_hip.ABI_VERSION
    assert L.nnmk_traj_launch_count() >= 0
    # the main header knows nothing of it
    assert "nnmk_traj" not in open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()


def test_covariance_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(dtype=2), dict(dtype=-1), dict(var_mode=3), dict(var_mode=-1), dict(B=-1), dict(Tmax=-1), dict(D=-6), dict(sd=-2),
             dict(D=7), dict(sd=3), dict(nw=0), dict(nw=9), dict(wl=None), dict(wu=None), dict(wc=None), dict(wl=i32(0, 2, 1)),
             dict(wu=i32(0, 1, 2)), dict(wl=i32(0, -1, 1)), dict(ld_in=5), dict(ld_band=1), dict(B=2 ** 24, sd=1, D=3, ld_band=1, ld_in=3),
             dict(B=2 ** 23, sd=65, D=195, ld_band=65, ld_in=195), dict(device=16), dict(device=-1), dict(var=None),
             dict(var_mode=1, var=None), dict(band=None), dict(logdet=None), dict(status=None),
             dict(band=fake(1)), dict(band=ctypes.c_void_p(4096 + 8)), dict(var_mode=1, band=ctypes.c_void_p(4096 + 40)),
             dict(band=ctypes.c_void_p(4096 * 2 - 8 * 3 * 2 * 10 * 2 + 16)), dict(logdet=fake(1000)), dict(status=ctypes.c_void_p(4096 * 1000 + 64)),
             dict(ld_in=2 ** 62), dict(ld_in=2 ** 63 - 1), dict(ld_band=2 ** 60), dict(ld_band=2 ** 63 - 1), dict(B=2 ** 20, Tmax=2 ** 30, ld_in=2 ** 12)]
    for kw in cases:
        rc = cov(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"trajectory:"), (kw, rc, L.mlpg_hip_last_error())
    assert cov(L, D=7) == -1 and b"num_windows * sd" in L.mlpg_hip_last_error()
    assert cov(L, wl=i32(0, 2, 1)) == -1 and b"extents" in L.mlpg_hip_last_error()
    assert cov(L, ld_band=1) == -1 and b"ld_band" in L.mlpg_hip_last_error()
    assert cov(L, B=2 ** 24, sd=1, D=3, ld_band=1, ld_in=3) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert cov(L, band=fake(1)) == -1 and b"overlap" in L.mlpg_hip_last_error()
    assert cov(L, var=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    assert cov(L, ld_band=2 ** 63 - 1) == -1 and b"past 2^62 bytes" in L.mlpg_hip_last_error()     # (no overflow in the alias check)
    assert cov(L, ld_in=2 ** 62) == -1 and b"ld_in" in L.mlpg_hip_last_error()
    # without want_band neither the band nor its stride is looked at
    null = dict(var=None, lengths=None, band=None, logdet=None, status=None)
    assert cov(L, B=0, var_mode=2, **null) == 0
    assert cov(L, Tmax=0, var_mode=2, **null) == 0
    assert cov(L, sd=0, D=0, ld_in=0, ld_band=0, var_mode=2, **null) == 0
    # ... but the arguments of an empty batch are still checked
    assert cov(L, B=0, dtype=2) == -1 and cov(L, B=0, device=16) == -1 and cov(L, B=0, wl=i32(0, 2, 1)) == -1 and cov(L, Tmax=0, D=7) == -1
    assert _counts(L) == c0


def test_nll_refusals_and_workspace(L):
    c0 = _counts(L)
    cases = [dict(dtype=2), dict(var_mode=3), dict(B=-1), dict(Tmax=-1), dict(D=7), dict(nw=0), dict(wl=i32(0, 2, 1)), dict(ld_in=5),
             dict(var_mode=2, var=None, ld_in=5), dict(ld_cbar=1), dict(ld_target=1), dict(ld_band=1), dict(var_mode=2, var=None),
             dict(var_mode=1), dict(var_mode=1, work=fake(11000), work_bytes=95), dict(var_mode=1, work=ctypes.c_void_p(4096 * 11 + 4), work_bytes=96),
             dict(work_bytes=-1), dict(device=16), dict(mean=None), dict(var=None), dict(cbar=None), dict(target=None), dict(logdet=None),
             dict(out=None), dict(band=None), dict(B=2 ** 24, sd=1, D=3, ld_in=3, ld_cbar=1, ld_target=1, ld_band=1),
             dict(ld_in=2 ** 62), dict(ld_cbar=2 ** 63 - 1), dict(ld_target=2 ** 61), dict(ld_band=2 ** 63 - 1)]
    for kw in cases:
        rc = nll(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"trajectory:"), (kw, rc, L.mlpg_hip_last_error())
    assert nll(L, var_mode=2, var=None) == -1 and b"unit variances have no gradient" in L.mlpg_hip_last_error()
    assert nll(L, var_mode=1) == -1 and b"workspace" in L.mlpg_hip_last_error()
    assert nll(L, band=None) == -1 and b"needs the band" in L.mlpg_hip_last_error()
    null = dict(mean=None, var=None, lengths=None, cbar=None, target=None, band=None, logdet=None, out=None, gm=None, gv=None)
    assert nll(L, B=0, var_mode=2, **null) == 0 and nll(L, Tmax=0, var_mode=2, **null) == 0
    assert nll(L, sd=0, D=0, ld_in=0, ld_cbar=0, ld_target=0, ld_band=0, var_mode=2, **null) == 0
    assert nll(L, B=0, ld_cbar=1) == -1
    assert L.nnmk_traj_nll_workspace(1, 1, 2, 6) == 96 and L.nnmk_traj_nll_workspace(1, 0, 2, 6) == 0
    assert L.nnmk_traj_nll_workspace(0, 1, 2, 6) == 0 and L.nnmk_traj_nll_workspace(2, 1, 2, 6) == 0
    assert L.nnmk_traj_nll_workspace(3, 1, 2, 6) == -1 and L.nnmk_traj_nll_workspace(1, 1, -2, 6) == -1
    assert _counts(L) == c0


def test_python_layer_raises_without_a_device():
    import torch
    from nnmnkwii_amd import autograd, paramgen
    for name in ("mlpg_covariance_batch", "mlpg_variance", "mlpg_logdet"):
        assert name in paramgen.__all__ and callable(getattr(paramgen, name))
    assert callable(autograd.trajectory_nll) and issubclass(autograd.TrajectoryNLL, torch.autograd.Function)
    win = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
    m, c = torch.zeros((2, 5, 6), dtype=torch.float64), torch.zeros((2, 5, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="out of scope"):
        autograd.trajectory_nll(m, None, win, c.clone().requires_grad_())
    with pytest.raises(ValueError, match="reduction"):
        autograd.trajectory_nll(m, None, win, c, reduction="avg")
    with pytest.raises(ValueError, match="multiple"):
        autograd.trajectory_nll(torch.zeros((2, 5, 7), dtype=torch.float64), None, win, c)
    with pytest.raises(ValueError, match="target must be"):
        autograd.trajectory_nll(m, None, win, m)
    with pytest.raises(TypeError, match="dtype"):
        autograd.trajectory_nll(m, torch.ones((2, 5, 6)), win, c)
    with pytest.raises(ValueError, match="variances must have"):
        autograd.trajectory_nll(m, torch.ones((2, 4, 6), dtype=torch.float64), win, c)


def test_band_strides_are_checked_with_the_module_s_own_error():
    """A band whose planes or utterances do not lie at the strides of one dense (Q + 1, B, Tmax, ld) tensor is refused by name,
    not by torch's view error; a column slice of such a tensor gives its row stride."""
    import torch
    from nnmnkwii_amd import _trajectory_calls as TC
    parent = torch.zeros((3, 2, 9, 7), dtype=torch.float64)
    assert TC._band_stride(parent[:, :, :, 2:5], 2, 2, 9, 3) == 7 and TC._band_stride(parent, 2, 2, 9, 7) == 7
    for bad in (parent[:, :, ::2, :3][:, :, :4], parent.permute(1, 0, 2, 3)[:, :2], parent[:, :, :, ::2][..., :3],
                torch.zeros((3, 4, 9, 3), dtype=torch.float64)[:, ::2]):
        B, T, sd = bad.shape[1:]
        with pytest.raises(ValueError, match="trajectory: band must be a column slice"):
            TC._band_stride(bad, bad.shape[0] - 1, B, T, sd)
