"""CPU-side checks of include/nnmnkwii_sample.h on the cross-compiled library (-m "not gpu"): the exports, the header text, the ABI
version, that the other headers and export lists know nothing of the new names, every refusal answered with fake pointers before
the runtime is touched and with no counter moving, the empty shapes, and the Python layer's errors that need no device."""
import ctypes
import glob
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
    from nnmnkwii_amd import _sample_hip, _trajectory_hip
    _trajectory_hip.lib()
    return _sample_hip.lib()


def _p(a):
    return a if a is None or isinstance(a, ctypes.c_void_p) else a.ctypes.data_as(ctypes.c_void_p)


def fac(L, device=0, dtype=1, var=fake(1), var_mode=0, ld_in=6, lengths=fake(2), B=2, Tmax=10, D=6, sd=2, nw=3, wl=WL, wu=WU, wc=WC,
        factor=fake(1000), ld_fac=2, logdet=fake(3000), status=fake(4000)):
    return L.nnmk_draw_factor(device, None, dtype, var, var_mode, ld_in, lengths, B, Tmax, D, sd, nw, _p(wl), _p(wu), _p(wc), factor, ld_fac,
                              logdet, status)


def draw(L, entry="sample", device=0, dtype=1, factor=fake(1000), ld_fac=2, status=fake(4000), lengths=fake(2), B=2, Tmax=10, sd=2, Q=2, K=3,
         src=fake(5000), ld_src=2, mean=fake(6000), ld_mean=2, out=fake(7000), ld_out=2):
    fn = L.nnmk_draw_sample if entry == "sample" else L.nnmk_draw_whiten
    return fn(device, None, dtype, factor, ld_fac, status, lengths, B, Tmax, sd, Q, K, src, ld_src, mean, ld_mean, out, ld_out)


def _counts(L):
    return [L.nnmk_draw_launch_count(), L.nnmk_traj_launch_count()] + [L.mlpg_hip_launch_count(k) for k in range(42)]


def test_exports_declarations_and_abi(L):
    from nnmnkwii_amd import _hip, _sample_hip
    header = open(os.path.join(ROOT, "include", "nnmnkwii_sample.h")).read()
    assert "#define NNMK_DRAW_ABI_VERSION 1" in header
    for name in _sample_hip.NAMES:
        assert getattr(L, name) is not None and re.search(r"\b%s\s*\(" % name, header), name
        assert name not in _hip.EXPORTS
    for name in ("nnmk_draw_abi_version", "nnmk_draw_launch_count", "nnmk_draw_factor", "nnmk_draw_sample", "nnmk_draw_whiten"):
        assert name in _sample_hip.NAMES
    assert L.nnmk_draw_abi_version() == 1 == _sample_hip.ABI_VERSION
    assert L.nnmk_draw_launch_count() >= 0 and L.nnmk_draw_group() >= 1
    # the other headers know nothing of it, and their versions are what they were
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if not path.endswith("nnmnkwii_sample.h"):
            assert "nnmk_draw" not in open(path).read(), path
    assert "#define NNMK_TRAJ_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "nnmnkwii_trajectory.h")).read()
    assert _hip.ABI_VERSION == 14 == L.mlpg_hip_abi_version() and L.nnmk_traj_abi_version() == 1


def test_factor_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(dtype=2), dict(dtype=-1), dict(var_mode=3), dict(var_mode=-1), dict(B=-1), dict(Tmax=-1), dict(D=-6), dict(sd=-2),
             dict(D=7), dict(sd=3), dict(nw=0), dict(nw=9), dict(wl=None), dict(wu=None), dict(wc=None), dict(wl=i32(0, 2, 1)),
             dict(wu=i32(0, 1, 2)), dict(wl=i32(0, -1, 1)), dict(ld_in=5), dict(ld_fac=1), dict(B=2 ** 24, sd=1, D=3, ld_fac=1, ld_in=3),
             dict(B=2 ** 23, sd=65, D=195, ld_fac=65, ld_in=195), dict(device=16), dict(device=-1), dict(var=None),
             dict(var_mode=1, var=None), dict(factor=None), dict(logdet=None), dict(status=None),
             dict(factor=fake(1)), dict(factor=ctypes.c_void_p(4096 + 8)), dict(var_mode=1, factor=ctypes.c_void_p(4096 + 40)),
             dict(factor=ctypes.c_void_p(4096 * 2 - 8 * 3 * 2 * 10 * 2 + 16)), dict(logdet=fake(1000)), dict(status=ctypes.c_void_p(4096 * 1000 + 64)),
             dict(ld_in=2 ** 62), dict(ld_in=2 ** 63 - 1), dict(ld_fac=2 ** 60), dict(ld_fac=2 ** 63 - 1), dict(B=2 ** 20, Tmax=2 ** 30, ld_in=2 ** 12)]
    for kw in cases:
        rc = fac(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"sample:"), (kw, rc, L.mlpg_hip_last_error())
    assert fac(L, D=7) == -1 and b"num_windows * sd" in L.mlpg_hip_last_error()
    assert fac(L, wl=i32(0, 2, 1)) == -1 and b"extents" in L.mlpg_hip_last_error()
    assert fac(L, ld_fac=1) == -1 and b"ld_fac" in L.mlpg_hip_last_error()
    assert fac(L, B=2 ** 24, sd=1, D=3, ld_fac=1, ld_in=3) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert fac(L, factor=fake(1)) == -1 and b"overlap" in L.mlpg_hip_last_error()
    assert fac(L, var=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    assert fac(L, ld_fac=2 ** 63 - 1) == -1 and b"past 2^62 bytes" in L.mlpg_hip_last_error()     # (no overflow in the alias check)
    null = dict(var=None, lengths=None, factor=None, logdet=None, status=None)
    assert fac(L, B=0, var_mode=2, **null) == 0
    assert fac(L, Tmax=0, var_mode=2, **null) == 0
    assert fac(L, sd=0, D=0, ld_in=0, ld_fac=0, var_mode=2, **null) == 0
    # ... but the arguments of an empty batch are still checked
    assert fac(L, B=0, dtype=2) == -1 and fac(L, B=0, device=16) == -1 and fac(L, B=0, wl=i32(0, 2, 1)) == -1 and fac(L, Tmax=0, D=7) == -1
    assert fac(L, B=0, ld_fac=1) == -1
    assert _counts(L) == c0


@pytest.mark.parametrize("entry", ["sample", "whiten"])
def test_draw_refusals_come_before_the_runtime_is_touched(L, entry):
    c0 = _counts(L)
    # the factor planes are 3 * 2 * 10 * 2 * 8 = 960 bytes at 4096000; out is 3 * 2 * 10 * 2 * 8 = 960 bytes
    cases = [dict(dtype=2), dict(dtype=-1), dict(B=-1), dict(Tmax=-1), dict(sd=-1), dict(K=-1), dict(Q=-1), dict(Q=3), dict(ld_fac=1),
             dict(ld_src=1), dict(ld_mean=1), dict(ld_out=1), dict(B=2 ** 24, sd=1, ld_fac=1, ld_src=1, ld_mean=1, ld_out=1),
             dict(B=2 ** 23, sd=65, ld_fac=65, ld_src=65, ld_mean=65, ld_out=65), dict(device=16), dict(device=-1), dict(factor=None),
             dict(status=None), dict(src=None), dict(out=None), dict(out=fake(1000)), dict(out=ctypes.c_void_p(4096 * 1000 + 952)),
             dict(out=ctypes.c_void_p(4096 * 1000 - 952)), dict(ld_fac=2 ** 60), dict(ld_src=2 ** 60), dict(ld_mean=2 ** 63 - 1),
             dict(ld_out=2 ** 63 - 1), dict(K=2 ** 30, B=2 ** 20, Tmax=2 ** 10, ld_src=2, ld_out=2)]
    for kw in cases:
        rc = draw(L, entry, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"sample:"), (kw, rc, L.mlpg_hip_last_error())
    assert draw(L, entry, K=-1) == -1 and b"K = -1" in L.mlpg_hip_last_error()
    assert draw(L, entry, Q=3) == -1 and b"Q = 3" in L.mlpg_hip_last_error()
    assert draw(L, entry, ld_out=1) == -1 and b"below sd" in L.mlpg_hip_last_error()
    assert draw(L, entry, out=fake(1000)) == -1 and b"overlaps the factor" in L.mlpg_hip_last_error()
    assert draw(L, entry, B=2 ** 24, sd=1, ld_fac=1, ld_src=1, ld_mean=1, ld_out=1) == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    assert draw(L, entry, ld_out=2 ** 63 - 1) == -1 and b"past 2^62 bytes" in L.mlpg_hip_last_error()
    # the inverse map reads the x of the frames behind t: its output may not lie on x
    if entry == "whiten":
        assert draw(L, entry, out=fake(5000)) == -1 and b"overlaps x" in L.mlpg_hip_last_error()
    # a NULL mean is no error, and its stride is not looked at: the empty shapes return 0 with it
    null = dict(factor=None, status=None, lengths=None, src=None, mean=None, out=None)
    assert draw(L, entry, B=0, **null) == 0 and draw(L, entry, Tmax=0, **null) == 0 and draw(L, entry, K=0, **null) == 0
    assert draw(L, entry, sd=0, ld_fac=0, ld_src=0, ld_mean=-5, ld_out=0, **null) == 0
    # ... but the arguments of an empty batch are still checked
    assert draw(L, entry, K=0, Q=3) == -1 and draw(L, entry, B=0, dtype=2) == -1 and draw(L, entry, Tmax=0, device=16) == -1
    assert draw(L, entry, K=0, ld_out=1) == -1
    assert _counts(L) == c0


def test_python_layer_raises_without_a_device():
    import torch
    from nnmnkwii_amd import _sample_calls as SC, compat, paramgen
    for name in ("mlpg_sample_batch", "mlpg_sample", "mlpg_whiten_batch"):
        assert name in paramgen.__all__ and callable(getattr(paramgen, name))
    assert "mlpg_sample" not in open(compat.__file__).read() and "mlpg_whiten" not in open(compat.__file__).read()
    win = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
    m = np.zeros((2, 5, 6))
    with pytest.raises(ValueError, match="num_samples"):
        paramgen.mlpg_sample_batch(m, None, win, num_samples=-1)
    with pytest.raises(ValueError, match="multiple"):
        paramgen.mlpg_sample_batch(np.zeros((2, 5, 7)), None, win)
    with pytest.raises(ValueError, match="noise must be"):
        paramgen.mlpg_sample_batch(m, None, win, num_samples=2, noise=np.zeros((3, 2, 5, 3)))
    # strides of (K, B, Tmax, sd) tensors: the planes of one dense tensor, refused by name otherwise
    parent = torch.zeros((3, 2, 9, 7), dtype=torch.float64)
    assert SC._planar_stride(parent[:, :, :, 2:5], "noise") == 7 and SC._planar_stride(parent, "noise") == 7
    for bad in (parent[:, :, ::2, :3][:, :, :4], parent.permute(1, 0, 2, 3)[:, :2], parent[:, :, :, ::2][..., :3],
                torch.zeros((3, 4, 9, 3), dtype=torch.float64)[:, ::2]):
        with pytest.raises(ValueError, match="sample: noise must be a column slice"):
            SC._planar_stride(bad, "noise")
    with pytest.raises(ValueError, match="CUDA tensor"):
        SC.sample(parent, torch.zeros((2, 7), dtype=torch.int32), None, torch.zeros((1, 2, 9, 7), dtype=torch.float64))
