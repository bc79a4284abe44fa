"""CPU-side checks of mlpg_hip_gv_ascent, mlpg_hip_gv and mlpg_hip_gv_max_frames (-m "not gpu"): exports and declarations, the
ABI version and the launch-counter kinds, every refusal answered with fake pointers before the runtime is touched and with no
counter moving, empty batches, and the Python layer's ValueErrors."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mlpg_hip_gv_ascent", "mlpg_hip_gv", "mlpg_hip_gv_max_frames")
fake = ctypes.c_void_p(64)
i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
WL, WU, WC = i32(0, 1, 1), i32(0, 1, 1), np.array([1.0, -0.5, 0.0, 0.5, 1.0, -2.0, 1.0])
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(40)]


def asc(L, device=0, dtype=1, mean=fake, var=fake, var_mode=0, lengths=fake, B=2, Tmax=10, D=6, nw=3, wl=WL, wu=WU, wc=WC, y_in=fake,
        y_out=ctypes.c_void_p(1 << 20), gv_mean=fake, gv_prec=fake, omega_scale=1.0, n_iter=10, step=-1.0, init=1, report=fake,
        status=fake):
    p = lambda a: a if a is None or isinstance(a, ctypes.c_void_p) else ptr(a)  # noqa: E731
    return L.mlpg_hip_gv_ascent(device, None, dtype, mean, var, var_mode, lengths, B, Tmax, D, nw, p(wl), p(wu), p(wc), y_in, y_out,
                                gv_mean, gv_prec, omega_scale, n_iter, step, init, report, status)


def gv(L, device=0, dtype=1, x=fake, ld_x=6, lengths=fake, B=2, Tmax=10, D=6, out=fake):
    return L.mlpg_hip_gv(device, None, dtype, x, ld_x, lengths, B, Tmax, D, out)


def test_exports_declarations_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, header)
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(35) >= 0 and L.mlpg_hip_launch_count(37) >= 0
    assert [L.mlpg_hip_launch_count(k) for k in (34, 36, 38)] == [-1, -1, -1]
    assert L.mlpg_hip_gv_max_frames() >= 2048 and _hip.gv_max_frames() == L.mlpg_hip_gv_max_frames()


def test_gv_ascent_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    big = L.mlpg_hip_gv_max_frames() + 1
    cases = [dict(n_iter=-1), dict(n_iter=100001), dict(D=7), dict(D=-3), dict(B=-1), dict(Tmax=-1), dict(nw=0), dict(nw=9),
             dict(wl=None), dict(wu=None), dict(wc=None), dict(wl=i32(0, 2, 1)), dict(wu=i32(0, 1, 2)), dict(wl=i32(0, -1, 1)),
             dict(dtype=2), dict(var_mode=3), dict(var_mode=0, var=None), dict(var_mode=1, var=None), dict(init=2), dict(init=-1),
             dict(omega_scale=0.0), dict(omega_scale=float("nan")), dict(omega_scale=float("inf")), dict(step=float("nan")),
             dict(step=float("inf")), dict(Tmax=big), dict(device=16), dict(device=-1), dict(mean=None), dict(y_in=None),
             dict(y_out=None), dict(gv_mean=None), dict(gv_prec=None), dict(report=None), dict(status=None)]
    for kw in cases:
        rc = asc(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error().startswith(b"gv_ascent:"), (kw, rc, L.mlpg_hip_last_error())
    assert asc(L, n_iter=100001) == -1 and b"[0, 100000]" in L.mlpg_hip_last_error()
    assert asc(L, D=7) == -1 and b"multiple" in L.mlpg_hip_last_error()
    assert asc(L, wl=i32(0, 2, 1)) == -1 and b"extents" in L.mlpg_hip_last_error()
    assert asc(L, Tmax=big) == -1 and b"at most %d frames" % (big - 1) in L.mlpg_hip_last_error()
    assert asc(L, mean=None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    # unit variances need no var; empty batches are no-ops: no pointer is looked at, nothing is launched
    null = dict(mean=None, var=None, lengths=None, y_in=None, y_out=None, gv_mean=None, gv_prec=None, report=None, status=None)
    assert asc(L, B=0, var_mode=2, **null) == 0
    assert asc(L, Tmax=0, var_mode=2, **null) == 0
    assert asc(L, D=0, var_mode=2, **null) == 0
    # ... but their arguments are still checked
    assert asc(L, B=0, n_iter=-1) == -1 and asc(L, B=0, device=16) == -1 and asc(L, B=0, wl=i32(0, 2, 1)) == -1
    assert _counts(L) == c0


def test_gv_refusals_and_empty_batches(L):
    c0 = _counts(L)
    for kw in (dict(dtype=2), dict(ld_x=5), dict(B=-1), dict(Tmax=-1), dict(D=-1, ld_x=0), dict(device=16), dict(x=None), dict(out=None)):
        assert gv(L, **kw) == -1 and L.mlpg_hip_last_error().startswith(b"gv:"), kw
    assert gv(L, B=0, x=None, out=None, lengths=None) == 0
    assert gv(L, D=0, ld_x=0, x=None, out=None, lengths=None) == 0
    assert gv(L, B=0, ld_x=5) == -1
    assert _counts(L) == c0


def test_python_layer_raises_value_errors_without_a_device():
    import torch
    from sklearn.mixture import GaussianMixture
    from nnmnkwii_amd import _hip, paramgen
    from nnmnkwii_amd.baseline.gmm import MLPG
    win = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
    m, v = np.zeros((2, 5, 6)), np.ones((2, 5, 6))
    one = np.ones(3)
    with pytest.raises(ValueError, match="gv_var must be positive"):
        paramgen.mlpg_gv_batch(m, v, win, one, np.array([1.0, 0.0, 1.0]))
    with pytest.raises(ValueError, match="gv_var must be positive"):
        paramgen.mlpg_gv(m[0], v[0], win, one, np.array([1.0, 1.0, -2.0]))
    with pytest.raises(ValueError, match="gv_var must be positive"):
        paramgen.mlpg_gv_batch(m, v, win, one, np.array([1.0, np.nan, 1.0]))
    with pytest.raises(ValueError, match="one entry per static dimension"):
        paramgen.mlpg_gv_batch(m, v, win, np.ones(2), np.ones(2))
    with pytest.raises(ValueError, match="init"):
        paramgen.mlpg_gv_batch(m, v, win, one, one, init="ml")
    with pytest.raises(ValueError, match="n_iter"):
        paramgen.mlpg_gv_batch(m, v, win, one, one, n_iter=100001)
    with pytest.raises(ValueError, match="omega_scale"):
        paramgen.mlpg_gv_batch(m, v, win, one, one, omega_scale=0.0)
    with pytest.raises(ValueError, match="step"):
        paramgen.mlpg_gv_batch(m, v, win, one, one, step=float("nan"))
    with pytest.raises(ValueError, match="multiple"):
        paramgen.mlpg_gv_batch(np.zeros((2, 5, 7)), np.ones((2, 5, 7)), win, one, one)
    for name in ("gv", "gv_stats", "mlpg_gv", "mlpg_gv_batch"):
        assert name in paramgen.__all__ and callable(getattr(paramgen, name))
    with pytest.raises(ValueError, match="CUDA"):
        _hip.gv(torch.zeros((2, 5, 3), dtype=torch.float64))
    # baseline.gmm.MLPG
    rng = np.random.RandomState(0)
    g = GaussianMixture(n_components=2, covariance_type="full", random_state=0).fit(rng.randn(200, 12))
    with pytest.raises(ValueError, match="diff=True"):
        MLPG(g, diff=True, gv=(one, one))
    with pytest.raises(ValueError, match="gv_var must be positive"):
        MLPG(g, gv=(one, np.zeros(3)))
    with pytest.raises(ValueError, match="one entry per static dimension"):
        MLPG(g, gv=(np.ones(6), np.ones(6)))
    with pytest.raises(ValueError, match="unknown gv_options"):
        MLPG(g, gv=(one, one), gv_options=dict(iterations=3))
    with pytest.raises(ValueError, match="gv_options go with"):
        MLPG(g, gv_options=dict(n_iter=3))
    with pytest.raises(ValueError, match="n_iter"):
        MLPG(g, gv=(one, one), gv_options=dict(n_iter=-1))
    mm = MLPG(g, gv=(one, 2 * one), gv_options=dict(n_iter=5, step=0.25))
    assert mm.gv_options == dict(n_iter=5, step=0.25, init="scaled", omega_scale=1.0) and np.array_equal(mm.gv[1], 2 * one)
    assert MLPG(g).gv is None
