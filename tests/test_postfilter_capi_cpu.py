"""CPU-side checks of the post-filter entry points (-m "not gpu"): exports and declarations, the ABI version and the
launch-counter kinds, the host-built table against the numpy model, refusals answered with fake pointers before the runtime is
touched, empty batches, and the Python layer's own argument checks."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import postfilter_model as PM  # noqa: E402

NAMES = ("mlpg_hip_postfilter_table", "mlpg_hip_merlin_post_filter")
fake = ctypes.c_void_p(64)


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(31)]


def pf(L, device=0, dtype=1, mgc=fake, ld_in=60, lengths=fake, B=2, Tmax=10, D=60, alpha=0.58, weight=fake, G=fake, fftlen=1024,
       out=ctypes.c_void_p(1 << 20), ld_out=60):
    return L.mlpg_hip_merlin_post_filter(device, None, dtype, mgc, ld_in, lengths, B, Tmax, D, alpha, weight, G, fftlen, out, ld_out)


def test_exports_declarations_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(29) >= 0
    assert L.mlpg_hip_launch_count(28) == -1 and L.mlpg_hip_launch_count(30) == -1
    # the frame tile the GPU tests stand on both sides of: one constant, the header's
    tile = int(re.search(r"#define\s+MLPG_HIP_POSTFILTER_FRAME_TILE\s+(\d+)", header).group(1))
    assert tile == _hip.POSTFILTER_FRAME_TILE and tile % 16 == 0


def test_the_table_agrees_with_the_model(L):
    from nnmnkwii_amd import _hip
    worst = 0.0
    for D in (1, 2, 3, 25, 60, 64):
        for order, fftlen in ((15, 32), (31, 64), (63, 64), (511, 1024)):
            if order < D - 1:
                continue
            for alpha in (0.0, 0.35, 0.58, 0.77, -0.42):
                G = _hip.postfilter_table_host(D, alpha, order, fftlen)
                ref = PM.table(D, alpha, order, fftlen)
                assert G.shape == ref.shape == (fftlen // 2 + 1, D)
                err = np.abs(G - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err <= 1e-13, (D, order, fftlen, alpha, err)
    print("table against the model: worst %.2e of max|G|" % worst)
    # the largest table the limits allow, and the smallest
    assert np.isfinite(_hip.postfilter_table_host(64, -0.9, 4095, 4096)).all()
    assert np.allclose(_hip.postfilter_table_host(1, 0.3, 0, 4), np.ones((3, 1)), rtol=0, atol=0)


def test_the_table_builder_refuses_what_is_outside_the_limits(L):
    c0 = _counts(L)
    buf = np.full(3 * 64, 7.0)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    for D, alpha, order, fftlen in [(0, 0.5, 15, 32), (65, 0.5, 511, 1024), (5, 0.5, 2, 3), (5, 0.5, 15, 24), (5, 0.5, 511, 8192),
                                    (5, 0.5, 32, 32), (5, 0.5, 1024, 1024), (5, 0.5, 3, 32), (5, 1.0, 15, 32), (5, -1.0, 15, 32),
                                    (5, float("nan"), 15, 32)]:
        assert L.mlpg_hip_postfilter_table(D, alpha, order, fftlen, p) == -1 and L.mlpg_hip_last_error(), (D, alpha, order, fftlen)
    assert L.mlpg_hip_postfilter_table(5, 0.5, 15, 32, None) == -1 and b"NULL" in L.mlpg_hip_last_error()
    assert L.mlpg_hip_postfilter_table(65, 0.5, 511, 1024, p) == -1 and b"[1, 64]" in L.mlpg_hip_last_error()
    assert L.mlpg_hip_postfilter_table(5, 0.5, 15, 24, p) == -1 and b"power of two" in L.mlpg_hip_last_error()
    assert (buf == 7.0).all() and _counts(L) == c0


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(D=0), dict(D=65, ld_in=65, ld_out=65), dict(fftlen=3), dict(fftlen=24), dict(fftlen=8192), dict(fftlen=2), dict(alpha=1.0),
             dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=1.5), dict(ld_in=59), dict(ld_out=59), dict(dtype=2), dict(dtype=-1),
             dict(device=-1), dict(device=16), dict(mgc=None), dict(weight=None), dict(G=None), dict(out=None), dict(B=-1),
             dict(Tmax=-1), dict(D=60, fftlen=32),                       # no order in [D - 1, fftlen) exists
             dict(mgc=fake, out=fake, ld_in=60, ld_out=61)]              # in place with unequal strides
    for kw in cases:
        rc = pf(L, **kw)
        assert rc == -1 and L.mlpg_hip_last_error(), (kw, rc)
    assert pf(L, D=65, ld_in=65, ld_out=65) == -1 and b"[1, 64]" in L.mlpg_hip_last_error()
    assert pf(L, fftlen=24) == -1 and b"power of two" in L.mlpg_hip_last_error()
    assert pf(L, alpha=1.0) == -1 and b"alpha" in L.mlpg_hip_last_error()
    assert pf(L, ld_in=59) == -1 and b"row strides" in L.mlpg_hip_last_error()
    assert pf(L, device=16) == -1 and b"merlin_post_filter: bad device" in L.mlpg_hip_last_error()
    # empty batches are no-ops: no pointer is looked at, nothing is launched
    assert pf(L, B=0, mgc=None, lengths=None, weight=None, G=None, out=None) == 0
    assert pf(L, Tmax=0, mgc=None, lengths=None, weight=None, G=None, out=None) == 0
    # ... but their sizes are still checked
    assert pf(L, B=0, D=65, ld_in=65, ld_out=65) == -1
    assert _counts(L) == c0


def test_python_layer_checks_its_arguments_without_a_device():
    from nnmnkwii_amd import _hip, compat, postfilters
    x = np.zeros((4, 5))
    for kw in (dict(fftlen=24), dict(fftlen=8192), dict(fftlen=2), dict(minimum_phase_order=3), dict(minimum_phase_order=1024),
               dict(weight=np.ones(4)), dict(weight=np.ones((5, 1)))):
        with pytest.raises(ValueError):
            postfilters.merlin_post_filter(x, 0.58, **kw)
    for alpha in (1.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            postfilters.merlin_post_filter(x, alpha)
    for bad in (np.zeros((4, 65)), np.zeros((4, 0)), np.zeros(5), np.zeros((2, 4, 5))):
        with pytest.raises(ValueError):
            postfilters.merlin_post_filter(bad, 0.58)
    with pytest.raises(ValueError):
        postfilters.merlin_post_filter_batch(np.zeros((4, 5)), 0.58)
    assert compat._SURFACE["nnmnkwii.postfilters"]["merlin_post_filter"] is postfilters.merlin_post_filter
    # the reference's signature and defaults
    import inspect
    sig = inspect.signature(postfilters.merlin_post_filter)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("mgc", inspect.Parameter.empty), ("alpha", inspect.Parameter.empty), ("minimum_phase_order", 511), ("fftlen", 1024),
        ("coef", 1.4), ("weight", None)]
    assert _hip.POSTFILTER_MAX_DIM == 64
