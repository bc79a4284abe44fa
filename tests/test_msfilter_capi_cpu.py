"""CPU-side checks of the modulation-spectrum filter's entry points (-m "not gpu"): exports and declarations, the ABI version and
the launch-counter kinds, mlpg_hip_modspec_filter_form, refusals answered with fake pointers before the runtime is touched, empty
batches, and the Python layer's own argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mlpg_hip_modspec_filter_form", "mlpg_hip_modspec_filter")
fake = ctypes.c_void_p(64)
F32, F64 = 0, 1


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(33)]


def mf(L, device=0, dtype=F64, x=fake, ld_x=5, lengths=fake, B=2, Tmax=10, D=5, n=16, ortho=0, A=fake, C=fake, limit_bin=9,
       log_domain=1, out=ctypes.c_void_p(1 << 20), ld_out=5):
    return L.mlpg_hip_modspec_filter(device, None, dtype, x, ld_x, lengths, B, Tmax, D, n, ortho, A, C, limit_bin, log_domain, out,
                                     ld_out)


def test_exports_declarations_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(31) >= 0
    assert L.mlpg_hip_launch_count(32) == -1 and L.mlpg_hip_launch_count(30) == -1


def test_filter_form_names_the_lengths_the_launch_takes(L):
    ns = list(range(-2, 70)) + [100, 1000, 1024, 2047, 2048, 4096, 4097, 8192]
    for n in ns:
        want = 1 if 2 <= n <= 4096 and n & (n - 1) == 0 else 0
        assert L.mlpg_hip_modspec_filter_form(n) == want == L.mlpg_hip_modspec_loss_form(n), n
    L.mlpg_hip_modspec_set_direct(1)
    try:
        for n in ns:
            assert L.mlpg_hip_modspec_filter_form(n) == 0, n
        c0 = _counts(L)
        assert mf(L, n=16) == -1 and L.mlpg_hip_last_error().startswith(b"modspec_filter:")
        assert _counts(L) == c0
    finally:
        L.mlpg_hip_modspec_set_direct(0)
    assert L.mlpg_hip_modspec_filter_form(4096) == 1


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    cases = [dict(dtype=2), dict(dtype=-1), dict(dtype=7),                                # float32 / float64 only
             dict(n=0), dict(n=1), dict(n=-16), dict(n=24), dict(n=100), dict(n=8192),     # n with form 0
             dict(Tmax=17), dict(n=8, Tmax=9),                                             # Tmax > n
             dict(ld_x=4), dict(ld_out=4), dict(ld_x=-1), dict(ld_out=0),                  # ld < D
             dict(A=None), dict(C=None),                                                   # exactly one table
             dict(limit_bin=-1), dict(limit_bin=10), dict(n=4096, Tmax=10, limit_bin=2050),  # limit_bin outside [0, nb]
             dict(B=-1), dict(Tmax=-1), dict(D=-1),                                        # negative sizes
             dict(device=-1), dict(device=16), dict(device=99),                            # device outside [0, 16)
             dict(x=None), dict(out=None),                                                 # NULL x / out
             dict(x=fake, out=fake, ld_x=5, ld_out=6)]                                     # in place with unequal strides
    for kw in cases:
        rc = mf(L, **kw)
        err = L.mlpg_hip_last_error().decode()
        assert rc == -1 and err.startswith("modspec_filter:"), (kw, rc, err)
    assert mf(L, Tmax=17) == -1 and b"time length" in L.mlpg_hip_last_error()
    assert mf(L, ld_x=4) == -1 and b"row strides" in L.mlpg_hip_last_error()
    assert mf(L, A=None) == -1 and b"both or neither" in L.mlpg_hip_last_error()
    assert mf(L, limit_bin=10) == -1 and b"limit_bin" in L.mlpg_hip_last_error()
    assert mf(L, device=16) == -1 and b"modspec_filter: bad device" in L.mlpg_hip_last_error()
    assert mf(L, n=24) == -1 and b"power of two" in L.mlpg_hip_last_error()
    assert _counts(L) == c0


def test_empty_batches_are_no_ops(L):
    c0 = _counts(L)
    for kw in (dict(B=0), dict(D=0, ld_x=0, ld_out=0), dict(B=0, D=0), dict(Tmax=0)):
        assert mf(L, x=None, lengths=None, A=None, C=None, out=None, **kw) == 0, kw
        assert mf(L, x=None, lengths=None, out=None, **kw) == 0, kw
    # ... but their arguments are still checked
    assert mf(L, B=0, n=24) == -1 and mf(L, B=0, limit_bin=10) == -1 and mf(L, D=0, dtype=2) == -1 and mf(L, B=0, device=16) == -1
    assert _counts(L) == c0


def test_python_layer_checks_its_arguments_without_a_device():
    from nnmnkwii_amd import postfilters, preprocessing
    x = np.zeros((2, 20, 3))
    A = np.ones((9, 3))
    with pytest.raises(RuntimeError, match="DFT length 16 must be larger than time length 20"):
        postfilters.modspec_post_filter_batch(x, A, A, n=16)
    with pytest.raises(RuntimeError, match="DFT length 16 must be larger than time length 20"):
        preprocessing.modspec_smoothing_batch(x, 200, n=16)
    with pytest.raises(ValueError, match="Nyquist"):
        postfilters.modspec_post_filter_batch(x, None, None, n=32, modfs=200, cutoff=101)
    with pytest.raises(ValueError, match="Nyquist"):
        preprocessing.modspec_smoothing_batch(x, 200, n=32, cutoff=101)
    with pytest.raises(ValueError, match="modfs"):
        postfilters.modspec_post_filter_batch(x, None, None, n=32, cutoff=50)
    with pytest.raises(ValueError, match="even"):
        postfilters.modspec_post_filter_batch(x, None, None, n=33)
    for a, c in ((A, None), (None, A)):
        with pytest.raises(ValueError, match="both or neither"):
            postfilters.modspec_post_filter_batch(x, a, c, n=32)
    for bad in (np.zeros((20, 3)), np.zeros(5)):
        with pytest.raises(ValueError):
            postfilters.modspec_post_filter_batch(bad, None, None, n=32)
    with pytest.raises(ValueError):
        postfilters.modspec_post_filter(x, None, None, n=32)
    with pytest.raises(ValueError):
        preprocessing.modspec_smoothing_batch(x, 200, n=1)


def test_the_python_table_builder_is_the_models():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import msfilter_model as MM
    from nnmnkwii_amd import postfilters
    rng = np.random.RandomState(0)
    mg, mn = rng.randn(9, 4), rng.randn(9, 4)
    sg, sn = rng.uniform(0.5, 2, (9, 4)), rng.uniform(0.5, 2, (9, 4))
    sg[0, 0], sg[1, 1], mg[2, 2], sn[3, 3] = 0.0, -1.0, np.nan, np.inf
    for k in (0.0, 0.85, 1.0):
        A, C = postfilters.modspec_post_filter_tables(mg, sg, mn, sn, k)
        Ar, Cr = MM.tables(mg, sg, mn, sn, k)
        assert A.dtype == C.dtype == np.float64 and (A == Ar).all() and (C == Cr).all()
    import torch
    At, Ct = postfilters.modspec_post_filter_tables(*(torch.from_numpy(t) for t in (mg, sg, mn, sn)), k=0.85)
    Ar, Cr = MM.tables(mg, sg, mn, sn, 0.85)
    assert np.allclose(At.numpy(), Ar, rtol=1e-15, atol=0) and np.allclose(Ct.numpy(), Cr, rtol=1e-14, atol=1e-16)
