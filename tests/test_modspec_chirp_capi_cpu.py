"""CPU-side checks of the chirp-z route of the float64 modulation-spectrum entry points (-m "not gpu"): mlpg_hip_modspec_route over
the DFT lengths with the direct switch off and on, the export and its declaration, counter kind 20, the ABI version, and
refusals at a chirp-z length answered with fake pointers before the runtime is touched."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

fake = ctypes.c_void_p(64)
LENGTHS = list(range(-2, 70)) + [100, 1000, 1024, 1025, 2047, 2048, 2049, 3000, 4096, 4097, 5000, 8192]


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(21)]


def _expected(n):
    """The rule of the issue, restated: powers of two in [2, 4096] FFT; any other n in [3, 2048] chirp-z; the rest direct."""
    if n < 2:
        return -1
    if n <= 4096 and n & (n - 1) == 0:
        return 0
    return 2 if 3 <= n <= 2048 else 1


def test_route_by_length_and_switch(L):
    from nnmnkwii_amd import _hip
    import chirp_model as CM
    for n in LENGTHS:
        assert L.mlpg_hip_modspec_route(n) == _expected(n) == _hip.modspec_route(n), n
        assert (L.mlpg_hip_modspec_route(n) == 2) == CM.takes(n), n
    assert [L.mlpg_hip_modspec_route(n) for n in (2, 3, 64, 100, 2047, 2048, 2049, 4096, 4097)] == [0, 2, 0, 2, 2, 0, 1, 0, 1]
    L.mlpg_hip_modspec_set_direct(1)
    try:
        for n in LENGTHS:
            assert L.mlpg_hip_modspec_route(n) == (1 if n >= 2 else -1), n
    finally:
        L.mlpg_hip_modspec_set_direct(0)
    assert L.mlpg_hip_modspec_route(100) == 2
    # the padded-minibatch entries keep their own routes: the fused step still takes powers of two only
    assert L.mlpg_hip_modspec_loss_form(100) == 0 and L.mlpg_hip_modspec_loss_form(1024) == 1


def test_export_declaration_counter_and_abi(L):
    from nnmnkwii_amd import _hip
    assert "mlpg_hip_modspec_route" in _hip.EXPORTS and L.mlpg_hip_modspec_route is not None
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    assert re.search(r"\bint\s+mlpg_hip_modspec_route\s*\(\s*int\s+n\s*\)\s*;", header)
    assert L.mlpg_hip_launch_count(20) >= 0
    assert L.mlpg_hip_launch_count(21) == -1
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION


def test_refusals_at_a_chirp_length_come_before_the_runtime_is_touched(L):
    """Every call below carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    n = 100
    assert L.mlpg_hip_modspec_route(n) == 2
    c0 = _counts(L)

    def spec(device=0, x=fake, B=2, T=10, D=3, n=n, ms=fake, ph=fake):
        return L.mlpg_hip_modspec(device, None, x, B, T, D, n, 0, ms, ph)

    def inverse(device=0, ms=fake, ph=fake, B=2, D=3, n=n, x=fake):
        return L.mlpg_hip_inv_modspec(device, None, ms, ph, B, n, D, 0, x)

    def smooth(device=0, x=fake, B=2, T=10, D=3, n=n, out=fake):
        return L.mlpg_hip_modspec_smoothing(device, None, x, B, T, D, n, 0, 10, 1, out)

    def backward(device=0, x=fake, g=fake, B=2, T=10, D=3, n=n, gx=fake):
        return L.mlpg_hip_modspec_backward(device, None, x, g, B, T, D, n, 0, gx)

    with_T = [dict(B=-1), dict(T=-1), dict(D=-1), dict(T=n + 1), dict(device=99)]
    cases = [(spec, with_T + [dict(x=None), dict(ms=None)]),
             (inverse, [dict(B=-1), dict(D=-1), dict(device=99), dict(ms=None), dict(ph=None), dict(x=None)]),
             (smooth, with_T + [dict(x=None), dict(out=None)]),
             (backward, with_T + [dict(x=None), dict(g=None), dict(gx=None)])]
    for call, kws in cases:
        for kw in kws:
            rc = call(**kw)
            assert rc == -1 and L.mlpg_hip_last_error(), (call.__name__, kw, rc)
    assert _counts(L) == c0
    # empty batches are no-ops on this route as on the others
    assert spec(B=0, x=None, ms=None, ph=None) == 0 and smooth(D=0, x=None, out=None) == 0
    assert _counts(L) == c0
