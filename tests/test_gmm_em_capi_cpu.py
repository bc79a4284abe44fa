"""CPU-side checks of the mixture entry points (-m "not gpu"): exports and declarations, refusals answered with fake pointers
before the runtime is touched, N == 0, the workspace size, the ABI version and the launch-counter kinds."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mlpg_hip_gmm_workspace_bytes", "mlpg_hip_gmm_estep", "mlpg_hip_gmm_mstep", "mlpg_hip_gmm_precisions")
fake = ctypes.c_void_p(64)
BIG = 1 << 40


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(25)]


def estep(L, device=0, X=fake, w=fake, mu=fake, U=fake, ld=fake, N=100, F=5, K=3, resp=fake, mean=fake, ws=fake, ws_bytes=BIG):
    return L.mlpg_hip_gmm_estep(device, None, X, w, mu, U, ld, N, F, K, resp, None, None, mean, ws, ws_bytes)


def mstep(L, device=0, X=fake, resp=fake, N=100, F=5, K=3, reg=1e-6, w=fake, mu=fake, cov=fake, ws=fake, ws_bytes=BIG):
    return L.mlpg_hip_gmm_mstep(device, None, X, resp, N, F, K, reg, w, mu, cov, ws, ws_bytes)


def precisions(L, device=0, cov=fake, F=5, K=3, U=fake, ld=fake, status=fake):
    return L.mlpg_hip_gmm_precisions(device, None, cov, F, K, U, ld, status)


def test_exports_declarations_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(21) == -1
    assert all(L.mlpg_hip_launch_count(k) >= 0 for k in (22, 23, 24))
    assert L.mlpg_hip_launch_count(25) == -1


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    sizes = [dict(F=0), dict(F=129), dict(K=0), dict(K=65), dict(N=-1), dict(device=-1), dict(device=16)]
    need = L.mlpg_hip_gmm_workspace_bytes(100, 5, 3)
    cases = [(estep, sizes + [dict(X=None), dict(w=None), dict(mu=None), dict(U=None), dict(ld=None), dict(ws=None),
                              dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(68))]),
             (mstep, sizes + [dict(X=None), dict(resp=None), dict(w=None), dict(mu=None), dict(cov=None), dict(ws=None),
                              dict(ws_bytes=need - 1), dict(reg=-1.0), dict(reg=float("nan"))]),
             (precisions, [dict(F=0), dict(F=129), dict(K=0), dict(K=65), dict(device=99), dict(cov=None), dict(U=None),
                           dict(ld=None), dict(status=None)])]
    for call, kws in cases:
        for kw in kws:
            rc = call(L, **kw)
            assert rc == -1 and L.mlpg_hip_last_error(), (call.__name__, kw, rc)
    assert estep(L, F=129) == -1 and b"[1, 128]" in L.mlpg_hip_last_error()
    assert mstep(L, K=65) == -1 and b"[1, 64]" in L.mlpg_hip_last_error()
    assert estep(L, device=16) == -1 and b"gmm_estep: bad device" in L.mlpg_hip_last_error()
    # N == 0 returns 0 and touches nothing (no pointer is looked at)
    assert estep(L, N=0, X=None, w=None, mu=None, U=None, ld=None, resp=None, mean=None, ws=None, ws_bytes=0) == 0
    assert mstep(L, N=0, X=None, resp=None, w=None, mu=None, cov=None, ws=None, ws_bytes=0) == 0
    assert _counts(L) == c0


def _slices(N, F, K):
    return max(1, min((N + 255) // 256, max(1, 2048 // (K * ((F + 15) // 16)))))


def _expected_bytes(N, F, K):
    r = lambda b: (b + 255) // 256 * 256  # noqa: E731
    S, S1 = _slices(N, F, K), max(1, min((N + 63) // 64, 1024))
    return r(8 * ((N + 63) // 64)) + r(8 * S1 * K * (F + 1)) + r(8 * K) + r(8 * S * K * F * F)


def test_workspace_size_follows_the_slice_rule(L):
    for N, F, K in [(1, 1, 1), (257, 6, 3), (1000, 33, 4), (230400, 50, 16), (5000, 128, 64), (10 ** 7, 16, 1), (0, 3, 2)]:
        assert L.mlpg_hip_gmm_workspace_bytes(N, F, K) == _expected_bytes(N, F, K), (N, F, K)
    # the number of slices depends on (N, F, K) alone and is bounded: the workspace of the largest model stays below 1 GB
    assert L.mlpg_hip_gmm_workspace_bytes(10 ** 8, 128, 64) < 1 << 30
    for N, F, K in [(-1, 3, 2), (10, 0, 2), (10, 129, 2), (10, 3, 0), (10, 3, 65)]:
        assert L.mlpg_hip_gmm_workspace_bytes(N, F, K) == 0


def test_the_row_bound_is_the_grids_thread_limit(L):
    """The E-step takes one workgroup of 256 threads per 64 rows, and a grid is 32 bits of threads: 2^24 - 1 workgroups, 2^30 - 64
    rows.  At the bound the call passes the row check (the next refusal, the device's, answers); one row more is refused with the
    limit named -- by the E-step, by the M-step that shares the rule, and by the workspace size.  Fake pointers, no counter moves."""
    c0 = _counts(L)
    most = ((1 << 24) - 1) * 64
    for f in (estep, mstep):
        assert f(L, N=most, device=16) == -1 and b"bad device" in L.mlpg_hip_last_error()
        assert f(L, N=most + 1, device=16) == -1
        err = L.mlpg_hip_last_error()
        assert b"16777215 workgroups of 256 threads" in err and b"bad device" not in err, err
    assert L.mlpg_hip_gmm_workspace_bytes(most, 5, 3) > 0 and L.mlpg_hip_gmm_workspace_bytes(most + 1, 5, 3) == 0
    assert _counts(L) == c0
