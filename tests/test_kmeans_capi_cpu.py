"""CPU-side checks of the k-means entry points (-m "not gpu"): exports and declarations, refusals answered with fake pointers
before the runtime is touched, N == 0, the workspace formula, the ABI version and the launch-counter kinds."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mlpg_hip_kmeans_workspace_bytes", "mlpg_hip_kmeans_seed_step", "mlpg_hip_kmeans_lloyd_step")
fake = ctypes.c_void_p(64)
BIG = 1 << 40


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(28)]


def seed(L, device=0, X=fake, shift=fake, N=100, F=5, cand=fake, C=3, closest=fake, d=fake, pots=fake, ws=fake, ws_bytes=BIG):
    return L.mlpg_hip_kmeans_seed_step(device, None, X, shift, N, F, cand, C, closest, d, pots, ws, ws_bytes)


def lloyd(L, device=0, X=fake, shift=fake, centers=fake, prev=fake, N=100, F=5, K=3, update=1, labels=fake, min_dist=fake, sums=fake,
          counts=fake, out=fake, stats=fake, ws=fake, ws_bytes=BIG):
    return L.mlpg_hip_kmeans_lloyd_step(device, None, X, shift, centers, prev, N, F, K, update, labels, min_dist, sums, counts, out,
                                        stats, ws, ws_bytes)


def test_exports_declarations_counters_and_abi(L):
    from nnmnkwii_amd import _hip
    header = open(os.path.join(ROOT, "include", "mlpg_hip.h")).read()
    for name in NAMES:
        assert name in _hip.EXPORTS and getattr(L, name) is not None
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.mlpg_hip_abi_version() == 14 == _hip.ABI_VERSION
    assert L.mlpg_hip_launch_count(26) >= 0 and L.mlpg_hip_launch_count(27) >= 0
    assert L.mlpg_hip_launch_count(25) == -1 and L.mlpg_hip_launch_count(28) == -1


def _r(b):
    return (b + 255) // 256 * 256


def _slices(N):
    return max(1, min((N + 63) // 64, 1024))


def _expected_bytes(N, F, K):
    S = _slices(N)
    return _r(8 * 8 * S) + _r(8 * S * K * (F + 1)) + _r(8 * S) + _r(8 * S) + _r(8 * K)


def test_refusals_come_before_the_runtime_is_touched(L):
    """Every call carries fake pointers: one that got as far as a launch would fault.  No counter moves."""
    c0 = _counts(L)
    sizes = [dict(F=0), dict(F=129), dict(N=-1), dict(device=-1), dict(device=16)]
    cases = [(seed, sizes + [dict(C=0), dict(C=9), dict(X=None), dict(cand=None), dict(d=None), dict(pots=None), dict(ws=None),
                             dict(ws_bytes=_r(64 * _slices(100)) - 1), dict(ws=ctypes.c_void_p(68))]),
             (lloyd, sizes + [dict(K=0), dict(K=65), dict(X=None), dict(centers=None), dict(prev=None), dict(labels=None),
                              dict(sums=None), dict(counts=None), dict(out=None), dict(stats=None), dict(stats=ctypes.c_void_p(68)),
                              dict(ws=None), dict(ws_bytes=_expected_bytes(100, 5, 3) - 1), dict(ws=ctypes.c_void_p(68))])]
    for call, kws in cases:
        for kw in kws:
            rc = call(L, **kw)
            assert rc == -1 and L.mlpg_hip_last_error(), (call.__name__, kw, rc)
    assert seed(L, F=129) == -1 and b"[1, 128]" in L.mlpg_hip_last_error()
    assert lloyd(L, K=65) == -1 and b"[1, 64]" in L.mlpg_hip_last_error()
    assert seed(L, C=9) == -1 and b"[1, 8]" in L.mlpg_hip_last_error()
    assert lloyd(L, device=16) == -1 and b"kmeans_lloyd_step: bad device" in L.mlpg_hip_last_error()
    # N == 0 returns 0 and touches nothing (no pointer is looked at)
    assert seed(L, N=0, X=None, shift=None, cand=None, closest=None, d=None, pots=None, ws=None, ws_bytes=0) == 0
    assert lloyd(L, N=0, X=None, shift=None, centers=None, prev=None, labels=None, min_dist=None, sums=None, counts=None, out=None,
                 stats=None, ws=None, ws_bytes=0) == 0
    assert _counts(L) == c0


def test_workspace_size_follows_the_documented_formula(L):
    for N, F, K in [(1, 1, 1), (64, 3, 2), (65, 3, 2), (257, 6, 3), (1000, 33, 4), (230400, 50, 16), (5000, 128, 64), (10 ** 7, 16, 1),
                    (0, 3, 2)]:
        assert L.mlpg_hip_kmeans_workspace_bytes(N, F, K) == _expected_bytes(N, F, K), (N, F, K)
    # the number of slices is bounded: the workspace of the largest model stays below 128 MB whatever N
    assert L.mlpg_hip_kmeans_workspace_bytes(10 ** 9, 128, 64) < 1 << 27
    for N, F, K in [(-1, 3, 2), (10, 0, 2), (10, 129, 2), (10, 3, 0), (10, 3, 65)]:
        assert L.mlpg_hip_kmeans_workspace_bytes(N, F, K) == 0
    # the mixture's own workspace formula is untouched
    assert L.mlpg_hip_gmm_workspace_bytes(257, 6, 3) == _r(8 * 5) + _r(8 * 5 * 3 * 7) + _r(8 * 3) + _r(8 * 2 * 3 * 36)


def test_the_aligner_checks_its_start_option_without_a_device():
    from nnmnkwii_amd.preprocessing.alignment import IterativeDTWAligner
    assert IterativeDTWAligner().gmm_init == "sklearn" and IterativeDTWAligner(gmm="device").gmm_init == "sklearn"
    assert IterativeDTWAligner(gmm="device", gmm_init="kmeans-device").gmm_init == "kmeans-device"
    for kw in (dict(gmm_init="kmeans-device"), dict(gmm="sklearn", gmm_init="kmeans-device"), dict(gmm="device", gmm_init="kmeans")):
        with pytest.raises(ValueError):
            IterativeDTWAligner(**kw)
    with pytest.raises(TypeError):
        IterativeDTWAligner(3, None, 1, 100, 16, 0, "first", "device", "kmeans-device")      # keyword only
