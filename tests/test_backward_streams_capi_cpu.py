"""CPU-side checks (-m "not gpu") of mlpg_hip_backward_streams: every refusal is answered before a device is touched (the
pointers below are fakes: a call that got as far as a launch would fault), its launch counter (kind 15) exists while kinds 12
and 14 read -1, the export and the Python surface are there and the ABI version is still 14."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from nnmnkwii_amd.csrc import build as hip_build
    hip_build.build()
    from nnmnkwii_amd import _hip
    return _hip.lib()


WL = np.array([0, 1, 1, 0, 2], dtype=np.int32)
WU = np.array([0, 1, 1, 0, 2], dtype=np.int32)
WC = np.array([1.0, -0.5, 0.0, 0.5, 1.0, -2.0, 1.0, 1.0, 1.0, -8.0, 0.0, 8.0, -1.0])
MERLIN = [(0, 0, 60, 3, 0), (180, 60, 1, 3, 0), (183, 61, 1, 0, 0), (184, 62, 5, 3, 0)]      # ld_in 199, ld_out 67


def _call(L, streams=MERLIN, device=0, dtype=1, algo=0, var_mode=0, var=64, mean=64, y=64, grad_out=64, grad_mean=64, grad_var=64,
          status=True, B=2, Tmax=8, ld_in=199, ld_out=67, n_win=5, tables=True):
    from nnmnkwii_amd import _hip
    table = (_hip.StreamDesc * max(len(streams), 1))()
    for k, s in enumerate(streams):
        table[k] = _hip.StreamDesc(*s)
    st = np.zeros(max(B, 1) * 4096, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    f = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    rc = L.mlpg_hip_backward_streams(device, None, dtype, algo, f(mean), f(var), var_mode, ld_in, f(y), f(grad_out), ld_out, None,
                                     B, Tmax, len(streams), ctypes.addressof(table), n_win, p(WL) if tables else None,
                                     p(WU) if tables else None, p(WC) if tables else None, f(grad_mean), f(grad_var),
                                     p(st) if status else None)
    return rc, L.mlpg_hip_last_error().decode()


def _counts(L):
    return [L.mlpg_hip_launch_count(k) for k in range(16)]


def test_backward_streams_validates_without_gpu(L):
    c0 = _counts(L)
    cases = [
        (dict(dtype=7), "dtype"),
        (dict(algo=9), "algo"),
        (dict(var_mode=5), "var_mode"),
        (dict(var=0), "var"),                                            # per-frame variances without an array
        (dict(var_mode=2, var=0), "MLPG_HIP_VAR_UNIT"),                  # grad_var with unit variances
        (dict(status=False), "status"),                                  # grad_var needs status
        (dict(ld_in=198), "stream 3 does not fit"),                      # bap ends at column 199
        (dict(ld_out=66), "stream 3 does not fit"),
        (dict(streams=[(0, 0, 60, 3, 3)]), "does not fit"),              # windows 3..5 of 5
        (dict(streams=[(0, k, 1, 0, 0) for k in range(65)]), "64 streams"),
        (dict(tables=False), "window tables"),
        (dict(device=-1), "device"),
        (dict(device=99), "device"),
        (dict(B=-1), "negative"),
        (dict(grad_out=0), "NULL"),
        (dict(grad_mean=0), "NULL"),
        (dict(y=0), "NULL"),                                             # the trajectory is needed for grad_var
        (dict(mean=0), "NULL"),
        # a forced family one dynamic stream cannot take: the stream and the algo are named
        (dict(algo=5), "stream 0: MLPG_HIP_ALGO_CONST"),                 # per-frame variances
        (dict(algo=2, Tmax=4000), "stream 0: MLPG_HIP_ALGO_WAVE"),       # beyond 2048 frames
        (dict(algo=7), "stream 0: MLPG_HIP_ALGO_FIR"),
        (dict(algo=3, streams=[(0, 0, 4, 3, 0), (12, 4, 2, 2, 3)], ld_in=16, ld_out=6), "stream 1: MLPG_HIP_ALGO_STRIP"),  # extent 2
        (dict(algo=6, streams=[(0, 0, 4, 1, 0)], ld_in=4, ld_out=4), "stream 0: MLPG_HIP_ALGO_CHUNK"),                    # no dynamic window
    ]
    for kw, word in cases:
        rc, err = _call(L, **kw)
        assert rc == -1 and word in err, (kw, rc, err)
    assert _counts(L) == c0                                              # a refused call moves no counter
    # empty batches and tables
    assert _call(L, B=0)[0] == 0
    assert _call(L, Tmax=0)[0] == 0
    assert _call(L, streams=[])[0] == 0
    assert _call(L, streams=[(0, 0, 0, 3, 0), (5, 0, 0, 0, 0)])[0] == 0
    assert _call(L, B=0, algo=2, Tmax=4000)[0] == 0
    assert _counts(L) == c0


def test_launch_counter_kind_15(L):
    assert L.mlpg_hip_launch_count(15) >= 0 and L.mlpg_hip_launch_count(13) >= 0
    assert L.mlpg_hip_launch_count(12) == -1 and L.mlpg_hip_launch_count(14) == -1 and L.mlpg_hip_launch_count(16) == -1


def test_binding_and_autograd_surface(L):
    import os
    import re
    from nnmnkwii_amd import _hip
    assert "mlpg_hip_backward_streams" in _hip.EXPORTS and _hip.ABI_VERSION == L.mlpg_hip_abi_version() == 14
    assert callable(_hip.backward_streams) and callable(_hip.forward_streams)
    from nnmnkwii_amd import autograd as AF
    assert AF.MultiStreamMLPG is not None and callable(AF.multi_stream_mlpg)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mlpg_hip.h")).read()
    assert re.search(r"int mlpg_hip_backward_streams\(int device, void \*stream, int dtype, int algo,", hdr)


def test_stream_table_is_shared_by_forward_and_backward():
    """One builder for both calls: table order output columns, a window list shared by object packed once."""
    from nnmnkwii_amd import _hip
    w = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
    w2 = [(0, 0, np.array([1.0]))]
    table, wl, wu, wc, n_win, out_col = _hip._stream_table([(0, 3, w), (6, 2, None), (8, 1, w), (10, 2, w2)])
    assert n_win == 3 and out_col == 8 and wl.tolist() == [0, 1, 0] and wc.tolist() == [1.0, -0.5, 0.0, 0.5, 1.0]
    got = [(s.in_col, s.out_col, s.static_dim, s.num_windows, s.win_first) for s in table]
    assert got == [(0, 0, 3, 2, 0), (6, 3, 2, 0, 0), (8, 5, 1, 2, 0), (10, 6, 2, 1, 2)]
