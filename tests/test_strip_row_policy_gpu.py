"""The strip kernel with the cache policy of level 1's row loads chosen per frame (row_load_aux, csrc/mlpg_strip_impl.h) against
the oracle, forward and backward, at the suite's usual tolerances (tests/test_strip_gpu.py, tests/test_backward_routes_gpu.py).

A policy bit changes no value, so what can go wrong is the plumbing: a frame loaded by the wrong copy of level 1.  The interior
copy carries the per-frame policies, the EDGE copy clamps its rows and stays plain, and the lengths here put an utterance's end
at every place against a chunk (16 frames) or strip (64 frames) boundary, where a boundary frame is also a clamped one:
T = 1, 15, 16, 17, 63, 64, 65, 129, 257.  B = 3, sd = 60, standard windows (the STD instantiations) with per-frame variances;
float64 and float32; one ragged batch; one batch whose dynamic variances are 100 x / 1000 x tighter than the static ones (level 3
sweeps the whole utterance)."""
import numpy as np
import pytest

from cases import WINDOW_SETS
from oracle import mlpg as O
from oracle.grad64 import mlpg_grad64

pytestmark = pytest.mark.gpu

TOL64 = 1e-9          # forward, float64 (test_strip_gpu.py)
TOL32 = 5e-6          # forward, float32
GTOL64 = 1e-10        # backward, float64 in and out (test_backward_routes_gpu.py)
GTOL32 = 3e-6         # backward, float32 on either side
B, SD = 3, 60
TS = [1, 15, 16, 17, 63, 64, 65, 129, 257]
STD3 = WINDOW_SETS["std3"]


def _rel_err(y, ref):
    scale = np.abs(ref).max(axis=0, keepdims=True)
    scale = np.where(scale == 0, 1.0, scale)
    return float((np.abs(y.astype(np.float64) - ref.astype(np.float64)) / scale).max())


def _grad_err(grad, ref, lengths):
    """max over utterances of |grad - ref| / max|ref of that utterance|; rows at and past its length must be exactly 0."""
    grad = grad.astype(np.float64)
    pad = np.arange(grad.shape[1])[None, :] >= np.asarray(lengths)[:, None]
    assert not grad[pad].any(), "padding rows not zero"
    err = np.abs(grad - ref).max(axis=(1, 2))
    scale = np.abs(ref).max(axis=(1, 2))
    return float((err / np.where(scale > 0, scale, 1.0)).max())


def _check(m, v, go, lengths, what, dtypes=(np.float64, np.float32)):
    import torch
    from nnmnkwii_amd import _hip
    T = m.shape[1]
    lens = np.full(m.shape[0], T, dtype=np.int32) if lengths is None else lengths
    L = None if lengths is None else torch.from_numpy(lengths).cuda()
    for dt in dtypes:
        md, vd, gd = m.astype(dt), v.astype(dt), go.astype(dt)
        # references from the values the kernel is given, computed once per dtype
        yo, _, rc = O.mlpg_batch(md, vd, STD3, lens)
        assert rc == 0
        gref = mlpg_grad64(vd, gd, STD3, lens)
        mt, vt, gt = (torch.from_numpy(a).cuda() for a in (md, vd, gd))
        n0 = _hip.lib().mlpg_hip_launch_count(2)
        y, st = _hip.forward(mt, vt, STD3, L, algo=_hip.ALGO_STRIP)
        assert int(st.abs().max()) == 0
        y = y.cpu().numpy()
        e = _rel_err(y.reshape(-1, SD), yo.reshape(-1, SD))
        print(what, dt.__name__, "forward rel err %.3e" % e)
        assert e <= (TOL64 if dt == np.float64 else TOL32), (what, dt.__name__, e)
        for b in range(m.shape[0]):
            assert not y[b, lens[b]:].any()
        outs = (torch.float64, torch.float32) if dt == np.float64 else (torch.float32,)
        for od in outs:
            g, sb = _hip.backward(vt, gt, STD3, 3 * SD, L, out_dtype=od, algo=_hip.ALGO_STRIP)
            assert int(sb.abs().max()) == 0
            ge = _grad_err(g.cpu().numpy(), gref, lens)
            print(what, dt.__name__, "->", od, "backward rel err %.3e" % ge)
            assert ge <= (GTOL64 if (dt == np.float64 and od == torch.float64) else GTOL32), (what, dt.__name__, od, ge)
        assert _hip.lib().mlpg_hip_launch_count(2) - n0 == 1 + len(outs)  # every launch was a strip launch


def _data(seed, T):
    rng = np.random.RandomState(seed)
    return rng.randn(B, T, 3 * SD), rng.rand(B, T, 3 * SD) + 0.1, rng.randn(B, T, SD)


@pytest.mark.parametrize("T", TS)
def test_every_end_against_a_chunk_or_strip_boundary(T):
    m, v, go = _data(4000 + T, T)
    _check(m, v, go, None, "T=%d" % T)


def test_ragged_lengths():
    """One batch, Tmax = 257: ends on a strip boundary, one past a chunk boundary, and a one-frame utterance (strips of padding)."""
    m, v, go = _data(4501, 257)
    _check(m, v, go, np.array([257, 64, 17], dtype=np.int32), "ragged")
    _check(m, v, go, np.array([129, 1, 255], dtype=np.int32), "ragged2", dtypes=(np.float64,))


def test_tight_dynamic_variances():
    """Delta / delta-delta variances 100 x / 1000 x tighter: the strips wait for the whole utterance (5 strips at T = 257)."""
    m, v, go = _data(4502, 257)
    v[:, :, SD:2 * SD] *= 1e-2
    v[:, :, 2 * SD:] *= 1e-3
    _check(m, v, go, np.array([257, 256, 65], dtype=np.int32), "tight")
