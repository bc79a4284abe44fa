"""GPU tests (-m gpu): a row index past 2^31.  One float32 parent with D = ld = 1, B = 65537 utterances of Tmax = 32768 frames:
2^31 + 32768 rows, 8 GiB + 128 KiB (tests/far.py).  The live utterances are 0, 65535 and 65536: utterance 65535 ends exactly at
row 2^31 and utterance 65536 begins there, so a row index (b * Tmax + t) kept in 32 bits wraps to rows of utterance 0 -- which
are live, hold other numbers, and in the in-place call must keep the bits the model gives them.  mlpg_hip_column_stats,
mlpg_hip_column_affine (in place) and mlpg_hip_gv; the result must be the model's (tools/norm_model.py, the gv model).  The last
test prints which boundaries each entry's array crossed and fails unless each crossed all three."""
import numpy as np
import pytest
import torch

import far
import gvmlpg_cases as GC
import norm_cases as C
from far import FarParent
from norm_cases import NM
from test_far_rows_gpu import bits, dev, far_test
from test_norm_gpu import same_bits

pytestmark = pytest.mark.gpu

B, T = 65537, 32768
LIVE = np.array([0, 65535, 65536])
LENS = np.array([T, T, T - 5], dtype=np.int32)
ALL = {"2^31 bytes", "2^32 bytes", "2^31 elements"}
COVER = {}                                          # (entry, array argument) -> boundaries crossed


def _parent():
    p = FarParent((B, T, 1), np.float32, low_guard_bytes=far.low_guard_for(B * T * 4))
    assert p.lo == 1 << 31
    return p


def _data(seed):
    rng = np.random.RandomState(seed)
    X = (rng.randn(3, T, 1) * np.array([1.0, 3.0, 0.5])[:, None, None] + np.array([0.0, 5.0, -2.0])[:, None, None]).astype(np.float32)
    X[2, T - 5:] = np.nan                                                # the padding of the last utterance
    return X


def _lengths():
    L = torch.zeros(B, dtype=torch.int32, device="cuda")
    L[torch.from_numpy(LIVE).cuda()] = torch.from_numpy(LENS).cuda()
    return L


def _place(p, X, entry, arg="x"):
    for i, b in enumerate(LIVE):
        p.place(int(b), T, 0, X[i])
    COVER[(entry, arg)] = p.crossed()
    first, _ = p.span(p.regions[-1])
    assert first == (1 << 31) * 4                                        # utterance 65536 begins at row 2^31


def sparse_kernel_state(X, lens, B=B, T=T, live=LIVE):
    """tools/norm_model.py's kernel_state for the (B, T, 1) batch whose live utterances `live` are X: the partials of a dead
    utterance are the empty state, which merge() hands through unchanged, so finish() over B * ceil(T / 512) partials is
    finish() over the live ones in their segments."""
    nblk = -(-T // NM.BLOCK_ROWS)
    P = B * nblk
    per = -(-P // NM.FIN_SEG)
    e = NM.empty_state(1)
    assert same_bits(NM.merge(e, NM.block_partial(X[0, :7])), NM.block_partial(X[0, :7]))
    assert same_bits(NM.merge(NM.block_partial(X[0, :7]), e), NM.block_partial(X[0, :7]))
    seg = [NM.empty_state(1) for _ in range(NM.FIN_SEG)]
    for i, b in enumerate(live):
        for j in range(nblk):
            t0 = j * NM.BLOCK_ROWS
            part = NM.block_partial(X[i, t0:max(t0, min(t0 + NM.BLOCK_ROWS, int(lens[i])))])
            q = (int(b) * nblk + j) // per
            seg[q] = NM.merge(seg[q], part)
    h = 1
    while h < NM.FIN_SEG:
        for q in range(0, NM.FIN_SEG, 2 * h):
            seg[q] = NM.merge(seg[q], seg[q + h])
        h *= 2
    return seg[0]


def test_the_sparse_form_of_the_model_is_the_model():
    """On a batch small enough for kernel_state itself: live utterances first, last and in the middle of dead ones."""
    b, t, live, lens = 300, 700, np.array([0, 151, 299]), np.array([700, 513, 1])
    X = np.random.RandomState(1).randn(3, t, 1).astype(np.float32)
    full = np.full((b, t, 1), np.nan, dtype=np.float32)
    full[live] = X
    L = np.zeros(b, dtype=np.int32)
    L[live] = lens
    assert same_bits(sparse_kernel_state(X, lens, b, t, live), NM.kernel_state(full, L))


@far_test
def test_column_stats_past_row_2_31():
    from nnmnkwii_amd import _hip
    X = _data(1)
    p = _parent()
    _place(p, X, "column_stats")
    state = _hip.column_stats(p.view, _lengths()).cpu().numpy()
    model = sparse_kernel_state(X, LENS)
    assert same_bits(state, model), (state, model)
    truth = NM.exact(X, LENS)
    count, mean, var, mn, mx = NM.stats_of(state)
    assert count == truth["count"] == int(LENS.sum())
    assert max(NM.ratios(mean, var, truth)) <= C.BOUND_RATIO                # tests/test_norm_gpu.py
    assert p.untouched() == []
    p.free()


@far_test
def test_column_affine_in_place_past_row_2_31():
    from nnmnkwii_amd import _hip
    X = _data(2)
    p = _parent()
    _place(p, X, "column_affine", "x = y")
    for b in LIVE:
        p.expect_written(int(b), T, 0, 1)
    a, c = np.array([1.75]), np.array([-0.375])
    r = _hip.column_affine(p.view, dev(a), dev(c), 1, _lengths(), p.view)
    torch.cuda.synchronize()
    assert r.data_ptr() == p.view.data_ptr()
    got = np.stack([p.read(int(b), T, 0, 1) for b in LIVE])
    assert same_bits(got, NM.affine(X, a, c, 1, LENS, np.float32))
    assert not got[2, T - 5:].any()
    assert p.untouched(rest=0) == []                                        # every row of a dead utterance: exact zeros
    p.free()


@far_test
def test_gv_past_row_2_31():
    from nnmnkwii_amd import _hip
    X = _data(3)
    p = _parent()
    _place(p, X, "gv")
    g = _hip.gv(p.view, _lengths())
    sel = torch.from_numpy(LIVE).cuda()
    gl = g[sel].cpu().numpy()
    ref = GC.GV.gv_padded(np.nan_to_num(X), LENS)
    assert np.abs(gl - ref).max() <= 4 * T * GC.EPS * float(np.nanmax(np.abs(X))) ** 2      # tests/test_gvmlpg_gpu.py
    compact = _hip.gv(dev(X), dev(LENS)).cpu().numpy()
    assert bits(gl) == bits(compact)                                        # a system's bits do not depend on the batch
    g[sel] = 0.0
    assert not bool(g.any()), "the gv of a dead utterance is not zero"
    assert p.untouched() == []
    p.free()


def test_every_array_crossed_every_boundary():
    """The table (entry, array argument) -> boundaries crossed, built from FarParent.crossed() as the tests above ran."""
    print()
    for entry, arg in (("column_stats", "x"), ("column_affine", "x = y"), ("gv", "x")):
        got = COVER.get((entry, arg), set())
        print("%-16s %-6s %s" % (entry, arg, ", ".join(sorted(got)) or "-"))
        assert got == ALL, (entry, arg, sorted(ALL - got))
