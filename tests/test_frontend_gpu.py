"""Frame expansion on the device: nnmk_frontend_expand and nnmk_frontend_frame_counts (csrc/frame_expand.hip) against the
specification tools/frontend_model.py through the C entry on guarded buffers -- payloads at odd element offsets, inputs
snapshotted, the phone rows and durations at or past num_phones holding NaN (or absurd integers), the phone matrix's extra
columns holding NaN, the output pre-filled with a poison byte -- then ``nnmnkwii_amd.frontend.merlin`` on CUDA tensors and numpy
arrays against what the reference gave (tests/golden/frontend_ref.npz).

No tolerance anywhere: every operation is one correctly rounded IEEE operation on both sides, so the comparisons are
``np.array_equal`` (and bytes, where padding and untouched columns are concerned)."""
import ctypes
import functools
import gc
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import far
from embed import Embedded, embedded, failed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frontend_model as FM  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCK = FM.BLOCK_ROWS
G = np.load(os.path.join(ROOT, "tests", "golden", "frontend_ref.npz"))
DUR_DTYPES = (np.int32, np.int64, np.float32, np.float64)
DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}
POISON = 0xA5
BOUNDARY_T = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3)

p = lambda b: None if b is None else ctypes.c_void_p(b.ptr())  # noqa: E731


def _lib():
    from nnmnkwii_amd import _frontend_hip, _metrics_hip
    _metrics_hip.lib()
    return _frontend_hip.lib()


def _counts():
    L = _lib()
    return [L.mlpg_hip_launch_count(k) for k in range(44)] + [L.nnmk_metrics_launch_count(), L.nnmk_frontend_launch_count()]


@functools.lru_cache(maxsize=None)
def cc_table():
    return FM.coarse_coding_table()


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def draw_frames(rng, Nmax, S, target):
    """(Nmax, S) frames per state that add up to `target`: small counts, zero-length states at the start, in the middle and at
    the end of phones, the rest of the target in one state."""
    r = rng.randint(0, 4, size=(Nmax, S))
    r[rng.rand(Nmax, S) < 0.3] = 0
    flat = r.reshape(-1)
    k = flat.size
    while flat.sum() > target:
        k -= 1
        flat[k] = 0
    flat[rng.randint(flat.size)] += target - flat.sum()
    assert flat.sum() == target
    return r


def encode(rng, r, dtype):
    """Durations of `dtype` that give the frames r with min_frames 0: halves that round to even, quarters, negatives and NaN
    for 0."""
    r = np.asarray(r, dtype=np.int64)
    if np.dtype(dtype).kind == "i":
        d = r.copy()
        d[(r == 0) & (rng.rand(*r.shape) < 0.5)] = -3
        return d.astype(dtype)
    even = r % 2 == 0
    u = rng.rand(*r.shape)
    d = r + np.where(even, np.where(u < 0.4, 0.5, np.where((u < 0.8) & (r > 0), -0.5, 0.0)), np.where(u < 0.5, 0.25, -0.25))
    zero = (r == 0) & (u > 0.8)
    d[zero] = np.where(rng.rand(int(zero.sum())) < 0.5, np.nan, -3.0)
    d = d.astype(dtype)
    assert np.array_equal(FM.frames(d, 0), r)
    return d


def make_case(seed, B, Nmax, S, Dl, targets, dur_dtype, num_phones=None):
    """P (B, Nmax, Dl) float64 and durations (B, Nmax, S) of dur_dtype whose live phones add up to targets[b] frames; the rows and
    durations at or past num_phones[b] hold NaN / absurd values: read, they would show in the output or in the counts."""
    rng = np.random.RandomState(seed)
    P = np.round(rng.randn(B, Nmax, Dl) * 4) / 4 + (rng.rand(B, Nmax, Dl) < 0.3) * rng.rand(B, Nmax, Dl)
    n = np.full(B, Nmax, dtype=np.int32) if num_phones is None else np.asarray(num_phones, dtype=np.int32)
    r = np.zeros((B, Nmax, S), dtype=np.int64)
    for b in range(B):
        m = int(np.clip(n[b], 0, Nmax))
        if m:
            r[b, :m] = draw_frames(rng, m, S, targets[b])
    d = encode(rng, r, dur_dtype)
    for b in range(B):
        m = int(np.clip(n[b], 0, Nmax))
        P[b, m:] = np.nan
        d[b, m:] = 1000000 if np.dtype(dur_dtype).kind == "i" else np.nan
    return P, d, (None if num_phones is None else n)


def run_expand(P, d, n, kind, min_frames, affine, p_dtype, out_dtype, Tmax=None, pad_p=0, pad_out=0, off=1, seed=0):
    """One call of nnmk_frontend_frame_counts and one of nnmk_frontend_expand on guarded buffers, compared with the model.
    Returns (out (B, Tmax, Dl + F), lengths)."""
    from nnmnkwii_amd import _hip
    L = _lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    name = FM.KINDS[kind]
    B, Nmax, Dl = P.shape
    S = d.shape[2]
    F = FM.SIZES[kind]
    W = Dl + F
    P = P.astype(p_dtype)
    rng = np.random.RandomState(seed + 7)
    scale_, min_ = (rng.rand(W) + 0.5, rng.randn(W)) if affine else (None, None)
    want, want_len, want_counts = FM.frame_features_batch(P, d, n, name, min_frames, scale_, min_, Tmax, out_dtype, cc_table())
    Tmax = want.shape[1]
    Pw = np.concatenate([P, np.full((B, Nmax, pad_p), np.nan, dtype=p_dtype)], axis=2)
    ins = dict(phone=embedded(Pw, off), durations=embedded(d, off + 2))
    if n is not None:
        ins["num_phones"] = embedded(n, off)
    if kind == FM.COARSE_CODING:
        ins["cc"] = embedded(cc_table(), off)
    if affine:
        ins["scale_"], ins["min_"] = embedded(scale_, off), embedded(min_, off + 1)
    out = Embedded((B, Tmax, W + pad_out), out_dtype, off, fill_byte=POISON)
    lengths = Embedded((B,), np.int32, off, fill_byte=POISON)
    counts = Embedded((B,), np.int64, off, fill_byte=POISON)
    c0 = _counts()
    rc = L.nnmk_frontend_frame_counts(dev.index, _hip._stream(dev), DT_CODE[d.dtype], p(ins["durations"]), p(ins.get("num_phones")), B, Nmax, S,
                                      min_frames, p(counts))
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    rc = L.nnmk_frontend_expand(dev.index, _hip._stream(dev), DT_CODE[np.dtype(p_dtype)], p(ins["phone"]), Dl + pad_p, DT_CODE[d.dtype],
                                p(ins["durations"]), p(ins.get("num_phones")), B, Nmax, S, Dl, min_frames, kind, p(ins.get("cc")),
                                p(ins.get("scale_")), p(ins.get("min_")), DT_CODE[np.dtype(out_dtype)], p(out), W + pad_out, Tmax, p(lengths))
    torch.cuda.synchronize()
    moved = [b - a for a, b in zip(c0, _counts())]
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    assert moved[-1] == 1 and sum(moved) == 1, moved                      # counted once, and nothing else counted
    bad = failed(ins, dict(out=out, lengths=lengths, counts=counts))
    assert not bad, bad
    got = out.host()
    assert np.array_equal(counts.host(), want_counts) and np.array_equal(lengths.host(), want_len)
    assert np.array_equal(got[:, :, :W], want), ("rows", name, np.argwhere(got[:, :, :W] != want)[:5])
    for b in range(B):
        assert not got[b, want_len[b]:, :W].any(), ("pad rows not zero", b)
    if pad_out and got.size:
        assert (np.frombuffer(np.ascontiguousarray(got[:, :, W:]).tobytes(), dtype=np.uint8) == POISON).all(), "a column at or past Dl + F was written"
    return got[:, :, :W], lengths.host()


# ---- the shapes: every B, Nmax, S and Dl with every other; the other choices rotate through them --------------------------------

SHAPES = list(itertools.product((1, 3, 5), (1, 7), (1, 5), (1, 3, 416, 419)))


def targets_of(B, k):
    """The frames of the B utterances: the block boundaries, an utterance of num_phones 0 ("none"), one whose durations are all 0."""
    t = BOUNDARY_T[k % 4]
    return {1: [t], 3: [t, "none", BOUNDARY_T[(k + 1) % 4]], 5: [BOUNDARY_T[(k + 1) % 4], 0, t, "none", 1]}[B]


@pytest.mark.parametrize("B,Nmax,S,Dl", SHAPES)
def test_kernel_against_the_model(B, Nmax, S, Dl):
    k = SHAPES.index((B, Nmax, S, Dl))
    kind = 1 + k % 7 if k % 8 else 0
    targets = targets_of(B, k)
    n = None if B == 1 else [0 if t == "none" else (Nmax if i % 2 else Nmax + 3) for i, t in enumerate(targets)]   # (above Nmax: clamped)
    frames = [0 if t == "none" else t for t in targets]
    P, d, n = make_case(1000 + k, B, Nmax, S, Dl, frames, DUR_DTYPES[k % 4], n)
    dts = [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)][(k // 4) % 4]
    longest = max(frames)
    out, lengths = run_expand(P, d, n, kind, 0, affine=bool((k // 2) % 2), p_dtype=dts[0], out_dtype=dts[1],
                              Tmax=None if k % 3 else longest + 5, pad_p=(0, 2)[k % 2], pad_out=(0, 3, 0, 1)[(k // 3) % 4], off=1 + 2 * (k % 2), seed=k)
    assert lengths.tolist() == frames


@pytest.mark.parametrize("kind", range(8), ids=[str(k) for k in FM.KINDS])
@pytest.mark.parametrize("dur_dtype", DUR_DTYPES, ids=[np.dtype(t).name for t in DUR_DTYPES])
def test_every_kind_with_every_duration_dtype(kind, dur_dtype):
    """Both min_frames (0, and 1: every state of a live phone then has at least a frame), with and without the affine map, a
    phone of one frame, float32 and float64 on either side."""
    k = kind * 4 + DUR_DTYPES.index(dur_dtype)
    P, d, n = make_case(2000 + k, 3, 7, 5, 3, [BLOCK + 1, 9, 2 * BLOCK + 3], dur_dtype, [7, 3, 6])
    d[1, 0] = 0
    d[1, 0, 2] = 1                                                  # a phone of one frame
    for mf in (0, 1):
        run_expand(P, d, n, kind, mf, affine=bool((k + mf) % 2), p_dtype=(np.float32, np.float64)[k % 2], out_dtype=(np.float64, np.float32)[(k // 2) % 2],
                   pad_out=k % 3, seed=k)


def test_the_halves_and_the_rest_of_the_rounding():
    d = np.array([[[0.5, 1.5, 2.5, -3.0, np.nan]], [[3.5, 4.5, np.inf, 0.49, 0.51]]])
    P = np.arange(2.0).reshape(2, 1, 1)
    assert FM.frames(d, 0).tolist() == [[[0, 2, 2, 0, 0]], [[4, 4, FM.MAX_FRAMES, 0, 1]]]
    d[1, 0, 2] = 2.75
    for dt in (np.float64, np.float32):
        _, lengths = run_expand(P, d.astype(dt), None, FM.FULL, 0, False, np.float64, np.float64)
        assert lengths.tolist() == [4, 12]
        _, lengths = run_expand(P, d.astype(dt), None, FM.FULL, 1, False, np.float64, np.float64)
        assert lengths.tolist() == [7, 13]
    i = np.array([[[0, 1, -3, 2, 0]], [[5, 0, 0, 0, 1]]])
    for dt in (np.int32, np.int64):
        _, lengths = run_expand(P, i.astype(dt), None, FM.FULL, 0, False, np.float64, np.float64)
        assert lengths.tolist() == [3, 6]
        _, lengths = run_expand(P, i.astype(dt), None, FM.FULL, 2, False, np.float64, np.float64)
        assert lengths.tolist() == [10, 13]


@pytest.mark.parametrize("kind", [FM.FULL, FM.COARSE_CODING])
def test_truncation(kind):
    """Tmax one below the need, and in the middle of a block: the rows that fit are right, nothing beyond them is written (the
    guards), lengths_out = Tmax."""
    P, d, n = make_case(3000 + kind, 3, 7, 5, 3, [2 * BLOCK + 3, 5, BLOCK], np.int32)
    full, _ = run_expand(P, d, n, kind, 0, True, np.float32, np.float32, pad_out=2)
    for Tmax in (2 * BLOCK + 2, BLOCK, BLOCK - 1, 1, 0):
        cut, lengths = run_expand(P, d, n, kind, 0, True, np.float32, np.float32, Tmax=Tmax, pad_out=2)
        assert np.array_equal(cut, full[:, :Tmax]) and lengths.tolist() == [min(t, Tmax) for t in (2 * BLOCK + 3, 5, BLOCK)]


def test_empty_batches():
    P, d, n = make_case(3100, 3, 7, 5, 3, [0, 0, 0], np.float64, [0, 0, 0])
    out, lengths = run_expand(P, d, n, FM.FULL, 1, False, np.float64, np.float64)          # num_phones 0 everywhere: Tmax 0
    assert out.shape == (3, 0, 12) and lengths.tolist() == [0, 0, 0]
    out, lengths = run_expand(P, d, n, FM.FULL, 1, False, np.float64, np.float64, Tmax=BLOCK + 1, pad_out=1)
    assert not out.any() and lengths.tolist() == [0, 0, 0]
    out, lengths = run_expand(P[:, :0], d[:, :0], None, FM.FULL, 0, False, np.float64, np.float64, Tmax=3)     # Nmax 0
    assert not out.any() and lengths.tolist() == [0, 0, 0]
    L = _lib()
    c0 = _counts()
    assert L.nnmk_frontend_expand(0, None, 0, None, 3, 2, None, None, 0, 7, 5, 3, 0, 1, None, None, None, 0, None, 12, 9, None) == 0     # B 0
    assert _counts() == c0


def test_the_largest_utterance_the_entry_accepts():
    """Nmax * S = NNMK_FRONTEND_MAX_STATES: every thread of the scan takes 32 states."""
    rng = np.random.RandomState(3200)
    Nmax, S = FM.MAX_STATES // 8, 8
    d = (rng.rand(2, Nmax, S) < 0.01).astype(np.int32)
    d[1, Nmax - 1, S - 1] = 3
    P = rng.randn(2, Nmax, 2)
    out, lengths = run_expand(P, d, np.array([Nmax, Nmax - 1], dtype=np.int32), FM.FULL, 0, False, np.float32, np.float32)
    assert lengths.tolist() == [int(d[0].sum()), int(d[1, :Nmax - 1].sum())] and min(lengths) > BLOCK


# ---- the public functions ---------------------------------------------------------------------------------------------------------

STATE_KINDS = ("full", "minimal_frame", "state_only", "frame_only", "uniform_state", "coarse_coding")
GOLDEN = [(g, k) for g in ("state", "state2") for k in STATE_KINDS] + [(g, k) for g in ("phone", "phone2") for k in ("minimal_phoneme", "coarse_coding")]


def reference_matrix(group, kind):
    return np.concatenate([G["P"][G[group + "/phone"]], G["%s/%s" % (group, kind)]], axis=1)


@pytest.mark.parametrize("group,kind", GOLDEN)
def test_the_reference_s_matrix_through_the_public_functions(group, kind):
    from nnmnkwii_amd.frontend import merlin as fe
    L = _lib()
    ref = reference_matrix(group, kind)
    P, d = G["P"], G[group + "/dur"]
    c0 = L.nnmk_frontend_launch_count()
    a = fe.frame_features(P, d, kind)                                                     # numpy in, numpy out
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and np.array_equal(a, ref)
    a32 = fe.frame_features(P, d, kind, dtype=np.float32)
    assert a32.dtype == np.float32 and np.array_equal(a32, ref.astype(np.float32))
    Pd, dd = torch.from_numpy(P).cuda(), torch.from_numpy(d).cuda()
    t = fe.frame_features(Pd, dd, kind)                                                   # CUDA tensors in, CUDA tensor out
    assert t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), ref)
    t32 = fe.frame_features(Pd.float(), dd.to(torch.float32) + 0.25, kind, min_frames=0)  # float durations that round to the same frames
    assert t32.dtype == torch.float32 and np.array_equal(t32.cpu().numpy(), ref.astype(np.float32))
    assert L.nnmk_frontend_launch_count() - c0 == 4                                       # one launch of the expansion each
    # in a batch: beside a shorter utterance, into a column slice of a wider tensor, with the affine map
    W = ref.shape[1]
    rng = np.random.RandomState(11)
    scale_, min_ = rng.rand(W) + 0.5, rng.randn(W)
    Pb, db = torch.stack([Pd, Pd]), torch.stack([dd, dd])
    n = torch.tensor([40, 13], dtype=torch.int32, device="cuda")
    short = FM.frame_features(P[:13], d[:13], kind)
    out, lengths = fe.frame_features_batch(Pb, db, n, kind)
    assert out.shape == (2, len(ref), W) and lengths.dtype == torch.int32 and lengths.tolist() == [len(ref), len(short)]
    o = out.cpu().numpy()
    assert np.array_equal(o[0], ref) and np.array_equal(o[1, :len(short)], short) and not o[1, len(short):].any()
    wide = torch.full((2, len(ref) + 2, W + 5), -7.0, dtype=torch.float32, device="cuda")
    view = wide[:, :, 2:2 + W]
    got, lengths = fe.frame_features_batch(Pb, db, n, kind, scale_=scale_, min_=min_, out=view)
    assert got.data_ptr() == view.data_ptr() and lengths.tolist() == [len(ref), len(short)]
    w = wide.cpu().numpy()
    assert np.array_equal(w[0, :len(ref), 2:2 + W], (ref * scale_ + min_).astype(np.float32)) and not w[0, len(ref):, 2:2 + W].any()
    assert np.array_equal(w[1, :len(short), 2:2 + W], (short * scale_ + min_).astype(np.float32)) and not w[1, len(short):, 2:2 + W].any()
    assert (w[:, :, :2] == -7).all() and (w[:, :, 2 + W:] == -7).all()
    nb, ln = fe.frame_features_batch(np.stack([P, P]), np.stack([d, d]), np.array([40, 13]), kind, scale_=scale_, min_=min_)     # numpy
    assert isinstance(nb, np.ndarray) and ln.tolist() == [len(ref), len(short)] and np.array_equal(nb[0], ref * scale_ + min_)


def test_strict_raises_on_truncation_and_lenient_reports_it():
    from nnmnkwii_amd.frontend import merlin as fe
    P, d = torch.from_numpy(G["P"]).cuda()[None], torch.from_numpy(G["state/dur"]).cuda()[None]
    Pb, db = torch.cat([P, P]), torch.cat([d, d])
    n = torch.tensor([13, 40], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="utterance 1 has 615 frames, Tmax is 614"):
        fe.frame_features_batch(Pb, db, n, "full", Tmax=614)
    out = torch.empty((2, 614, 425), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="utterance 1 has 615 frames"):
        fe.frame_features_batch(Pb, db, n, "full", out=out)
    got, lengths = fe.frame_features_batch(Pb, db, n, "full", Tmax=614, strict=False)
    ref = reference_matrix("state", "full")
    assert lengths.tolist() == [int(G["state/dur"][:13].sum()), 614] and np.array_equal(got[1].cpu().numpy(), ref[:614])
    got, lengths = fe.frame_features_batch(Pb, db, n, "full", Tmax=700)                 # strict, and it fits
    assert got.shape == (2, 700, 425) and lengths.tolist()[1] == 615 and not got[1, 615:].any()


# ---- a row beyond 4 GiB -----------------------------------------------------------------------------------------------------------

def test_a_row_past_4_gib_from_the_pointer():
    """B = 1, three frames, and a row stride that puts the second row past 2^31 bytes and the third past 2^32 bytes from the
    pointer.  The rows are right and no other byte of the 6 GiB parent or of its guards changed (tests/far.py)."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    from nnmnkwii_amd import _hip
    L = _lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    ld = (1 << 29) + 40                                                     # elements: row 2 starts 2^32 + 320 bytes in
    P, d, _ = make_case(4000, 1, 2, 5, 3, [3], np.int64)
    want, want_len, _ = FM.frame_features_batch(P.astype(np.float32), d, None, "full", 0, dtype=np.float32)
    assert want.shape == (1, 3, 12)
    nbytes = 3 * ld * 4
    parent = far.FarParent((1, 3, ld), np.float32, low_guard_bytes=far.low_guard_for(nbytes))
    try:
        for col in (0, 23):
            parent.expect_written(0, 3, col, 12)
            assert {"2^31 bytes", "2^32 bytes"} <= parent.crossed(col)
            Pd, dd = torch.from_numpy(P.astype(np.float32)).cuda(), torch.from_numpy(d).cuda()
            lengths = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            c0 = L.nnmk_frontend_launch_count()
            rc = L.nnmk_frontend_expand(dev.index, _hip._stream(dev), 0, Pd.data_ptr(), 3, 3, dd.data_ptr(), None, 1, 2, 5, 3, 0, FM.FULL, None, None,
                                        None, 0, parent.ptr(col), ld, 3, lengths.data_ptr())
            torch.cuda.synchronize()
            assert rc == 0, L.mlpg_hip_last_error()
            assert L.nnmk_frontend_launch_count() - c0 == 1 and lengths.tolist() == [3]
            assert np.array_equal(parent.read(0, 3, col, 12), want[0])
            fails = parent.untouched()
            assert fails == [], fails
            parent.forget()
        peak = torch.cuda.max_memory_allocated()
    finally:
        parent.free()
        gc.collect()
        torch.cuda.empty_cache()
    assert peak <= far.MEM_CAP, "peak device memory %.2f GiB" % (peak / 2.0 ** 30)
