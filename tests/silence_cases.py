"""Inputs shared by the silence-removal tests (tests/test_silence_host_cpu.py, tests/test_silence_gpu.py,
tests/test_embed_silence_gpu.py, tests/test_far_silence_gpu.py): utterances given as plans -- one (frames, flagged) pair per
phone -- whose frames are dealt to the phone's states with zeros among them, encoded in each duration dtype so that every dtype
gives the same frames, with everything at or past num_phones poisoned."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frontend_model as FM  # noqa: E402
import silence_model as SM  # noqa: E402

from test_frontend_host_cpu import encode  # noqa: E402  (durations of a dtype that give chosen frames)

DUR_DTYPES = (np.int32, np.int64, np.float32, np.float64)
BLOCK = SM.BLOCK_ROWS
GOLDEN = os.path.join(ROOT, "tests", "golden", "silence_ref.npz")

# K_b = 0 (all flagged, a flagged phone of 0 frames), 1 (first and last flagged), 63 (the flagged phone covers source frames
# 60 .. 69: it straddles a block of the source), 64 (flagged phones of 0 frames beside it), 65 (the flagged phone lies between
# output rows 63 and 64: it straddles a block of the output), 131 (no phone flagged; a phone of 0 frames)
PLANS_A = ([(5, 1), (0, 1), (7, 1)],
           [(4, 1), (1, 0), (3, 1)],
           [(60, 0), (10, 1), (3, 0)],
           [(3, 1), (64, 0), (0, 1), (9, 1)],
           [(64, 0), (8, 1), (1, 0)],
           [(40, 0), (0, 0), (50, 0), (41, 0)])
K_A = (0, 1, 63, 64, 65, 131)
# no phones at all, the last phone flagged, phones of 0 frames on both sides of flagged ones, a flagged phone between two blocks of
# both, many short phones with every third flagged
PLANS_B = ([],
           [(20, 0), (6, 0), (11, 1)],
           [(2, 0), (0, 0), (5, 1), (0, 0), (0, 1), (3, 0), (0, 1)],
           [(70, 0), (130, 1), (70, 0)],
           [(1 + k % 4, k % 3 == 1) for k in range(12)],
           [(9, 1)])


def deal(rng, total, S, zero_first=False, zero_last=False):
    """`total` frames over S states, some of them 0."""
    w = rng.rand(S) * (rng.rand(S) > 0.35)
    if zero_first:
        w[0] = 0.0
    if zero_last:
        w[-1] = 0.0
    if not w.any() or S == 1:
        w = np.zeros(S)
        w[S // 2] = 1.0
    r = np.floor(w / w.sum() * total).astype(np.int64)
    r[int(np.argmax(w))] += total - r.sum()
    assert r.sum() == total and (r >= 0).all()
    return r


def make_batch(seed, plans, S, Dl, dur_dtype, Nmax=None, spare=1):
    """(P (B, Nmax, Dl) float64, durations (B, Nmax, S) of dur_dtype, silence (B, Nmax) uint8, num_phones (B) int32, frames
    (B, Nmax, S) int64).  Nmax: the longest plan + spare; what lies at or past num_phones is poisoned: phone rows NaN, durations
    NaN or the type's largest integer, flags 1.  A state beside a flagged phone is a state of 0 frames where S > 1."""
    rng = np.random.RandomState(seed)
    B = len(plans)
    Nmax = max(len(p) for p in plans) + spare if Nmax is None else Nmax
    r = np.zeros((B, Nmax, S), dtype=np.int64)
    sil = np.zeros((B, Nmax), dtype=np.uint8)
    n = np.array([len(p) for p in plans], dtype=np.int32)
    for b, plan in enumerate(plans):
        for k, (total, flagged) in enumerate(plan):
            after = k > 0 and plan[k - 1][1] and not flagged
            before = k + 1 < len(plan) and plan[k + 1][1] and not flagged
            r[b, k] = deal(rng, total, S, zero_first=after, zero_last=before)
            sil[b, k] = 3 if flagged and k % 2 else bool(flagged)       # (any non-zero byte is a flag)
    P = np.round(rng.randn(B, Nmax, Dl) * 4) / 4 + (rng.rand(B, Nmax, Dl) < 0.3) * rng.rand(B, Nmax, Dl)
    d = encode(rng, r, dur_dtype)
    for b in range(B):
        P[b, n[b]:] = np.nan
        d[b, n[b]:] = np.iinfo(d.dtype).max if d.dtype.kind == "i" else np.nan
        sil[b, n[b]:] = 1
    return P, d, sil, n, r


def kept_counts(plans):
    return np.array([sum(t for t, f in p if not f) for p in plans], dtype=np.int64)


def all_counts(plans):
    return np.array([sum(t for t, f in p) for p in plans], dtype=np.int64)


def affine(seed, W):
    rng = np.random.RandomState(seed + 77)
    return rng.rand(W) + 0.5, np.round(rng.randn(W) * 8) / 8


def source(seed, B, Tmax, D, lengths, dtype=np.float64):
    """A (B, Tmax, D) matrix whose rows at or past each length hold NaN (they are never read)."""
    rng = np.random.RandomState(seed + 5)
    Y = rng.randn(B, Tmax, D).astype(dtype)
    Y[rng.rand(B, Tmax, D) < 0.05] = -0.0
    for b in range(B):
        Y[b, max(int(lengths[b]), 0):] = np.nan
    return Y


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the C entries on guarded buffers (GPU tests) ---------------------------------------------------------------------------------

DT_CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}
POISON = 0xA5


def launches():
    from nnmnkwii_amd import _silence_hip
    return _silence_hip.lib().nnmk_sil_launch_count()


def run_entries(P, d, sil, n, kind, min_frames, with_affine, p_dtype, out_dtype, Tcap=None, gather=None, pad_p=2, pad_out=3, offs=(1, 3, 1, 1, 1, 3),
                seed=0, want=None):
    """nnmk_sil_frame_counts, nnmk_sil_expand and (gather: dict(Y, len or None, Tcap or None)) nnmk_sil_gather on tests/embed.py
    buffers -- payloads `offs` elements into byte buffers of one value, inputs snapshotted, the phone matrix and the source as
    column slices of wider rows whose other columns hold NaN, the outputs filled with a poison byte -- compared with
    tools/silence_model.py bit for bit.  offs: the element offsets of (phone, durations, flags, num_phones / len_src, scale_ /
    min_ / cc, outputs).  want: the model's (out, lengths, counts) in float64 if the caller has it.  Returns the kept rows and
    their lengths (and the gather's)."""
    import ctypes
    import torch
    from embed import Embedded, embedded, failed
    from nnmnkwii_amd import _hip, _silence_hip
    L = _silence_hip.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    ptr = lambda b: None if b is None else ctypes.c_void_p(b.ptr())  # noqa: E731
    B, Nmax, Dl = P.shape
    S = d.shape[2]
    W = Dl + FM.SIZES[kind]
    P = P.astype(p_dtype)
    scale_, min_ = affine(seed, W) if with_affine else (None, None)
    cc = FM.coarse_coding_table() if kind == FM.COARSE_CODING else None
    if want is None:
        want = SM.kept_frame_features_batch(P, d, sil, n, FM.KINDS[kind], min_frames, scale_, min_, Tcap, np.float64, cc)
    want_out, want_len, want_counts = want[0].astype(out_dtype), want[1], want[2]
    Tcap = want_out.shape[1]
    o_p, o_d, o_s, o_n, o_c, o_o = offs
    Pw = np.concatenate([P, np.full((B, Nmax, pad_p), np.nan, dtype=p_dtype)], axis=2)
    ins = dict(phone=embedded(Pw, o_p), durations=embedded(d, o_d), silence=embedded(sil.astype(np.uint8), o_s), num_phones=embedded(n, o_n),
               cc=embedded(cc, o_c), scale_=embedded(scale_, o_c), min_=embedded(min_, o_c + 2))
    out = Embedded((B, Tcap, W + pad_out), out_dtype, o_o, fill_byte=POISON)
    lengths, counts = Embedded((B,), np.int32, o_o, fill_byte=POISON), Embedded((B, 2), np.int64, o_o, fill_byte=POISON)
    outs = dict(out=out, lengths=lengths, counts=counts)
    st = _hip._stream(dev)
    n0 = L.nnmk_sil_launch_count()
    rc = L.nnmk_sil_frame_counts(dev.index, st, DT_CODE[d.dtype], ptr(ins["durations"]), ptr(ins["num_phones"]), ptr(ins["silence"]), B, Nmax, S,
                                 min_frames, ptr(counts))
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    rc = L.nnmk_sil_expand(dev.index, st, DT_CODE[np.dtype(p_dtype)], ptr(ins["phone"]), Dl + pad_p, DT_CODE[d.dtype], ptr(ins["durations"]),
                           ptr(ins["num_phones"]), ptr(ins["silence"]), B, Nmax, S, Dl, min_frames, kind, ptr(ins["cc"]), ptr(ins["scale_"]),
                           ptr(ins["min_"]), DT_CODE[np.dtype(out_dtype)], ptr(out), W + pad_out, Tcap, ptr(lengths))
    assert rc == 0, (rc, L.mlpg_hip_last_error())
    calls = 2
    if gather is not None:
        Y, ln = gather["Y"], gather["len"]
        Tmax, D = Y.shape[1:]
        gwant, gwant_len, _ = SM.remove_silence_frames_batch(Y, d, sil, ln, n, min_frames, gather.get("Tcap"), out_dtype)
        Tg = gwant.shape[1]
        Yw = np.concatenate([Y, np.full((B, Tmax, pad_p), np.nan, dtype=Y.dtype)], axis=2)
        ins.update(src=embedded(Yw, o_p), len_src=embedded(None if ln is None else np.asarray(ln, dtype=np.int32), o_n))
        gout, glen = Embedded((B, Tg, D + pad_out), out_dtype, o_o, fill_byte=POISON), Embedded((B,), np.int32, o_o, fill_byte=POISON)
        outs.update(gather_out=gout, gather_lengths=glen)
        rc = L.nnmk_sil_gather(dev.index, st, DT_CODE[d.dtype], ptr(ins["durations"]), ptr(ins["num_phones"]), ptr(ins["silence"]), B, Nmax, S,
                               min_frames, DT_CODE[Y.dtype], ptr(ins["src"]), D + pad_p, ptr(ins["len_src"]), Tmax, D, DT_CODE[np.dtype(out_dtype)],
                               ptr(gout), D + pad_out, Tg, ptr(glen))
        assert rc == 0, (rc, L.mlpg_hip_last_error())
        calls = 3
    torch.cuda.synchronize()
    assert L.nnmk_sil_launch_count() == n0 + calls                         # one per call
    assert failed(inputs=ins, outputs=outs) == []
    fill = np.frombuffer(bytes([POISON]) * 8, dtype=out_dtype)[0]
    got = out.host()
    assert np.array_equal(counts.host()[:, 0], want_counts) and np.array_equal(counts.host(), SM.frame_counts(d, sil, n, min_frames))
    assert np.array_equal(lengths.host(), want_len), (lengths.host(), want_len)
    assert same_bits(got[:, :, :W], want_out)
    assert same_bits(got[:, :, W:], np.full((B, Tcap, pad_out), fill, dtype=out_dtype))      # foreign columns: untouched
    res = [got[:, :, :W], lengths.host()]
    if gather is not None:
        gg = gout.host()
        assert np.array_equal(glen.host(), gwant_len), (glen.host(), gwant_len)
        assert same_bits(gg[:, :, :D], gwant)
        assert same_bits(gg[:, :, D:], np.full((B, Tg, pad_out), fill, dtype=out_dtype))
        res += [gg[:, :, :D], glen.host()]
    return res
