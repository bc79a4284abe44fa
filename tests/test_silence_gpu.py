"""Silence removal on the device (-m gpu): nnmk_sil_frame_counts, nnmk_sil_expand and nnmk_sil_gather (csrc/frame_keep.hip)
against the specification tools/silence_model.py through the C entries on guarded, poisoned buffers (tests/silence_cases.py:
run_entries), then ``frontend.merlin.kept_frame_features*`` and ``preprocessing.remove_silence_frames*`` on CUDA tensors and
numpy arrays against what the reference gave (tests/golden/silence_ref.npz).

No tolerance anywhere: every comparison is ``np.array_equal`` or bytes."""
import ctypes

import numpy as np
import pytest
import torch

import silence_cases as SC
from silence_cases import FM, SM

pytestmark = pytest.mark.gpu

G = np.load(SC.GOLDEN)
BLOCK = SC.BLOCK
F32, F64 = np.float32, np.float64


def exact32(P):
    """The same values in both phone dtypes."""
    return P.astype(F32).astype(F64)


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("kind", range(8))
def test_every_kind_dtype_and_flag_case(kind, S):
    """Both batches of plans (K_b = 0, 1, 63, 64, 65, 131; flagged phones across blocks of the output and of the source; first,
    last, all and no phones flagged; a flagged phone of 0 frames; states of 0 frames beside a flagged phone; num_phones 0 and
    below Nmax with flags behind it) at every kind, over the four duration dtypes and both output dtypes; the gather beside it
    with len_src 0, T_b - 1, T_b and T_b + 70 and D 1 and 65."""
    i = kind * 2 + (S == 5)
    for j, plans in enumerate((SC.PLANS_A, SC.PLANS_B)):
        T = SC.all_counts(plans)
        Tmax = int(T.max()) + 70
        lens = np.array([[0, T[1] - 1, T[2], T[3] + 70, T[4] - 1, T[5] + 70], [5, T[1], T[2] - 1, T[3] - 100, T[4] + 70, 0]][j])
        want = None
        for k, dur in enumerate(SC.DUR_DTYPES):
            P, d, sil, n, _ = SC.make_batch(i + 40 * j, plans, S, 3, dur)
            P = exact32(P)
            with_affine = bool((i + j) % 2)
            if want is None:
                sc, mn = SC.affine(i, 3 + FM.SIZES[kind]) if with_affine else (None, None)
                want = SM.kept_frame_features_batch(P, d, sil, n, FM.KINDS[kind], 0, sc, mn, None, F64,
                                                    FM.coarse_coding_table() if kind == FM.COARSE_CODING else None)
                assert list(want[2]) == list(SC.kept_counts(plans))
            for out_dtype in (F32, F64):
                g = dict(Y=SC.source(i, len(plans), Tmax, (1, 65)[(k + j) % 2], np.clip(lens, 0, Tmax), (F32, F64)[k % 2]), len=lens) \
                    if out_dtype == (F32, F64)[k % 2] or k == 0 else None
                SC.run_entries(P, d, sil, n, kind, 0, with_affine, (F32, F64)[(k + (out_dtype == F64)) % 2], out_dtype, gather=g, seed=i, want=want)


@pytest.mark.parametrize("Dl,kind", [(0, FM.STATE_ONLY), (55, FM.FULL), (56, FM.FULL), (121, FM.FULL), (64, FM.NONE)])
def test_widths(Dl, kind):
    """Dl + F = 1, 64, 65 (a second pass over the columns) and 130 (a third)."""
    P, d, sil, n, _ = SC.make_batch(Dl, SC.PLANS_A, 5, Dl, np.int32)
    assert Dl + FM.SIZES[kind] in (1, 64, 65, 130)
    SC.run_entries(P, d, sil, n, kind, 0, Dl % 2 == 0, F64, F32, seed=Dl)
    SC.run_entries(P, d, sil, n, kind, 0, Dl % 2 == 1, F32, F64, seed=Dl)


@pytest.mark.parametrize("Tcap", [0, 1, BLOCK, 2 * BLOCK + 3, 200])
def test_capacity_below_and_above_the_kept_frames(Tcap):
    """Tcap below K_b: the rows are cut and the lengths capped; above: zero rows behind them.  The gather's capacity likewise."""
    P, d, sil, n, _ = SC.make_batch(Tcap, SC.PLANS_A, 5, 2, SC.DUR_DTYPES[Tcap % 4])
    lens = np.array([150, 3, 73, 76, 150, 131])
    g = dict(Y=SC.source(Tcap, 6, 150, 2, lens), len=lens, Tcap=Tcap)
    out, lengths, gout, glen = SC.run_entries(P, d, sil, n, FM.FULL, 0, False, F64, F64, Tcap=Tcap, gather=g)
    assert list(lengths) == [min(k, Tcap) for k in SC.K_A]
    assert list(glen) == [min(k, Tcap) for k in (138, 0, 63, 64, 65 + 77, 131)]
    for b in range(6):
        assert not out[b, lengths[b]:].any() and not gout[b, glen[b]:].any()


def test_no_num_phones_no_lengths_min_frames_and_the_state_cap():
    """NULL num_phones and len_src; min_frames 1; and Nmax * S = 8192 states, whose running counts take more LDS than a kernel gets
    unasked."""
    plans = [[(3, 0), (4, 1), (2, 0)], [(1, 1), (1, 0), (6, 1)]]
    for S in (1, 5):
        P, d, sil, n, _ = SC.make_batch(S, plans, S, 4, F64, spare=0)
        SC.run_entries(P, d, sil, None, FM.FULL, 1, True, F64, F32, Tcap=40, gather=dict(Y=SC.source(S, 2, 40, 3, [40, 40]), len=None, Tcap=40))
    rng = np.random.RandomState(8)
    Nmax, S = 1024, 8
    r = (rng.rand(1, Nmax, S) < 0.02).astype(np.int64)
    sil = (rng.rand(1, Nmax) < 0.3).astype(np.uint8)
    r[0, -1, -1] = 2                                                        # the last state of all is found
    sil[0, -1] = 0
    P = exact32(rng.randn(1, Nmax, 1))
    T = int(r.sum())
    SC.run_entries(P, r.astype(np.int32), sil, None, FM.MINIMAL_FRAME, 0, False, F32, F32,
                   gather=dict(Y=SC.source(9, 1, T + 3, 2, [T + 3]), len=None))


def test_refusals_on_the_device():
    """out == src, and a batch of more output blocks than one grid takes (refused with its text, as the header says): nothing is
    launched."""
    from nnmnkwii_amd import _silence_hip as SH
    L = SH.lib()
    x = torch.zeros((2, 70, 3), dtype=torch.float64, device="cuda")
    d = torch.ones((2, 4, 5), dtype=torch.int32, device="cuda")
    s = torch.zeros((2, 4), dtype=torch.bool, device="cuda")
    n0 = SC.launches()
    with pytest.raises(ValueError, match="must not be the source"):
        SH.gather(x, None, d, None, s, 0, x)
    lengths = torch.zeros(2, dtype=torch.int32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.nnmk_sil_gather(0, None, 2, vp(d), None, vp(s), 2, 4, 5, 0, 1, vp(x), 3, None, 70, 3, 1, vp(x), 3, 70, vp(lengths))
    assert rc == -1 and b"out == src" in L.mlpg_hip_last_error()
    rc = L.nnmk_sil_gather(0, None, 2, vp(d), None, vp(s), 2, 4, 5, 0, 1, vp(x), 3, None, 70, 3, 1, vp(x), 3, 1 << 30, vp(lengths))
    assert rc == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    rc = L.nnmk_sil_expand(0, None, 1, vp(x), 3, 2, vp(d), None, vp(s), 2, 4, 5, 3, 0, 0, None, None, None, 1, vp(x), 3, 1 << 30, vp(lengths))
    assert rc == -1 and b"too large for one grid" in L.mlpg_hip_last_error()
    torch.cuda.synchronize()
    assert SC.launches() == n0 and not x.any()


# ---- the public functions against the reference ------------------------------------------------------------------------------------

GROUPS = (("state", "P9"), ("state2", "P9"), ("phone2", "P9"), ("a0001", "P1"), ("a00012", "P1"))


def kinds_of(group):
    return sorted(k.split("/")[2] for k in G.files if k.startswith(group + "/default/") and not k.endswith("/phone"))


def golden(group, pname, rx, kind):
    phone = G["%s/%s/phone" % (group, rx)]
    return np.concatenate([G[pname][phone], G["%s/%s/%s" % (group, rx, kind)]], axis=1)


@pytest.mark.parametrize("rx", ["default", "wide"])
def test_kept_frame_features_give_the_reference_s_matrices(rx):
    """One utterance at a time from numpy, every group and kind; then all state-aligned groups as one padded batch of CUDA
    tensors, float durations, with out= a column slice of a wider tensor."""
    from nnmnkwii_amd.frontend import merlin as fe
    for group, pname in GROUPS:
        d, sil = G[group + "/dur"], G["%s/sil_%s" % (group, rx)]
        for kind in kinds_of(group):
            got = fe.kept_frame_features(G[pname], d, sil, kind)
            assert got.dtype == F64 and np.array_equal(got, golden(group, pname, rx, kind)), (group, kind)
    groups = [g for g in GROUPS if g[0] != "phone2"]
    Nmax = max(len(G[g + "/dur"]) for g, _ in groups)
    B = len(groups)
    P, d, sil = np.full((B, Nmax, 416), np.nan), np.full((B, Nmax, 5), np.nan), np.ones((B, Nmax), dtype=bool)
    n = np.zeros(B, dtype=np.int32)
    for b, (g, pname) in enumerate(groups):
        n[b] = len(G[g + "/dur"])
        P[b, :n[b]], d[b, :n[b]], sil[b, :n[b]] = G[pname], G[g + "/dur"], G["%s/sil_%s" % (g, rx)]
    want = [golden(g, pname, rx, "full") for g, pname in groups]
    K = max(len(w) for w in want)
    wide = torch.full((B, K + 5, 430), -7.0, dtype=torch.float64, device="cuda")
    n0 = SC.launches()
    out, lengths = fe.kept_frame_features_batch(torch.from_numpy(P).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(sil).cuda(),
                                                torch.from_numpy(n).cuda(), "full", min_frames=0, out=wide[:, :, 2:427], strict=False)
    assert SC.launches() == n0 + 1 and out.data_ptr() == wide[:, :, 2:427].data_ptr()
    got, host = wide.cpu().numpy(), lengths.cpu().numpy()
    assert list(host) == [len(w) for w in want] and (got[:, :, :2] == -7.0).all() and (got[:, :, 427:] == -7.0).all()
    for b, w in enumerate(want):
        assert np.array_equal(got[b, :len(w), 2:427], w) and not got[b, len(w):, 2:427].any()
    # strict: the first utterance whose kept frames do not fit is named; strict=False caps the lengths
    with pytest.raises(ValueError, match="utterance 0 has %d kept frames, Tmax is 100" % len(want[0])):
        fe.kept_frame_features_batch(P, d, sil, n, "full", min_frames=0, Tmax=100)
    out, lengths = fe.kept_frame_features_batch(P, d, sil, n, "full", min_frames=0, Tmax=100, strict=False, dtype=F32)
    assert out.dtype == F32 and list(lengths) == [100] * B and np.array_equal(out[0], want[0][:100].astype(F32))
    out, lengths = fe.kept_frame_features_batch(P, d, sil, n, "full", min_frames=0)
    assert out.shape == (B, K, 425) and list(lengths) == [len(w) for w in want]


def test_rounded_once_it_is_merlin_s_own_file():
    from nnmnkwii_amd.frontend import merlin as fe
    got = fe.kept_frame_features(torch.from_numpy(G["P1"]).cuda(), torch.from_numpy(G["a0001/dur"]).cuda(),
                                 torch.from_numpy(G["a0001/sil_default"]).cuda(), "full", dtype=torch.float32)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (578, 425)
    got = got.cpu().numpy()
    assert np.array_equal(got[:, 416:], G["merlin/sub"]) and np.array_equal(got[:, :416], G["P1"][G["merlin/phone"]].astype(F32))
    # with no flags the existing function's rows
    same = fe.kept_frame_features(G["P1"], G["a0001/dur"], np.zeros(len(G["P1"]), dtype=np.int64), "full")
    assert np.array_equal(same, fe.frame_features(G["P1"], G["a0001/dur"], "full"))


@pytest.mark.parametrize("rx", ["default", "wide"])
def test_remove_silence_frames_is_np_delete(rx):
    from nnmnkwii_amd import preprocessing as PP
    d, sil = G["a0001/dur"], G["a0001/sil_" + rx]
    ys = [G["gather/y_%d" % k] for k in range(3)]
    want = [G["gather/%s/out_%d" % (rx, k)] for k in range(3)]
    for y, w in zip(ys, want):
        got = PP.remove_silence_frames(y, d, sil)
        assert got.dtype == F64 and np.array_equal(got, w)
        got = PP.remove_silence_frames(torch.from_numpy(y).cuda().float(), torch.from_numpy(d).cuda(), torch.from_numpy(sil).cuda())
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), w.astype(F32))
    # the three as one padded batch: a column slice in, a column slice out
    lens = np.array([len(y) for y in ys], dtype=np.int32)
    Tmax = int(lens.max())
    src = torch.full((3, Tmax, 9), float("nan"), dtype=torch.float64, device="cuda")
    for b, y in enumerate(ys):
        src[b, :len(y), 3:8] = torch.from_numpy(y).cuda()
    D3, S3 = np.repeat(d[None], 3, 0), np.repeat(sil[None], 3, 0)
    wide = torch.full((3, Tmax, 8), -7.0, dtype=torch.float32, device="cuda")
    n0 = SC.launches()
    out, lengths = PP.remove_silence_frames_batch(src[:, :, 3:8], torch.from_numpy(D3).cuda(), torch.from_numpy(S3).cuda(), torch.from_numpy(lens).cuda(),
                                                  out=wide[:, :, 1:6], strict=False)
    assert SC.launches() == n0 + 1
    got = wide.cpu().numpy()
    assert list(lengths.cpu().numpy()) == [len(w) for w in want] and (got[:, :, 0] == -7.0).all() and (got[:, :, 6:] == -7.0).all()
    for b, w in enumerate(want):
        assert np.array_equal(got[b, :len(w), 1:6], w.astype(F32)) and not got[b, len(w):, 1:6].any()
    # numpy in, numpy out, cut to the longest; strict names the utterance that does not fit
    Y = np.zeros((3, Tmax, 5))
    for b, y in enumerate(ys):
        Y[b, :len(y)] = y
    out, lengths = PP.remove_silence_frames_batch(Y, D3, S3, lens)
    assert out.shape == (3, max(len(w) for w in want), 5) and list(lengths) == [len(w) for w in want]
    assert all(np.array_equal(out[b, :len(w)], w) and not out[b, len(w):].any() for b, w in enumerate(want))
    cap = min(len(w) for w in want)
    first = next(b for b, w in enumerate(want) if len(w) > cap)
    with pytest.raises(ValueError, match="utterance %d keeps %d frames, Tmax is %d" % (first, len(want[first]), cap)):
        PP.remove_silence_frames_batch(Y, D3, S3, lens, Tmax=cap)
    out, lengths = PP.remove_silence_frames_batch(Y, D3, S3, lens, Tmax=cap, strict=False)
    assert list(lengths) == [cap] * 3 and np.array_equal(out[2], want[2][:cap])
    x = torch.from_numpy(Y).cuda()
    with pytest.raises(ValueError, match="must not be the matrix itself"):
        PP.remove_silence_frames_batch(x, D3, S3, lens, out=x)
