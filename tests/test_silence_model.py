"""tools/silence_model.py against what the reference gives (-m "not gpu"): tests/golden/silence_ref.npz holds
``np.delete(linguistic_features(...), labels.silence_frame_indices(regex), axis=0)`` for the reference's labels under two
expressions, Merlin's own no-silence file, and ``np.delete`` of random matrices (tests/golden/make_golden_silence.py).  Every
comparison is ``np.array_equal``."""
import numpy as np
import pytest

import silence_cases as SC
from silence_cases import FM, SM

G = np.load(SC.GOLDEN)
GROUPS = (("state", "P9"), ("state2", "P9"), ("phone", "P9"), ("phone2", "P9"), ("a0001", "P1"), ("a00012", "P1"))
RX = ("default", "wide")


def kinds_of(group):
    return sorted(k.split("/")[2] for k in G.files if k.startswith(group + "/default/") and not k.endswith("/phone"))


@pytest.mark.parametrize("group,pname", GROUPS)
@pytest.mark.parametrize("rx", RX)
def test_model_gives_the_reference_s_matrices(group, pname, rx):
    P, d, sil = G[pname], G[group + "/dur"], G["%s/sil_%s" % (group, rx)]
    phone = G["%s/%s/phone" % (group, rx)]
    assert len(kinds_of(group)) in (2, 6)
    for kind in kinds_of(group):
        got = SM.kept_frame_features(P, d, sil, kind)
        assert got.dtype == np.float64 and np.array_equal(got[:, :416], P[phone]) and np.array_equal(got[:, 416:], G["%s/%s/%s" % (group, rx, kind)])
    assert np.array_equal(SM.frame_counts(d[None], sil[None])[0], [len(phone), d.sum()])
    assert np.array_equal(np.repeat(np.arange(len(d)), d.sum(1))[SM.keep_mask(d, sil)], phone)


def test_the_flags_are_where_the_issue_says():
    assert [int(G["%s/sil_%s" % (g, rx)].sum()) for g in ("state", "a0001") for rx in RX] == [2, 9, 2, 11]
    assert G["state2/sil_default"][-1] and G["state2/dur"][-1].sum() == 0           # a flagged phone of 0 frames
    assert (G["state2/dur"] == 0).any(axis=1).sum() > 5                             # states of 0 frames


def test_model_rounded_once_is_merlin_s_own_file():
    got = SM.kept_frame_features(G["P1"], G["a0001/dur"], G["a0001/sil_default"], "full", dtype=np.float32)
    assert got.shape == (578, 425) and np.array_equal(got[:, 416:], G["merlin/sub"])
    assert np.array_equal(got[:, :416], G["P1"][G["merlin/phone"]].astype(np.float32))


@pytest.mark.parametrize("rx", RX)
def test_gather_is_np_delete(rx):
    d, sil = G["a0001/dur"], G["a0001/sil_" + rx]
    T = int(d.sum())
    assert list(G["gather/len"]) == [T - 37, T, T + 70]
    for k in range(3):
        y = G["gather/y_%d" % k]
        got = SM.remove_silence_frames(y, d, sil)
        assert np.array_equal(got, G["gather/%s/out_%d" % (rx, k)])
        out, lengths, counts = SM.remove_silence_frames_batch(y[None], d[None], sil[None])
        assert np.array_equal(out[0], got) and lengths[0] == len(got) == counts[0]


def test_tiled_forms_walk_to_the_same_result():
    for j, plans in enumerate((SC.PLANS_A, SC.PLANS_B)):
        for S in (1, 5):
            P, d, sil, n, _ = SC.make_batch(j + S, plans, S, 2, SC.DUR_DTYPES[(j + S) % 4])
            sc, mn = SC.affine(j, 2 + 9)
            for Tcap in (None, 0, 64, 70):
                a = SM.kept_frame_features_batch(P, d, sil, n, "full", 0, sc, mn, Tcap=Tcap)
                b = SM.tiled_kept_frame_features_batch(P, d, sil, n, "full", 0, sc, mn, Tcap=Tcap)
                assert all(SC.same_bits(x, y) for x, y in zip(a, b)), (j, S, Tcap)
            T = SC.all_counts(plans)
            Tmax = int(T.max()) + 70
            for lens in (None, np.maximum(T - 1, 0), T, T + 70, np.zeros_like(T), T // 2):
                Y = SC.source(j, len(plans), Tmax, 3, np.full(len(plans), Tmax) if lens is None else lens)
                for Tcap in (None, 64, Tmax):
                    a = SM.remove_silence_frames_batch(Y, d, sil, lens, n, 0, Tcap)
                    b = SM.tiled_remove_silence_frames_batch(Y, d, sil, lens, n, 0, Tcap)
                    assert all(SC.same_bits(x, y) for x, y in zip(a, b)), (j, S, lens, Tcap)
    # the golden labels, flagged phones in the middle of the utterance
    P, d, sil = G["P9"][None, :, :4], G["state/dur"][None], G["state/sil_wide"][None]
    a = SM.kept_frame_features_batch(P, d, sil, None, "full")
    b = SM.tiled_kept_frame_features_batch(P, d, sil, None, "full")
    assert all(SC.same_bits(x, y) for x, y in zip(a, b)) and a[1][0] == 477


def test_duration_rule_and_subphone_rows_are_the_frontend_model_s_own():
    assert SM.frames is FM.frames and SM.subphone_row is FM.subphone_row and SM.BLOCK_ROWS == FM.BLOCK_ROWS == 64


def test_no_phone_flagged_is_the_frontend_model():
    for kind in FM.KINDS:
        for S in (1, 5):
            P, d, sil, n, _ = SC.make_batch(S, SC.PLANS_A, S, 2, np.float64)
            sil[:] = 0
            want = FM.frame_features_batch(P, d, n, kind, 1, Tmax=150, dtype=np.float32)
            got = SM.kept_frame_features_batch(P, d, sil, n, kind, 1, Tcap=150, dtype=np.float32)
            assert all(SC.same_bits(x, y) for x, y in zip(got, want))
            Y = SC.source(S, 6, 150, 2, np.full(6, 150))
            assert SC.same_bits(SM.remove_silence_frames_batch(Y, d, sil, None, n, 1)[0], Y)
