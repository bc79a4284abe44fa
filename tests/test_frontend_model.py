"""tools/frontend_model.py, the executable specification of frame expansion, against what the reference gave
(tests/golden/frontend_ref.npz, written by tests/golden/make_golden_frontend.py): bit for bit, for every sub-phone kind and both
alignments, on the reference's example labels and on the same labels with redrawn durations (states and phones of 0 frames);
the numpy coarse-coding table against the reference's scipy one; the rounding of durations; the affine map."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frontend_model as FM  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "frontend_ref.npz"))
STATE_KINDS = ("full", "minimal_frame", "state_only", "frame_only", "uniform_state", "coarse_coding")
PHONE_KINDS = ("minimal_phoneme", "coarse_coding")
CASES = [(g, k) for g in ("state", "state2") for k in STATE_KINDS] + [(g, k) for g in ("phone", "phone2") for k in PHONE_KINDS]


def test_the_golden_file_holds_what_the_generator_says():
    assert G["P"].shape == (40, 416) and G["P"].dtype == np.float64 and G["cc"].shape == (3, 600)
    assert G["state/dur"].shape == (40, 5) and G["phone/dur"].shape == (40, 1) and G["state/dur"].sum() == 615 == G["phone/dur"].sum()
    assert np.array_equal(G["state/dur"].sum(1, keepdims=True), G["phone/dur"])
    for g, S in (("state2", 5), ("phone2", 1)):
        d = G[g + "/dur"]
        assert d.shape == (40, S) and (d.sum(1) == 0).any() and (d == 0).any() and d.sum() == len(G[g + "/phone"])
    d = G["state2/dur"]
    assert (d[:, 0] == 0).any() and (d[:, -1] == 0).any() and (d[:, 1:-1] == 0).any() and (d.sum(1) == 1).any()
    for g, k in CASES:
        assert G["%s/%s" % (g, k)].shape == (len(G[g + "/phone"]), FM.get_frame_feature_size(k))


@pytest.mark.parametrize("group,kind", CASES)
def test_model_equals_the_reference_bit_for_bit(group, kind):
    P = G["P"]
    out, phone = FM.frame_features(P, G[group + "/dur"], kind, with_phone=True)
    assert out.dtype == np.float64 and np.array_equal(phone, G[group + "/phone"])
    assert np.array_equal(out[:, :416], P[phone]) and np.array_equal(out[:, 416:], G["%s/%s" % (group, kind)])
    assert len(out) == FM.frame_count(G[group + "/dur"])
    # float durations that round to the same frames (min_frames 0: the zeros stay) give the same rows
    again = FM.frame_features(P, G[group + "/dur"] + 0.25, kind, min_frames=0)
    assert np.array_equal(again, out)


def test_no_subphone_columns_is_the_row_gather():
    out, phone = FM.frame_features(G["P"], G["state2/dur"], None, with_phone=True)
    assert out.shape == (len(phone), 416) and np.array_equal(out, G["P"][phone])


def test_coarse_coding_table_equals_the_reference_s():
    cc = FM.coarse_coding_table()
    assert cc.dtype == np.float64 and np.array_equal(cc, G["cc"])


def test_feature_sizes_and_names():
    assert [FM.get_frame_feature_size(k) for k in FM.KINDS] == [0, 9, 2, 1, 1, 2, 4, 3]
    assert FM.get_frame_feature_size(" Full ") == 9
    with pytest.raises(ValueError, match="deprecated"):
        FM.get_frame_feature_size("none")
    with pytest.raises(ValueError, match="Unknown"):
        FM.get_frame_feature_size("phoneme")


def test_rounding_of_durations():
    d = np.array([0.5, 1.5, 2.5, -3.0, np.nan, 3.49, 1e12, np.inf, -np.inf])
    assert FM.frames(d, 0).tolist() == [0, 2, 2, 0, 0, 3, FM.MAX_FRAMES, FM.MAX_FRAMES, 0]
    assert FM.frames(d, 1).tolist() == [1, 2, 2, 1, 1, 3, FM.MAX_FRAMES, FM.MAX_FRAMES, 1]
    assert FM.frames(d).tolist() == FM.frames(d, 1).tolist()                      # floating point: the Merlin recipe
    assert FM.frames(d.astype(np.float32), 0).tolist() == FM.frames(d, 0).tolist()
    i = np.array([0, 1, -3, 7, 2 ** 40])
    assert FM.frames(i).tolist() == [0, 1, 0, 7, FM.MAX_FRAMES] and FM.frames(i, 2).tolist() == [2, 2, 2, 7, FM.MAX_FRAMES]
    assert FM.frames(i.astype(np.int32)[:4]).tolist() == [0, 1, 0, 7]
    with pytest.raises(ValueError):
        FM.frames(i, -1)


@pytest.mark.parametrize("kind", ["full", "coarse_coding", None])
def test_affine_map_and_output_dtype(kind):
    rng = np.random.RandomState(5)
    P, d = G["P"][:7], G["state2/dur"][:7]
    F = FM.frame_features(P, d, kind)
    W = F.shape[1]
    scale_, min_ = rng.rand(W) + 0.01, rng.randn(W)
    got = FM.frame_features(P, d, kind, scale_=scale_, min_=min_)
    assert np.array_equal(got, F * scale_ + min_)
    got32 = FM.frame_features(P, d, kind, scale_=scale_, min_=min_, dtype=np.float32)
    assert got32.dtype == np.float32 and np.array_equal(got32, (F * scale_ + min_).astype(np.float32))
    with pytest.raises(ValueError):
        FM.frame_features(P, d, kind, scale_=scale_)


def test_batch_pads_with_zeros_and_truncates():
    P = np.stack([G["P"][:6], G["P"][6:12], G["P"][12:18]])
    d = np.stack([G["state2/dur"][:6], G["state2/dur"][6:12], G["state2/dur"][12:18]])
    n = np.array([6, 0, 9])
    out, lengths, counts = FM.frame_features_batch(P, d, n, "full")
    each = [FM.frame_features(P[b, :m], d[b, :m], "full") for b, m in enumerate((6, 0, 6))]
    assert counts.tolist() == [len(e) for e in each] and lengths.tolist() == counts.tolist() and out.shape == (3, counts.max(), 425)
    for b, e in enumerate(each):
        assert np.array_equal(out[b, :len(e)], e) and not out[b, len(e):].any()
    cut, lengths, counts2 = FM.frame_features_batch(P, d, n, "full", Tmax=int(counts.max()) - 1)
    assert np.array_equal(cut, out[:, :-1]) and lengths.tolist() == np.minimum(counts, counts.max() - 1).tolist() and counts2.tolist() == counts.tolist()
