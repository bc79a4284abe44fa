"""Writes tests/golden/silence_ref.npz: what the reference gives for

    X = linguistic_features(labels, ..., add_frame_features=True, subphone_features=kind)
    X = np.delete(X, labels.silence_frame_indices(regex), axis=0)

on its example labels (arctic_a0009_state.lab, arctic_a0009_phone.lab) and its test label
(tests/data/label_state_align/arctic_a0001.lab), under the default expression ``.*-sil+.*`` ("default") and under
``.*-(sil|pau|t|ax)\\+.*`` ("wide": flagged phones in the middle of the utterances), with the reference loaded from its files as
tests/golden/make_golden_frontend.py does:

    python tests/golden/make_golden_silence.py /path/to/reference

The file holds data only:
  P9, P1                      the phone-level matrices of arctic_a0009 (40, 416) and arctic_a0001 (add_frame_features=False)
  <group>/dur                 the durations in frames, (N, 5) or (N, 1)
  <group>/sil_<rx>            the flags: zeros(N, bool) with labels.silence_phone_indices(regex) set
  <group>/<rx>/phone          each KEPT frame's phone index (K,)
  <group>/<rx>/<kind>         the sub-phone columns (K, F) of the reference's matrix after np.delete; the generator asserts that
                              the columns in front of them equal P[phone], so they are not stored
  merlin/sub, merlin/phone    the sub-phone columns (578, 9) float32 of Merlin's own no-silence file
                              tests/data/nn_no_silence_lab_425/arctic_a0001.lab and its rows' phone indices (those of
                              a0001/default); the generator asserts that the 416 columns in front equal float32(P1[phone])
  gather/y_<k>, gather/len    random (T, 5) matrices for T below (k = 0), at (1) and above (2) the frames of arctic_a0001
  gather/<rx>/out_<k>         np.delete(y_<k>, idx, axis=0), idx = silence_frame_indices(regex).  For T below the label's frames
                              the indices at or past T are dropped first, as np.delete of older numpy did silently (numpy 1.19 and
                              later raise IndexError for them): the acoustic matrix is shorter than the labels, the silent
                              frames it does not have cannot be deleted.
Groups "state", "phone" and "a0001" are the labels as they are; "state2", "phone2" and "a00012" the same label strings with
redrawn durations (make_golden_frontend.redrawn): states and phones of 0 frames, the last phone -- flagged by both expressions --
among them."""
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_frontend import PHONE_KINDS, STATE_KINDS, durations_of, load_reference, redrawn  # noqa: E402

REGEX = {"default": None, "wide": re.compile(r".*-(sil|pau|t|ax)\+.*")}


def run_group(fe, labels, binary, numeric, kinds, S, P, out, group):
    dur = durations_of(labels, S)
    phone = np.repeat(np.arange(len(dur)), dur.sum(1))
    out[group + "/dur"] = dur
    for rx, regex in REGEX.items():
        sil = np.zeros(len(dur), dtype=bool)
        sil[labels.silence_phone_indices(regex)] = True
        idx = labels.silence_frame_indices(regex).astype(np.int64)
        kept = np.delete(phone, idx)
        out["%s/sil_%s" % (group, rx)], out["%s/%s/phone" % (group, rx)] = sil, kept
        assert np.array_equal(kept, phone[~sil[phone]]), (group, rx)        # a frame is silent iff its phone is flagged
        for kind in kinds:
            M = fe.linguistic_features(labels, binary, numeric, subphone_features=kind, add_frame_features=True)
            M = np.delete(M, idx, axis=0)
            assert M.dtype == np.float64 and M.shape == (len(kept), P.shape[1] + fe.get_frame_feature_size(kind)), (group, rx, kind, M.shape)
            assert np.array_equal(M[:, :P.shape[1]], P[kept]), (group, rx, kind)
            out["%s/%s/%s" % (group, rx, kind)] = np.ascontiguousarray(M[:, P.shape[1]:])
        print(group, rx, int(sil.sum()), "phones flagged,", len(kept), "of", len(phone), "frames kept")


def main(root):
    hts, fe = load_reference(root)
    data = os.path.join(root, "nnmnkwii", "util", "_example_data")
    tests = os.path.join(root, "tests", "data")
    binary, numeric = hts.load_question_set(os.path.join(data, "questions-radio_dnn_416.hed"))
    state = hts.load(os.path.join(data, "arctic_a0009_state.lab"))
    phone = hts.load(os.path.join(data, "arctic_a0009_phone.lab"))
    a0001 = hts.load(os.path.join(tests, "label_state_align", "arctic_a0001.lab"))
    P9 = fe.linguistic_features(state, binary, numeric, subphone_features=None, add_frame_features=False)
    P1 = fe.linguistic_features(a0001, binary, numeric, subphone_features=None, add_frame_features=False)
    out = {"P9": P9, "P1": P1}
    rng = np.random.RandomState(20241)
    with tempfile.TemporaryDirectory() as tmp:
        for group, labels, kinds, S, P in (("state", state, STATE_KINDS, 5, P9), ("phone", phone, PHONE_KINDS, 1, P9),
                                           ("a0001", a0001, STATE_KINDS, 5, P1)):
            assert labels.num_states() == S
            run_group(fe, labels, binary, numeric, kinds, S, P, out, group)
            again = redrawn(hts, labels, S, rng, tmp)
            run_group(fe, again, binary, numeric, kinds, S, P, out, group + "2")
            assert out[group + "2/sil_default"][-1] and out[group + "2/dur"][-1].sum() == 0       # a flagged phone of 0 frames
    # Merlin's own file
    M = np.fromfile(os.path.join(tests, "nn_no_silence_lab_425", "arctic_a0001.lab"), dtype=np.float32).reshape(-1, 425)
    kept = out["a0001/default/phone"]
    assert M.shape == (578, 425) == (len(kept), 425) and np.array_equal(M[:, :416], P1[kept].astype(np.float32))
    assert np.array_equal(M[:, 416:], out["a0001/default/full"].astype(np.float32))
    out["merlin/sub"], out["merlin/phone"] = np.ascontiguousarray(M[:, 416:]), kept
    # the gather
    T = int(out["a0001/dur"].sum())
    lens = np.array([T - 37, T, T + 70], dtype=np.int64)
    out["gather/len"] = lens
    for k, n in enumerate(lens):
        y = rng.randn(n, 5)
        out["gather/y_%d" % k] = y
        for rx, regex in REGEX.items():
            idx = a0001.silence_frame_indices(regex).astype(np.int64)
            out["gather/%s/out_%d" % (rx, k)] = np.delete(y, idx[idx < n], axis=0)
    path = os.path.join(HERE, "silence_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
