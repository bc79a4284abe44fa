"""Writes tests/golden/frontend_ref.npz: what the reference's ``frontend.merlin.linguistic_features`` gives on its two example
labels (arctic_a0009_state.lab and arctic_a0009_phone.lab: 40 phones, 615 frames) with its 416-question set, for every
sub-phone kind its loaders accept (state alignment: full, minimal_frame, state_only, frame_only, uniform_state, coarse_coding;
phone alignment: minimal_phoneme, coarse_coding).

Run where the reference's source tree is at hand (its io/hts.py and frontend/merlin.py are loaded from their files through a
stand-in package object, because the reference's own __init__ does not import here, and run unchanged, on the CPU):

    python tests/golden/make_golden_frontend.py /path/to/reference

The file holds data only:
  P                     the phone-level matrix (40, 416) (add_frame_features=False, subphone_features=None; the same from both labels)
  cc                    the reference's coarse-coding table (3, 600), from scipy
  <group>/dur           the durations in frames, (40, 5) or (40, 1)
  <group>/phone         each frame's phone index (T,)
  <group>/<kind>        the sub-phone columns (T, F) of the reference's frame-level matrix; the generator asserts that the columns
                        in front of them equal P[phone], so they are not stored
Groups "state" and "phone" are the example labels as they are.  Groups "state2" and "phone2" are the same label strings with
redrawn durations -- states of 0 frames at the start, in the middle and at the end of a phone, and whole phones of 0 frames --
written out as temporary label files and read back by the reference's loader (hts.load does not refuse a line of zero length;
only HTSLabelFile.append in strict mode does, and the loader does not go through it)."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STATE_KINDS = ("full", "minimal_frame", "state_only", "frame_only", "uniform_state", "coarse_coding")
PHONE_KINDS = ("minimal_phoneme", "coarse_coding")
SHIFT = 50000


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    base = os.path.join(root, "nnmnkwii")
    for name in ("nnmnkwii", "nnmnkwii.io"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    hts = _load("nnmnkwii.io.hts", os.path.join(base, "io", "hts.py"))
    sys.modules["nnmnkwii.io"].hts = hts
    _load("nnmnkwii.frontend", os.path.join(base, "frontend", "__init__.py"))
    fe = _load("nnmnkwii.frontend.merlin", os.path.join(base, "frontend", "merlin.py"))
    return hts, fe


def durations_of(labels, S):
    d = (np.asarray(labels.end_times, dtype=np.int64) - np.asarray(labels.start_times, dtype=np.int64)) // SHIFT
    return d.reshape(-1, S)


def run_group(fe, labels, binary, numeric, kinds, S, P, out, group):
    dur = durations_of(labels, S)
    phone = np.repeat(np.arange(len(dur)), dur.sum(1))
    out[group + "/dur"], out[group + "/phone"] = dur, phone
    for kind in kinds:
        M = fe.linguistic_features(labels, binary, numeric, subphone_features=kind, add_frame_features=True)
        F = fe.get_frame_feature_size(kind)
        assert M.dtype == np.float64 and M.shape == (len(phone), P.shape[1] + F), (group, kind, M.shape)
        assert np.array_equal(M[:, :P.shape[1]], P[phone]), (group, kind)
        out["%s/%s" % (group, kind)] = np.ascontiguousarray(M[:, P.shape[1]:])
        print(group, kind, M.shape)


def redrawn(hts, labels, S, rng, tmp):
    """The same label strings with new durations, through a label file and the reference's loader."""
    n = len(labels) // S
    d = rng.randint(0, 5, size=(n, S))
    d[rng.rand(n, S) < 0.25] = 0
    d[3], d[n - 1] = 0, 0                            # whole phones of 0 frames, the last one among them
    d[0] = [0, 2, 0, 1, 0][:S] if S > 1 else [1]     # zero states at the start, in the middle and at the end of a phone
    d[5] = [1] + [0] * (S - 1)                       # a phone of one frame
    ends = np.cumsum(d.reshape(-1)) * SHIFT
    starts = np.concatenate([[0], ends[:-1]])
    path = os.path.join(tmp, "redrawn_%d.lab" % S)
    with open(path, "w") as fh:
        for s, e, c in zip(starts, ends, labels.contexts):
            fh.write("%d %d %s\n" % (s, e, c))
    got = hts.load(path)
    assert np.array_equal(durations_of(got, S), d)
    return got


def main(root):
    hts, fe = load_reference(root)
    data = os.path.join(root, "nnmnkwii", "util", "_example_data")
    binary, numeric = hts.load_question_set(os.path.join(data, "questions-radio_dnn_416.hed"))
    state = hts.load(os.path.join(data, "arctic_a0009_state.lab"))
    phone = hts.load(os.path.join(data, "arctic_a0009_phone.lab"))
    P = fe.linguistic_features(state, binary, numeric, subphone_features=None, add_frame_features=False)
    assert P.shape == (40, 416) and np.array_equal(P, fe.linguistic_features(phone, binary, numeric, subphone_features=None, add_frame_features=False))
    out = {"P": P, "cc": fe.compute_coarse_coding_features()}
    rng = np.random.RandomState(20240)
    with tempfile.TemporaryDirectory() as tmp:
        for group, labels, kinds, S in (("state", state, STATE_KINDS, 5), ("phone", phone, PHONE_KINDS, 1)):
            assert labels.num_states() == S
            run_group(fe, labels, binary, numeric, kinds, S, P, out, group)
            run_group(fe, redrawn(hts, labels, S, rng, tmp), binary, numeric, kinds, S, P, out, group + "2")
    assert out["state/dur"].sum() == 615 == out["phone/dur"].sum()
    path = os.path.join(HERE, "frontend_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
