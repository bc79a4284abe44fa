"""Writes tests/golden/norm_golden.npz: what the reference's meanvar, meanstd, minmax, scale, inv_scale, minmax_scale and
inv_minmax_scale give on the corpora of tests/norm_cases.py.

Run where the reference's source tree is at hand (it is loaded from its file, preprocessing/generic.py, with the scikit-learn
installed there -- 1.7.2 when this fixture was written -- running its meanvar unchanged):

    python tests/golden/make_golden_norm.py /path/to/reference

The file holds data only: the inputs (so that a change of the generator cannot move them), the reference's outputs, and the
reference's own worst distance from the exact truth (tools/norm_model.py: exact) in units of the error scales, over the columns
that are not constant (float64 cases; the reference does not promise exactness on a constant column).  The
reference's three slt_arctic Y_acoustic utterances (1859 x 187 float32) do not fit the size limit of a committed file; the case
"arctic" has their shape -- 187 columns, lengths 578, 675 and 606 cut to a sixth -- with the columns of the probe."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import norm_cases as C  # noqa: E402
from norm_cases import NM  # noqa: E402

# name -> (seed, lengths, D, dtype)
CASES = {
    "probe64": (1, [40, 117, 3, 90, 61, 200, 27], 12, np.float64),        # 7 utterances, 538 frames, 12 columns
    "probe32": (2, [40, 117, 3, 90, 61, 200, 27], 12, np.float32),
    "blocks64": (3, C.LENGTHS[5], 65, np.float64),
    "arctic": (4, [96, 112, 101], 187, np.float32),
}
FEATURE_RANGE = (0.01, 0.99)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_generic", os.path.join(root, "nnmnkwii", "preprocessing", "generic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root):
    R = load_reference(root)
    out = {}
    for name, (seed, lengths, D, dtype) in CASES.items():
        utts = C.corpus(seed, lengths, D, dtype)
        X, L = NM.pad(utts)
        out[name + "/X"], out[name + "/lengths"] = X, L
        mean, var, count = R.meanvar(utts, return_last_sample_count=True)
        std = R.meanstd(utts)[1]
        mn, mx = R.minmax(utts)
        truth = NM.exact(X, L)
        out[name + "/mean"], out[name + "/var"], out[name + "/count"], out[name + "/std"] = mean, var, np.int64(count), std
        out[name + "/min"], out[name + "/max"] = mn, mx
        out[name + "/ref_ratio"] = np.array(NM.ratios(mean, var, truth, skip_zero_scale=True) if dtype == np.float64 else (np.nan, np.nan))
        # streamed: the first two utterances, then the rest from that state (and through a padded batch with lengths)
        m2, v2, c2 = R.meanvar(utts[:2], return_last_sample_count=True)
        out[name + "/prior_mean"], out[name + "/prior_var"], out[name + "/prior_count"] = m2, v2, np.int64(c2)
        m3, v3, c3 = R.meanvar(X[2:], L[2:], m2, v2, c2, return_last_sample_count=True)
        out[name + "/streamed_mean"], out[name + "/streamed_var"], out[name + "/streamed_count"] = m3, v3, np.int64(c3)
        x = utts[1]
        out[name + "/scale"] = R.scale(x, mean, std)
        out[name + "/inv_scale"] = R.inv_scale(x, mean, std)
        out[name + "/minmax_scale"] = R.minmax_scale(x, mn, mx, feature_range=FEATURE_RANGE)
        min_, scale_ = R.minmax_scale_params(mn, mx, feature_range=FEATURE_RANGE)
        out[name + "/min_"], out[name + "/scale_"] = min_, scale_
        out[name + "/minmax_scale_params"] = R.minmax_scale(x, scale_=scale_, min_=min_)
        out[name + "/inv_minmax_scale"] = R.inv_minmax_scale(x, mn, mx, feature_range=FEATURE_RANGE)
        out[name + "/inv_minmax_scale_params"] = R.inv_minmax_scale(x, scale_=scale_, min_=min_)
    out["feature_range"] = np.array(FEATURE_RANGE)
    path = os.path.join(HERE, "norm_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for name in CASES:
        print(name, "reference against the truth (S_mean, S_var):", out[name + "/ref_ratio"])


if __name__ == "__main__":
    main(sys.argv[1])
