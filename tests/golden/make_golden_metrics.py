"""Writes tests/golden/metrics_ref.npz: what the reference's melcd, mean_squared_error, lf0_mean_squared_error and vuv_error give
on the batches of tests/metrics_cases.py (golden_inputs: seeded float64 and float32), with and without lengths, for the shapes
(D,), (T, D), (B, T, D), (B, T) and (B, T, 1), in the log and the linear F0 domain.

Run where the reference's source tree is at hand (its metrics/__init__.py is loaded from its file and run unchanged, on the CPU):

    python tests/golden/make_golden_metrics.py /path/to/reference

The file holds data only: the inputs (so that a change of the generator cannot move them) and the reference's outputs."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_cases as C  # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_metrics", os.path.join(root, "nnmnkwii", "metrics", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root):
    R = load_reference(root)
    out = {}
    for name in C.G_CASES:
        X, Y, lengths = C.golden_inputs(name)
        out[name + "/X"], out[name + "/Y"], out[name + "/lengths"] = X, Y, lengths
        for key, value in C.golden_calls(R, X, Y, lengths).items():
            out["%s/%s" % (name, key)] = np.float64(value)
            print(name, key, value)
    path = os.path.join(HERE, "metrics_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
