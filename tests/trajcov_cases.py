"""Shared by the K19 tests (trajectory covariance and likelihood): the window sets, the inputs and the error bound."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import trajcov_model as TM  # noqa: E402

WINDOWS = {
    "static": [(0, 0, np.array([1.0]))],
    "std2": [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))],
    "std3": [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))],
    "asym": [(0, 0, np.array([1.0])), (1, 0, np.array([-1.0, 1.0]))],
}
MODES = (TM.VAR_FRAME, TM.VAR_GLOBAL, TM.VAR_UNIT)
EPS = TM.EPS


def variances(seed, B, Tmax, sd, wname, mode, dtype=np.float64, tight=False):
    """Variances in [0.5, 2) of the mode's shape (None for unit ones); tight: the dynamic windows' 100 times smaller."""
    nw = len(WINDOWS[wname])
    if mode == TM.VAR_UNIT:
        return None
    rng = np.random.RandomState(seed)
    v = 0.5 + 1.5 * rng.rand(*((B, Tmax, nw * sd) if mode == TM.VAR_FRAME else (nw * sd,)))
    if tight:
        v[..., sd:] *= 0.01
    return v.astype(dtype)


def features(seed, B, Tmax, D, dtype=np.float64):
    return np.random.RandomState(seed).randn(B, Tmax, D).astype(dtype)


def cond2(R):
    return float(np.linalg.cond(R)) if R.shape[0] else 1.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def logdet_bound(var, wname, T, sd):
    """(T + 4) 2^-53 sum_t |log D_t| per dim: the sequential sum of T terms plus log's last-place error."""
    tau = TM.precisions(var, WINDOWS[wname], T, sd)
    fac, _, _ = TM.factor(TM.assemble(tau, WINDOWS[wname]))
    with np.errstate(all="ignore"):
        return (T + 4) * EPS * np.abs(np.log(fac[:, 0])).sum(axis=0) if T else np.zeros(sd)
