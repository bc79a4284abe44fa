"""Inputs shared by the tests of MLPG with gv (tests/test_gvmlpg_*.py): window sets, random padded batches whose y_in is the
maximum-likelihood trajectory of the model's own (P, r), gv statistics above the trajectory's gv (over-smoothing is what the
method is for), and the tolerance of kernel against model."""
import os
import sys

import numpy as np
from scipy.linalg import solveh_banded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gvmlpg_model as GV  # noqa: E402

EPS = np.finfo(np.float64).eps
WINDOWS = {
    "static": [(0, 0, np.array([1.0]))],
    "std2": [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))],
    "std3": [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))],
}
# Kernel against the model run in long double, n_iter = 100, on the shapes of tests/test_gvmlpg_host_cpu.py: the worst
# |y - y_ref| / (eps max|y|) of the host build was 3.43, recorded rounded up (float64 storage).  The bound is 8 times that; it must stay
# below 1e-10 / eps = 4.5e5 (a wrong halo, a dropped term or a wrong omega sits above 1e-4 max|y|).
WORST_RATIO = 3.44
BOUND_RATIO = 8 * WORST_RATIO
assert BOUND_RATIO * EPS <= 1e-10
EPS32 = float(np.finfo(np.float32).eps)


def ml_trajectory(mean, var, windows, lengths):
    """(B, Tmax, sd) float64: the solution of P y = r per system from the model's banded assembly; 0 on pad frames."""
    B, Tmax, D = mean.shape
    nw = len(windows)
    sd = D // nw
    mode = GV.var_mode_of(var)
    live = GV.live_frames(lengths, B, Tmax)
    y = np.zeros((B, Tmax, sd))
    for b in range(B):
        T = int(live[b])
        for d in range(sd if T else 0):
            mu = np.stack([mean[b, :T, w * sd + d].astype(np.float64) for w in range(nw)])
            tau = GV.precisions(var[b] if mode == GV.VAR_FRAME else var, mode, windows, T, sd, d)
            pk, r = GV.system_banded(mu, tau, windows)
            y[b, :T, d] = solveh_banded(pk[:min(3, T)], r, lower=True)
    return y


def make_case(seed, B, Tmax, sd, wname="std3", var_mode=GV.VAR_FRAME, dtype=np.float64, lengths=None, tight=False):
    """dict(mean, var, y_in, gv_mean, gv_prec, windows, lengths): arrays of `dtype` (the gv statistics float64)."""
    rng = np.random.RandomState(seed)
    windows = WINDOWS[wname]
    D = sd * len(windows)
    t = np.arange(Tmax)[None, :, None]
    static = np.sin(0.11 * t + rng.rand(B, 1, sd) * 6) * (1 + rng.rand(1, 1, sd)) + 0.3 * rng.randn(B, Tmax, sd)
    mean = np.concatenate([static] + [0.3 * rng.randn(B, Tmax, sd) for _ in windows[1:]], axis=2)
    scale = 0.01 if tight else 1.0
    if var_mode == GV.VAR_FRAME:
        var = (rng.rand(B, Tmax, D) + 0.1) * scale
        var[:, :, :sd] = rng.rand(B, Tmax, sd) + 0.1           # the dynamic variances are the ones that tighten
    elif var_mode == GV.VAR_GLOBAL:
        var = (rng.rand(D) + 0.1) * scale
        var[:sd] = rng.rand(sd) + 0.1
    else:
        var = None
    mean = mean.astype(dtype)
    var = None if var is None else var.astype(dtype)
    y = ml_trajectory(mean, var, windows, lengths)
    live = GV.live_frames(lengths, B, Tmax)
    v = np.array([[y[b, :live[b], d].var() if live[b] else 0.0 for d in range(sd)] for b in range(B)])
    gv_mean = 1.6 * v[live > 0].mean(axis=0) + 0.05 if (live > 0).any() else np.ones(sd)
    gv_prec = 1.0 / (0.2 * gv_mean) ** 2
    return dict(mean=mean, var=var, y_in=y.astype(dtype), gv_mean=gv_mean, gv_prec=gv_prec, windows=windows, lengths=lengths,
                B=B, Tmax=Tmax, sd=sd, D=D, dtype=dtype)


def model(case, n_iter=100, step=None, init=1, omega_scale=1.0, work=np.float64, form="banded"):
    return GV.gv_ascent_padded(case["mean"], case["var"], case["windows"], case["lengths"], case["y_in"], case["gv_mean"],
                               case["gv_prec"], omega_scale, n_iter, step, init, form=form, work=work)


def tolerance(y_ref, dtype):
    """Bound on |y - y_ref| per element: BOUND_RATIO eps max|y|, plus half a float32 ulp of max|y| for float32 storage (the output
    cast; the arithmetic is float64 either way)."""
    big = float(np.abs(np.asarray(y_ref, dtype=np.float64)).max()) if y_ref.size else 0.0
    return BOUND_RATIO * EPS * big + (EPS32 * big if dtype == np.float32 else 0.0)
