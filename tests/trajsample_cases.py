"""Shared by the K20 tests (draws from the trajectory distribution and the whitening map): the model, the inputs with NaN in every
padded row, the device calls, and the K20 error bound per system."""
import os
import sys

import numpy as np

import trajcov_cases as C
from trajcov_cases import TM

sys.path.insert(0, os.path.join(C.ROOT, "tools"))
import trajsample_model as SM  # noqa: E402

F32_EPS = 2.0 ** -24


def inputs(seed, K, B, Tmax, sd, wname, mode, dtype, lengths, tight=False):
    """(var, noise (K, B, Tmax, sd), mean (B, Tmax, sd)) of the dtype, NaN in every row at or past an utterance's length."""
    var = C.variances(seed, B, Tmax, sd, wname, mode, dtype, tight=tight)
    rng = np.random.RandomState(seed + 1)
    noise, mean = rng.randn(K, B, Tmax, sd).astype(dtype), rng.randn(B, Tmax, sd).astype(dtype)
    for b, T in enumerate(TM.live_frames(lengths, B, Tmax)):
        noise[:, b, T:] = np.nan
        mean[b, T:] = np.nan
        if mode == TM.VAR_FRAME:
            var[b, T:] = np.nan
    return var, noise, mean


def units(var, wname, lengths, B, Tmax, sd):
    """2^-53 cond_2(R) of every system, (B, sd) (1 for an utterance without frames)."""
    out = np.ones((B, sd))
    for b, T in enumerate(TM.live_frames(lengths, B, Tmax)):
        if T:
            v = None if var is None else (var if var.ndim == 1 else var[b])
            R = TM.dense_definition(v, C.WINDOWS[wname], int(T), sd)[0]
            out[b] = [C.cond2(R[d]) for d in range(sd)]
    return C.EPS * out


def within_bound(got, want64, unit, lengths, is_f32):
    """|got - want64| <= BOUND_C 2^-53 cond_2(R) max|want64| per system and draw over its live rows, plus one float32 rounding of
    the value where the dtype is float32; the rows at or past T must be exactly the model's (zeros).  want64: the model evaluated
    in float64 on the inputs as the device got them.  Returns the worst error in units of the bound."""
    K, B, Tmax, sd = want64.shape
    worst = 0.0
    for b, T in enumerate(TM.live_frames(lengths, B, Tmax)):
        T = int(T)
        assert np.array_equal(got[:, b, T:], np.zeros((K, Tmax - T, sd), dtype=got.dtype)), "rows at or past T must be zero"
        if T:
            w = want64[:, b, :T]
            tol = SM.BOUND_C * unit[b][None, None, :] * np.abs(w).max(axis=1, keepdims=True) + (F32_EPS * np.abs(w) if is_f32 else 0.0)
            err = np.abs(got[:, b, :T].astype(np.float64) - w)
            assert (err <= tol).all(), (b, float((err / tol).max()))
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


def dev(a, slack=0):
    """The array on the device; slack > 0: as a column slice of a tensor `slack` columns wider (NaN in the foreign columns)."""
    import torch
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not slack or t.dim() < 2:
        return t
    wide = torch.full(t.shape[:-1] + (t.shape[-1] + slack,), float("nan"), dtype=t.dtype, device="cuda")
    view = wide[..., 1:1 + t.shape[-1]]
    view.copy_(t)
    return view


def dev_lengths(lengths):
    import torch
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device="cuda")
