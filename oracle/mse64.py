"""The unit-variance MLPG + MSE training step in float64, numpy and the C oracle only -- TEST INFRASTRUCTURE ONLY.

The anchor for every form of ``mlpg_hip_unit_mse_step`` (include/mlpg_hip.h); it does not load ``libmlpg_hip``.  For a
zero-padded batch ``means`` (B, Tmax, D), ``target`` (B, Tmax, sd), utterance b of length L_b and static dim d:

* y = MLPG(means) with unit variances, in the input dtype (``oracle.mlpg.mlpg_batch``): the trajectory the kernels
  round to before they form the error ("the trajectory as the caller sees it");
* status[b, d]: the same solve's verdict, 0 or k for "k-th leading minor not positive definite";
* loss = sum over live frames t < L_b of systems with status 0 of (float64(y) - float64(target))^2 / n_elems, in float64;
* grad = ``oracle.grad64.mlpg_grad64`` of dy = 2 (y - target) / n_elems on those frames and 0 elsewhere; the columns
  w * sd + d of a failed system are 0; rows at and past each length are exactly 0.

``n_elems`` defaults to B * Tmax * sd, as ``_hip.unit_mse_step`` does (nn.MSELoss over the padded batch).
"""
import numpy as np

from oracle.grad64 import mlpg_grad64
from oracle.mlpg import mlpg_batch


def unit_mse_step64(means, target, windows, lengths=None, n_elems=None):
    """Returns (y (B, Tmax, sd) in the input dtype, loss float, grad (B, Tmax, D) float64, status (B, sd) int32)."""
    means = np.ascontiguousarray(means)
    target = np.asarray(target)
    B, Tmax, D = means.shape
    nw = len(windows)
    assert D % nw == 0
    sd = D // nw
    assert target.shape == (B, Tmax, sd)
    if lengths is None:
        lengths = np.full(B, Tmax, dtype=np.int32)
    lengths = np.asarray(lengths, dtype=np.int32)
    assert lengths.shape == (B,) and (lengths >= 0).all() and (lengths <= Tmax).all()
    if n_elems is None:
        n_elems = float(B * Tmax * sd)
    # one utterance per (b, d), so that every system gets its own verdict (the oracle stops an utterance at its first
    # failing static dim, the kernels solve every system): (B, T, nw, sd) -> (B * sd, T, nw)
    per_sys = means.reshape(B, Tmax, nw, sd).transpose(0, 3, 1, 2).reshape(B * sd, Tmax, nw)
    ys, st, _ = mlpg_batch(np.ascontiguousarray(per_sys), np.ones(nw, dtype=means.dtype), windows, np.repeat(lengths, sd))
    y = np.ascontiguousarray(ys.reshape(B, sd, Tmax).transpose(0, 2, 1))
    status = st.reshape(B, sd)
    ok = status == 0
    y = np.where(ok[:, None, :], y, 0).astype(means.dtype)
    live = (np.arange(Tmax)[None, :, None] < lengths[:, None, None]) & ok[:, None, :]
    e = np.where(live, y.astype(np.float64) - np.where(live, target, 0).astype(np.float64), 0.0)
    loss = float((e * e).sum() / n_elems)
    dy = 2.0 * e / n_elems
    with np.errstate(divide="ignore", invalid="ignore"):      # a failed system's matrix is singular: its columns are set below
        grad = mlpg_grad64(None, dy, windows, lengths)
    bad_cols = np.tile(~ok, (1, nw))                            # column w * sd + d
    grad = np.where(bad_cols[:, None, :], 0.0, grad)
    return y, loss, grad, status
