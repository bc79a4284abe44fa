"""Multi-stream MLPG with its gradients w.r.t. the means AND the variances in float64, numpy only -- TEST INFRASTRUCTURE ONLY.

The anchor of tests/test_backward_streams_gpu.py: tests/vargrad64.mlpg_var_grad64 on every dynamic stream's own column slice,
and the pass-through rule for the others, scattered into arbitrary in_col / out_col layouts.  It loads no compiled library.

A stream is a dict with in_col, out_col, static_dim and windows (a list of (l, u, coeff) triples; None or [] for a pass-through
stream).  Input rows are (B, T, ld_in): a dynamic stream owns columns [in_col, in_col + len(windows) * static_dim), window-major;
a pass-through stream [in_col, in_col + static_dim).  Output rows are (B, T, ld_out): stream k at [out_col, out_col + static_dim).

* dynamic stream: (y, grad_mean, grad_var) of mlpg_var_grad64 on its slice;
* pass-through stream: y = means and grad_mean = grad_out on live rows, 0 at and past each length; grad_var = 0; its variance
  columns are never read;
* columns that belong to no stream: 0 in every result (`owned_in` / `owned_out` say which columns the streams own).
"""
import numpy as np

import vargrad64


def stream_cols(s):
    """The input columns of a stream."""
    nw = len(s["windows"]) if s["windows"] else 0
    return np.arange(s["in_col"], s["in_col"] + max(nw, 1) * s["static_dim"])


def owned(streams, ld_in, ld_out):
    """Boolean (ld_in,), (ld_out,): the columns some stream owns."""
    oi, oo = np.zeros(ld_in, dtype=bool), np.zeros(ld_out, dtype=bool)
    for s in streams:
        oi[stream_cols(s)] = True
        oo[s["out_col"]:s["out_col"] + s["static_dim"]] = True
    return oi, oo


def multi_stream_grad64(means, var, grad_out, streams, lengths=None):
    """(y (B, T, ld_out), grad_mean (B, T, ld_in), grad_var (B, T, ld_in) or None) in float64.

    means (B, T, ld_in); var of the same shape, a global (ld_in,) vector or None (unit variances: grad_var is None); grad_out
    (B, T, ld_out); lengths (B,) or None.  With a global vector grad_var holds every frame's contribution (the gradient of the
    vector is its sum over the first two axes), which is what mlpg_var_grad64 gives for per-frame arrays of the same values: the
    reciprocals are taken in var's dtype either way."""
    means = np.asarray(means)
    grad_out = np.asarray(grad_out)
    B, T, ld_in = means.shape
    ld_out = grad_out.shape[2]
    assert grad_out.shape[:2] == (B, T)
    if lengths is None:
        lengths = np.full(B, T, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    live = (np.arange(T)[None, :] < lengths[:, None])[:, :, None]
    y = np.zeros((B, T, ld_out))
    gm = np.zeros((B, T, ld_in))
    gv = None if var is None else np.zeros((B, T, ld_in))
    for s in streams:
        sd, ic, oc = s["static_dim"], s["in_col"], s["out_col"]
        if sd == 0:
            continue
        g = np.ascontiguousarray(grad_out[:, :, oc:oc + sd])
        if not s["windows"]:
            y[:, :, oc:oc + sd] = np.where(live, means[:, :, ic:ic + sd].astype(np.float64), 0.0)
            gm[:, :, ic:ic + sd] = np.where(live, g.astype(np.float64), 0.0)
            continue
        cols = stream_cols(s)
        m = np.ascontiguousarray(means[:, :, cols])
        if var is None:
            v = np.ones(m.shape, dtype=means.dtype)
        elif np.ndim(var) == 1:
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(var)[cols], m.shape))
        else:
            v = np.ascontiguousarray(np.asarray(var)[:, :, cols])
        ys, gms, gvs = vargrad64.mlpg_var_grad64(m, v, g, s["windows"], lengths)
        y[:, :, oc:oc + sd] = ys
        gm[:, :, cols] = gms
        if gv is not None:
            gv[:, :, cols] = gvs
    return y, gm, gv
