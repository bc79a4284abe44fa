"""MLPG on MI355X behind the signatures of ``nnmnkwii.paramgen``.

Host-side mirror of /root/reference/nnmnkwii/paramgen/_mlpg.py.  All numerical
work is done by the HIP kernels in ``nnmnkwii_amd/csrc`` through the C ABI in
``include/mlpg_hip.h``; this module only validates arguments the way the
reference does, moves arrays to the GPU and maps kernel status words to the
reference's exceptions.
"""
import numpy as np

from .. import _hip

__all__ = [
    "build_win_mats",
    "mlpg",
    "mlpg_grad",
    "unit_variance_mlpg_matrix",
    "reshape_means",
    "full_window_mat",
    "mlpg_batch",
    "multi_stream_mlpg",
    "gv",
    "gv_stats",
    "mlpg_gv",
    "mlpg_gv_batch",
    "mlpg_covariance_batch",
    "mlpg_variance",
    "mlpg_logdet",
    "mlpg_sample_batch",
    "mlpg_sample",
    "mlpg_whiten_batch",
]


class BandMat(object):
    """Minimal stand-in for the reference's bandmat.BandMat container
    (paramgen/_bandmat/core.pyx:20-87): ``l``, ``u``, ``data``, ``transposed``,
    ``.T``, ``.size`` and ``.full()``.  LAPACK band layout:
    ``full[j + i, j] == data[u + i, j]`` for ``i in [-u, l]``.
    """

    def __init__(self, l, u, data, transposed=False):
        self.l = l
        self.u = u
        self.data = data
        self.transposed = transposed
        assert self.l >= 0 and self.u >= 0
        assert self.data.ndim == 2 and self.data.shape[0] == self.l + self.u + 1

    def __repr__(self):
        return "BandMat(%r, %r, %r, transposed=%r)" % (self.l, self.u, self.data, self.transposed)

    @property
    def size(self):
        return self.data.shape[1]

    @property
    def T(self):
        return BandMat(self.u, self.l, self.data, transposed=not self.transposed)

    def full(self):
        l, u = (self.u, self.l) if self.transposed else (self.l, self.u)
        n = self.size
        m = np.zeros((n, n))
        for i in range(-u, l + 1):
            j = np.arange(max(0, -i), max(0, n + min(0, -i)))
            m[j + i, j] = self.data[u + i, j]
        return m.T if self.transposed else m


def build_win_mats(windows, T):
    """Window matrices as banded containers (reference: paramgen/_mlpg.py:13-50).

    ``W[t, t+k] = win_coeff[l+k]`` for ``k in [-l, u]``, one ``T x T`` Toeplitz
    band per window.
    """
    win_mats = []
    for l, u, win_coeff in windows:
        assert l >= 0 and u >= 0
        assert len(win_coeff) == l + u + 1
        data = np.tile(np.reshape(np.asarray(win_coeff, dtype=np.float64), (l + u + 1, 1)), T)
        win_mats.append(BandMat(u, l, data).T)
    return win_mats


def full_window_mat(win_mats, T):
    """Concatenated dense window matrix ``(T*num_windows, T)`` (paramgen/_mlpg.py:284-294)."""
    return np.concatenate([w.full() for w in win_mats], axis=0) if len(win_mats) else np.zeros((0, T))


def _as_float(a):
    a = np.asarray(a)
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    return a


def _match_dtypes(m, v):
    """Means and variances of different float dtypes, as the reference treats them (_mlpg.py:180-188): the reciprocal
    is taken in the VARIANCES' dtype, everything after it in float64, the result is cast to the means' dtype.
    float64 means + float32 variances: the float32 reciprocal is taken here (one elementwise pass) and handed to the
    float64 kernel as an exactly invertible float64 variance; float32 means + float64 variances: float64 kernel."""
    torch = _hip.torch_mod()
    if v.dtype == m.dtype:
        return m, v
    if m.dtype == torch.float64 and v.dtype == torch.float32:
        tau32 = torch.reciprocal(v)                        # float32 reciprocal, correctly rounded
        return m, torch.reciprocal(tau32.to(torch.float64))
    return m.to(torch.float64), v.to(torch.float64)


def mlpg_batch(means, variances, windows, lengths=None, algo=_hip.ALGO_AUTO, check=True, device=None):
    """Batched MLPG over a zero-padded ``(B, Tmax, D)`` batch -- the GPU-native
    form of the reference's per-utterance loop (util/__init__.py:44-66).

    ``means``/``variances`` are numpy arrays or CUDA tensors (float32/float64);
    ``variances`` may be ``(B, Tmax, D)``, a global ``(D,)`` or ``None`` (unit
    variances).  ``lengths`` (B,) gives the valid frames per utterance; output
    frames beyond it are zero.  Returns the same kind of object as ``means``,
    shape ``(B, Tmax, D // len(windows))``.  numpy input: ``device`` may also be
    a list of GPU indices or ``"all"`` -- the utterance chunks are then dealt
    round-robin over those devices from this one process (mlpg_hip_forward_host_multi).
    """
    if isinstance(means, np.ndarray) or not hasattr(means, "is_cuda"):
        return _mlpg_batch_host(means, variances, windows, lengths, algo, check, device)
    torch = _hip.torch_mod()
    dev = _hip.require_gpu(means.device if means.is_cuda else device)
    m = means.to(dev).contiguous()
    assert m.dim() == 3
    out_dtype = m.dtype
    if variances is None:
        v = None
    else:
        v = (variances if torch.is_tensor(variances) else
             torch.from_numpy(np.ascontiguousarray(_as_float(variances)))).to(dev).contiguous()
        m, v = _match_dtypes(m, v)
    if v is not None and v.dim() != 1:
        assert v.shape == m.shape                         # paramgen/_mlpg.py:171
    L = None
    if lengths is not None:
        L = torch.as_tensor(np.asarray(lengths) if not torch.is_tensor(lengths) else lengths).to(
            device=dev, dtype=torch.int32).contiguous()
    out, status = _hip.forward(m, v, windows, L, algo=algo, want_status=check)
    if check:
        _hip.raise_on_status(status, out.shape[-1])
    if out.dtype != out_dtype:
        out = out.to(out_dtype)                            # output dtype = dtype of the means (_mlpg.py:166,183)
    return out


def _mlpg_batch_host(means, variances, windows, lengths, algo, check, device):
    """numpy in -> numpy out through the host-pointer entry point of the C ABI (no torch): chunked, with the PCIe
    transfers overlapped with the kernels (include/mlpg_hip.h mlpg_hip_forward_host)."""
    m = np.ascontiguousarray(_as_float(means))
    assert m.ndim == 3
    out_dtype = m.dtype
    v = None
    if variances is not None:
        v = np.ascontiguousarray(_as_float(variances))
        if v.ndim != 1:
            assert v.shape == m.shape                      # paramgen/_mlpg.py:171
        if v.dtype != m.dtype:                             # see _match_dtypes: reciprocal in the variances' dtype
            if m.dtype == np.float64:
                v = 1.0 / (np.float32(1.0) / v).astype(np.float64)
            else:
                m = m.astype(np.float64)
    # default: the process's current GPU, not GPU 0; a list of indices or "all": the chunks dealt over those devices
    out, status = _hip.forward_host(m, v, windows, lengths, algo=algo, device=device)
    if check and status.any():
        _raise_host_status(status)
    return out if out.dtype == out_dtype else out.astype(out_dtype)


def _raise_host_status(status):
    """The reference's LinAlgError (linalg.pyx:79-82) for the first failing (utterance, dim) system of a host-memory call."""
    st = status.ravel()
    bad = np.flatnonzero(st)
    if bad.size:
        k = int(st[bad[0]])
        if k > 0:
            raise np.linalg.LinAlgError("%d-th leading minor not positive definite" % k)
        raise np.linalg.LinAlgError("the blocked elimination broke down (numerically singular system)" if k == -2
                                    else "internal error: inter-workgroup wait timed out")


def stream_list(windows, stream_sizes, has_dynamic_features, error=AssertionError):
    """The ``[(in_col, static_dim, windows)]`` table of multi_stream_mlpg's arguments (also autograd.multi_stream_mlpg's, which
    asks for ValueError): streams side by side, ``windows`` one list for all dynamic streams or one list per stream."""
    per_stream = len(windows) > 0 and len(windows[0]) > 0 and isinstance(windows[0][0], (tuple, list))
    if per_stream and len(windows) != len(stream_sizes):
        raise error("one window list per stream expected (%d streams, %d lists)" % (len(stream_sizes), len(windows)))
    streams, col = [], 0
    for k, (size, dyn) in enumerate(zip(stream_sizes, has_dynamic_features)):
        if dyn:
            w = windows[k] if per_stream else windows
            if size % len(w) != 0:
                raise error("stream %d: %d columns are not a multiple of the %d windows" % (k, size, len(w)))
            streams.append((col, size // len(w), w))
        else:
            streams.append((col, size, None))
        col += size
    return streams


def multi_stream_mlpg(inputs, variances, windows, stream_sizes, has_dynamic_features, lengths=None,
                      algo=_hip.ALGO_AUTO, check=True, device=None):
    """MLPG over every stream of a multi-stream acoustic feature matrix in ONE call.

    The Merlin-style layout the reference's data sources use (util/files.py:90-115): the feature
    axis is ``[stream 0 | stream 1 | ...]`` with ``stream_sizes`` columns each (e.g. mgc 180 | lf0 3 |
    vuv 1 | bap 15); a stream with dynamic features is window-major (static, delta, delta-delta) and
    is replaced by its maximum-likelihood static trajectory ``paramgen.mlpg(stream, var, windows)``;
    a stream without (``has_dynamic_features[k]`` False, e.g. vuv) is copied through.  This is the
    per-stream, per-utterance loop users write with ``util.apply_each2d_padded`` (util/__init__.py:
    44-66), done on the GPU directly on the padded ``(N, Tmax, D)`` batch, each stream consumed in
    place (no slicing copies).

    inputs: ``(T, D)`` or ``(N, Tmax, D)`` numpy array / CUDA tensor; variances: same shape, a
    global ``(D,)`` or None (unit); windows: one window list for all dynamic streams or a list of
    window lists, one per stream; lengths: valid frames per utterance (3-D input).  Returns the
    static features of all streams side by side, same kind and rank as ``inputs``.
    """
    torch = _hip.torch_mod()
    is_np = not torch.is_tensor(inputs)
    dev = _hip.require_gpu(device if is_np or not inputs.is_cuda else inputs.device)
    m = torch.from_numpy(np.ascontiguousarray(_as_float(inputs))).to(dev) if is_np else inputs.to(dev).contiguous()
    two_d = m.dim() == 2
    if two_d:
        m = m[None]
    assert m.dim() == 3
    D = m.shape[-1]
    assert len(stream_sizes) == len(has_dynamic_features) and sum(stream_sizes) == D
    out_dtype = m.dtype
    if variances is None:
        v = None
    else:
        v = (variances if torch.is_tensor(variances) else
             torch.from_numpy(np.ascontiguousarray(_as_float(variances)))).to(dev).contiguous()
        m, v = _match_dtypes(m, v)
    if v is not None and v.dim() != 1:
        if two_d and v.dim() == 2:
            v = v[None]
        assert v.shape == m.shape
    streams = stream_list(windows, stream_sizes, has_dynamic_features)
    L = None
    if lengths is not None:
        L = torch.as_tensor(np.asarray(lengths) if not torch.is_tensor(lengths) else lengths).to(
            device=dev, dtype=torch.int32).contiguous()
    out, status = _hip.forward_streams(m, v, streams, L, algo=algo, want_status=check)
    if check:
        _hip.raise_on_status(status, out.shape[-1])
    if out.dtype != out_dtype:
        out = out.to(out_dtype)
    if two_d:
        out = out[0]
    return out.cpu().numpy() if is_np else out


def mlpg(mean_frames, variance_frames, windows):
    """Maximum Likelihood Parameter Generation, ``(T, D) -> (T, static_dim)``.

    Drop-in for ``nnmnkwii.paramgen.mlpg`` (paramgen/_mlpg.py:92-199): same
    arguments, same output dtype (that of ``mean_frames``), accepts per-frame
    ``(T, D)`` or global ``(D,)`` variances, raises ``AssertionError`` on a shape
    mismatch and ``numpy.linalg.LinAlgError`` ("k-th leading minor not positive
    definite") when a system is not positive definite.

    Windows: what the reference's ``build_win_mats`` accepts (paramgen/_mlpg.py:13-50) within the library's compile-time
    limits -- at most 8 windows, window extents ``l, u <= 4`` (half-bandwidth of ``P`` <= 8), at most 48 coefficients in
    total (csrc/common.h: kMaxWindows, kMaxExtent, kMaxCoef); beyond those the call raises ``HipExtensionError`` (the
    reference itself has no limit).  Which kernel a window set gets (``MLPG_HIP_ALGO_AUTO``; DESIGN.md "AUTO routing",
    measured in profiles/r05_auto_routing.json):

    * extents <= 1 (the usual static / delta / delta-delta set, also one or two windows): the fast kernels -- strip,
      wave-per-system, constant-coefficient, FIR -- at 0.4-0.5 of the HBM roofline for wide streams; batches of narrow
      streams (1-32 static dims: lf0, bap) ride the strip kernel with its lanes over several utterances;
    * extents of 2 (the reference's 5-tap test windows, tests/test_paramgen.py:21-26), up to three windows: the chunked
      kernel, which reads the inputs twice: 0.22 of the roofline;
    * more than three windows with an extent of 2, or extents of 3-4: the natural-order kernel, one lane per system and
      the factor through HBM: 0.04-0.07 of the roofline (correct, slow).
    """
    mean_frames = np.asarray(mean_frames)
    variance_frames = np.asarray(variance_frames)
    dtype = mean_frames.dtype
    T, D = mean_frames.shape
    if not (variance_frames.ndim == 1 and variance_frames.shape[0] == D):
        assert mean_frames.shape == variance_frames.shape
        variance_frames = variance_frames[None]
    y = mlpg_batch(mean_frames[None], variance_frames, windows)
    return y[0].astype(dtype, copy=False)


def mlpg_grad(mean_frames, variance_frames, windows, grad_output):
    """Gradient of MLPG w.r.t. the means, ``float32 (T, D)``.

    Drop-in for ``nnmnkwii.paramgen.mlpg_grad`` (paramgen/_mlpg.py:202-281).
    The reference solves a dense ``T x T`` right-hand side per (dim, window);
    the HIP kernel computes the same quantity in O(T):
    ``grad[:, w*sd+d] = tau_w * (W_w P_d^-1 o_d)``.  ``variance_frames`` ``(T, D)``, or a global ``(D,)`` (the reference
    leaves that broadcast to its caller, autograd/_impl/mlpg.py:196-197).
    """
    mean_frames = np.asarray(mean_frames)
    v = np.ascontiguousarray(_as_float(variance_frames))
    T, D = mean_frames.shape
    if v.ndim == 2:
        assert v.shape == (T, D)
        v = v[None]
    # numpy in -> numpy out through the host-memory entry point (mlpg_hip_backward_host: the library's short path -- no torch
    # tensor, one C call; the arithmetic runs in the variances' dtype class as before: float32 variances -> float32 inputs)
    go = np.ascontiguousarray(np.asarray(grad_output), dtype=v.dtype)
    assert go.shape == (T, D // len(windows))
    grad, status = _hip.backward_host(v, go[None], windows, D, out_dtype=np.float32)
    if status.any():
        _raise_host_status(status)
    return grad[0]


# ---- MLPG with the likelihood of the trajectory's gv (Toda, Black, Tokuda 2007, section IV) --------------------
def _as_device_batch(X, dev=None):
    """numpy or tensor, float32 / float64 -> (CUDA tensor, was it numpy)."""
    torch = _hip.torch_mod()
    is_np = not torch.is_tensor(X)
    dev = _hip.require_gpu(dev if is_np or not X.is_cuda else X.device)
    return (torch.from_numpy(np.ascontiguousarray(_as_float(X))).to(dev) if is_np else X.to(dev)), is_np


def _device_lengths(lengths, dev):
    if lengths is None:
        return None
    torch = _hip.torch_mod()
    return torch.as_tensor(np.asarray(lengths) if not torch.is_tensor(lengths) else lengths).to(device=dev, dtype=torch.int32).contiguous()


def gv(X, lengths=None):
    """The gv of features: the variance over time of each dimension of one utterance.  ``X`` (T, sd) -> (sd,), or a zero-padded
    batch (B, Tmax, sd) with ``lengths`` (B,) -> (B, sd); float64, numpy for numpy input, a CUDA tensor for a CUDA tensor.  An
    utterance without live frames gives 0.  One launch of ``mlpg_hip_gv``."""
    x, is_np = _as_device_batch(X)
    two_d = x.dim() == 2
    if two_d:
        if lengths is not None:
            raise ValueError("gv: lengths go with a padded (B, Tmax, sd) batch")
        x = x[None]
    if x.dim() != 3:
        raise ValueError("gv takes (T, sd) features or a padded (B, Tmax, sd) batch")
    out = _hip.gv(x, _device_lengths(lengths, x.device))
    if two_d:
        out = out[0]
    return out.cpu().numpy() if is_np else out


def gv_stats(X, lengths):
    """(gv_mean, gv_var): float64 (sd,) mean and variance of the gv over the utterances of a padded batch that have live frames
    (``lengths > 0``) -- what ``mlpg_gv`` takes.  The gv comes from the device (``gv``), the two moments are taken on the host."""
    g = gv(X, lengths)
    g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
    keep = np.asarray(lengths if not hasattr(lengths, "cpu") else lengths.cpu().numpy()) > 0
    if not keep.any():
        raise ValueError("gv_stats: no utterance has live frames")
    return g[keep].mean(axis=0), g[keep].var(axis=0)


def _gv_options(gv_mean, gv_var, sd, n_iter, step, init, omega_scale):
    """The checks of mlpg_gv / mlpg_gv_batch that need no device: ValueError, or (gv_mean, gv_prec) as float64 (sd,) arrays."""
    gm, gvv = np.asarray(gv_mean, dtype=np.float64).ravel(), np.asarray(gv_var, dtype=np.float64).ravel()
    if gm.shape != (sd,) or gvv.shape != (sd,):
        raise ValueError("gv_mean and gv_var must have one entry per static dimension (%d), got %d and %d" % (sd, gm.size, gvv.size))
    if not (gvv > 0).all():
        raise ValueError("gv_var must be positive (entry %d is %r)" % (int(np.flatnonzero(~(gvv > 0))[0]), float(gvv[~(gvv > 0)][0])))
    if init not in _hip.GV_INIT:
        raise ValueError("init must be 'scaled' or 'given', got %r" % (init,))
    if not (0 <= int(n_iter) <= 100000):
        raise ValueError("n_iter must be in [0, 100000], got %r" % (n_iter,))
    if not (omega_scale > 0 and np.isfinite(omega_scale)):
        raise ValueError("omega_scale must be positive and finite, got %r" % (omega_scale,))
    if step is not None and not np.isfinite(step):
        raise ValueError("step must be finite (None or <= 0: the derived step), got %r" % (step,))
    return gm, 1.0 / gvv


def raise_on_gv_status(status, report, step):
    """ValueError for the first (utterance, dim) whose ascent failed: status 1 (non-finite) or 2 (no ascent)."""
    st = status.cpu().numpy()
    bad = np.argwhere(st != 0)
    if len(bad):
        b, d = (int(i) for i in bad[0])
        if st[b, d] == 1:
            raise ValueError("mlpg_gv: a non-finite value appeared in utterance %d, dim %d" % (b, d))
        rep = report[b, d].cpu().numpy()
        raise ValueError("mlpg_gv: no ascent in utterance %d, dim %d (the likelihood went from %r to %r): the step %s is too large"
                         % (b, d, float(rep[0]), float(rep[1]), "derived by the kernel" if step is None or step <= 0 else repr(step)))


def mlpg_gv_batch(means, variances, windows, gv_mean, gv_var, lengths=None, n_iter=100, step=None, init="scaled", omega_scale=1.0,
                  algo=_hip.ALGO_AUTO, check=True, return_report=False, device=None):
    """MLPG that also maximises the likelihood of the trajectory's gv, over a zero-padded ``(B, Tmax, D)`` batch: the plain
    maximum-likelihood trajectory (``mlpg_batch``: any route) followed, in place, by ``n_iter`` steps of steepest ascent on
    ``L(y) = omega (-1/2 y'Py + y'r) - 1/2 (v(y) - gv_mean)^2 / gv_var``, ``omega = omega_scale / (2 T)``, in ONE further launch
    (``mlpg_hip_gv_ascent``).  ``gv_mean``, ``gv_var`` (static_dim,): mean and variance of the gv of natural speech
    (``gv_stats``); the gv density is diagonal.  ``init``: "scaled" (the trajectory scaled about its mean to the gv ``gv_mean``;
    with ``n_iter=0`` the familiar variance-scaling filter) or "given"; ``step``: None for the step the kernel derives per system.
    Inputs and result as ``mlpg_batch`` (numpy -> numpy, CUDA tensor -> CUDA tensor, the dtype of the means).  ``check``: raise
    ``LinAlgError`` as ``mlpg_batch`` does and ``ValueError`` where the ascent met a non-finite value or did not ascend.
    ``return_report``: also return ``(report (B, sd, 4): L(start), L(final), v(ML trajectory), v(final); status (B, sd))``.
    Window extents of at most 1 and ``Tmax <= _hip.gv_max_frames()``."""
    nw = _hip._nw(windows)
    D = np.shape(means)[-1]
    if nw < 1 or D % nw:
        raise ValueError("D = %d is not a multiple of the %d windows" % (D, nw))
    gm, gp = _gv_options(gv_mean, gv_var, D // nw, n_iter, step, init, omega_scale)
    torch = _hip.torch_mod()
    m, is_np = _as_device_batch(means, device)
    dev = m.device
    m = m.contiguous()
    assert m.dim() == 3
    out_dtype = m.dtype
    v = None
    if variances is not None:
        v = (variances if torch.is_tensor(variances) else
             torch.from_numpy(np.ascontiguousarray(_as_float(variances)))).to(dev).contiguous()
        m, v = _match_dtypes(m, v)
    L = _device_lengths(lengths, dev)
    y = mlpg_batch(m, v, windows, L, algo=algo, check=check)
    y, report, status = _hip.gv_ascent(m, v, windows, y, torch.from_numpy(gm).to(dev), torch.from_numpy(gp).to(dev), L,
                                       n_iter=n_iter, step=step, init=init, omega_scale=omega_scale)
    if check:
        raise_on_gv_status(status, report, step)
    if y.dtype != out_dtype:
        y = y.to(out_dtype)
    if is_np:
        y, report, status = y.cpu().numpy(), report.cpu().numpy(), status.cpu().numpy()
    return (y, report, status) if return_report else y


def mlpg_gv(mean_frames, variance_frames, windows, gv_mean, gv_var, n_iter=100, step=None, init="scaled", omega_scale=1.0):
    """``mlpg`` followed by the ascent on the likelihood with the gv term, ``(T, D) -> (T, static_dim)``: see ``mlpg_gv_batch``.
    Arguments and result as ``mlpg`` (numpy, the dtype of ``mean_frames``; per-frame ``(T, D)`` or global ``(D,)`` variances)."""
    mean_frames = np.asarray(mean_frames)
    variance_frames = np.asarray(variance_frames)
    dtype = mean_frames.dtype
    T, D = mean_frames.shape
    if not (variance_frames.ndim == 1 and variance_frames.shape[0] == D):
        assert mean_frames.shape == variance_frames.shape
        variance_frames = variance_frames[None]
    y = mlpg_gv_batch(mean_frames[None], variance_frames, windows, gv_mean, gv_var, None, n_iter, step, init, omega_scale)
    return y[0].astype(dtype, copy=False)


# ---- the covariance of the trajectory distribution N(c; cbar, R^-1) ------------------------------------------------
def raise_on_trajectory_status(status):
    """The reference's LinAlgError for the first (utterance, dim) whose R has a non-positive pivot; the frame is the minor."""
    st = status.cpu().numpy() if hasattr(status, "cpu") else np.asarray(status)
    bad = np.argwhere(st != 0)
    if len(bad):
        b, d = (int(i) for i in bad[0])
        raise np.linalg.LinAlgError("%d-th leading minor not positive definite (utterance %d, dim %d, frame %d)"
                                    % (int(st[b, d]), b, d, int(st[b, d]) - 1))


def mlpg_covariance_batch(variances, windows, lengths=None, *, B=None, Tmax=None, band=True, out=None):
    """The other half of MLPG's trajectory distribution ``N(c; cbar, R^-1)`` over a zero-padded batch: the band of the covariance
    ``S = R^-1`` and ``log det R`` of every (utterance, static dim), ``R = sum_w W_w' diag(1 / var_w) W_w`` with the reference's
    edge-frame and dtype rules -- the matrix every ``mlpg`` route solves with.  One launch of ``nnmk_traj_covariance``: banded
    ``L D L'`` and Takahashi's recurrence, ``O(T Q^2)`` per system, no dense ``T x T`` matrix anywhere.

    ``variances``: ``(B, Tmax, D)``, a global ``(D,)`` or ``None`` (unit variances: one static dim), numpy or CUDA tensors,
    float32 or float64; ``(D,)`` and ``None`` are read in place, never broadcast to a copy, and take the batch shape from
    ``lengths`` / ``B`` / ``Tmax``.  Returns ``(band, logdet)``, float64, the kind of ``variances`` (numpy unless a CUDA tensor was
    given): ``band`` ``(Q + 1, B, Tmax, static_dim)`` with ``band[k, b, t] = S[t, t + k]`` -- ``band[0]`` is the posterior variance
    of the generated trajectory --, zero where ``t + k`` is at or past the utterance's length; ``logdet`` ``(B, static_dim)``.
    ``band=False``: the factorisation alone, ``(None, logdet)``.  ``out``: a float64 CUDA tensor for the band.  A system that is
    not positive definite raises ``numpy.linalg.LinAlgError`` naming the first failing (utterance, dim, frame), as ``mlpg`` does.
    Window extents of at most 1."""
    from .. import _trajectory_calls as TH
    torch = _hip.torch_mod()
    nw = _hip._nw(windows)
    is_np = not torch.is_tensor(variances)
    v = None
    if variances is None:
        dev = _hip.require_gpu(out.device if out is not None else None)
        D, dtype = nw, torch.float64
    else:
        v, _ = _as_device_batch(variances)
        v = v.contiguous() if v.dim() != 3 else v
        dev, D, dtype = v.device, v.shape[-1], v.dtype
        if v.dim() not in (1, 3):
            raise ValueError("variances must be (B, Tmax, D), (D,) or None, got %s" % (tuple(v.shape),))
    if nw < 1 or D % nw:
        raise ValueError("D = %d is not a multiple of the %d windows" % (D, nw))
    if v is not None and v.dim() == 3:
        if (B is not None and B != v.shape[0]) or (Tmax is not None and Tmax != v.shape[1]):
            raise ValueError("B and Tmax disagree with the variances' shape %s" % (tuple(v.shape),))
        B, Tmax = v.shape[:2]
    else:
        host_len = None if lengths is None else np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).reshape(-1)
        B = int(B) if B is not None else (len(host_len) if host_len is not None else 1)
        if Tmax is None:
            if host_len is None:
                raise ValueError("global or unit variances need Tmax or lengths")
            Tmax = int(host_len.max()) if len(host_len) else 0
    L = _device_lengths(lengths, dev)
    bnd, logdet, status = TH.covariance(v, windows, L, int(B), int(Tmax), D, dtype=dtype, device=dev, want_band=bool(band), band=out)
    raise_on_trajectory_status(status)
    if is_np and out is None:
        return (bnd.cpu().numpy() if bnd is not None else None), logdet.cpu().numpy()
    return bnd, logdet


def mlpg_variance(variance_frames, windows):
    """The posterior variance of the trajectory ``mlpg(mean_frames, variance_frames, windows)`` generates, ``(T, D) -> (T,
    static_dim)`` float64: ``diag(R^-1)`` (the reference has it for unit variances alone, as a dense ``T x T`` inverse).
    ``variance_frames``: ``(T, D)`` numpy, float32 or float64."""
    v = _as_float(variance_frames)
    assert v.ndim == 2
    band, _ = mlpg_covariance_batch(v[None], windows)
    return band[0, 0]


def mlpg_logdet(variance_frames, windows):
    """``log det R`` of the trajectory distribution per static dim, ``(T, D) -> (static_dim,)`` float64."""
    v = _as_float(variance_frames)
    assert v.ndim == 2
    return mlpg_covariance_batch(v[None], windows, band=False)[1][0]


# ---- draws from the trajectory distribution N(c; cbar, R^-1) and the whitening map ----------------------------------
def _trajectory_factor(means, variances, windows, lengths):
    """(means on the device, variances or None, lengths or None, factor, logdet, status, was numpy, the means' dtype) for the
    functions below; the means and variances brought to one dtype as mlpg_batch does."""
    from .. import _sample_calls as SC
    torch = _hip.torch_mod()
    m, is_np = _as_device_batch(means)
    m = m.detach()
    if m.dim() != 3:
        raise ValueError("means must be (B, Tmax, D), got %s" % (tuple(m.shape),))
    B, Tmax, D = m.shape
    out_dtype = m.dtype
    v = None
    if variances is not None:
        v = _as_device_batch(variances, m.device)[0].detach()
        if v.dim() not in (1, 3) or (v.dim() == 3 and v.shape != m.shape) or (v.dim() == 1 and v.shape[0] != D):
            raise ValueError("variances must be like the means, (D,) or None, got %s" % (tuple(v.shape),))
        m, v = _match_dtypes(m, v)
        v = v.contiguous() if v.dim() == 1 else v
    L = _device_lengths(lengths, m.device)
    fac, logdet, status = SC.factor(v, windows, L, B, Tmax, D, dtype=m.dtype, device=m.device)
    raise_on_trajectory_status(status)
    return m, v, L, fac, logdet, status, is_np, out_dtype


def mlpg_sample_batch(means, variances, windows, lengths=None, num_samples=1, *, noise=None, generator=None, cbar=None, return_logdet=False,
                      out=None):
    """Draws from MLPG's trajectory distribution ``N(c; cbar, R^-1)`` over a zero-padded batch: ``c = cbar + L^-T D^-1/2 z`` with
    ``R = L D L'`` the banded factor ``mlpg_covariance_batch`` eliminates with and ``z`` white.  Two launches (``nnmk_draw_factor``,
    ``nnmk_draw_sample``) after the mean's: ``O(T Q)`` per draw, no dense ``T x T`` factor anywhere.

    ``means`` ``(B, Tmax, D)`` and ``variances`` (like the means, a global ``(D,)`` or ``None``): numpy arrays or CUDA tensors,
    float32 or float64.  ``cbar`` ``(B, Tmax, static_dim)``: the mean trajectory, if it is at hand; otherwise ``mlpg_batch(means,
    variances, windows, lengths)`` gives it.  ``noise`` ``(num_samples, B, Tmax, static_dim)``: the white ``z``; otherwise
    ``torch.randn(..., generator=generator)`` on the device (``generator``: a CUDA ``torch.Generator``, for reproducible draws).
    Returns ``(num_samples, B, Tmax, static_dim)`` in the dtype of the means -- zero at or past an utterance's length --, numpy for
    numpy means, else a CUDA tensor (``out``, if given); with ``return_logdet`` also ``log det R`` ``(B, static_dim)`` float64.  All
    work goes on the current stream.  The draws are NOT differentiable: tensors that require a gradient are accepted and the result is
    detached.  A system that is not positive definite raises ``numpy.linalg.LinAlgError`` naming utterance, dim and frame.
    Window extents of at most 1."""
    from .. import _sample_calls as SC
    torch = _hip.torch_mod()
    K = int(num_samples)
    if K < 0:
        raise ValueError("num_samples must not be negative, got %d" % K)
    nw = _hip._nw(windows)
    if nw < 1 or np.shape(means)[-1] % nw:
        raise ValueError("D = %d is not a multiple of the %d windows" % (np.shape(means)[-1], nw))
    if noise is not None and (np.ndim(noise) != 4 or np.shape(noise)[0] != K):
        raise ValueError("noise must be (num_samples = %d, B, Tmax, static_dim), got %s" % (K, tuple(np.shape(noise))))
    m, v, L, fac, logdet, status, is_np, out_dtype = _trajectory_factor(means, variances, windows, lengths)
    B, Tmax, D = m.shape
    sd = D // nw
    if cbar is None:
        cb = mlpg_batch(m, v, windows, L)
    else:
        cb = _as_device_batch(cbar, m.device)[0].detach()
    cb = cb.to(m.dtype)
    if noise is None:
        z = torch.randn((K, B, Tmax, sd), dtype=m.dtype, device=m.device, generator=generator)
    else:
        z = _as_device_batch(noise, m.device)[0].detach().to(m.dtype)
    x = SC.sample(fac, status, L, z, cb, out=out)
    if x.dtype != out_dtype and out is None:
        x = x.to(out_dtype)
    if is_np and out is None:
        x, logdet = x.cpu().numpy(), logdet.cpu().numpy()
    return (x, logdet) if return_logdet else x


def mlpg_sample(mean_frames, variance_frames, windows, num_samples=1, *, noise=None, generator=None):
    """``num_samples`` draws from the trajectory distribution of one utterance, ``(T, D) -> (num_samples, T, static_dim)`` in the
    dtype of ``mean_frames``; ``mlpg(mean_frames, variance_frames, windows)`` is their mean.  ``variance_frames``: ``(T, D)`` or a
    global ``(D,)``; ``noise`` ``(num_samples, T, static_dim)``.  See :func:`mlpg_sample_batch`."""
    mean_frames = np.asarray(mean_frames)
    variance_frames = np.asarray(variance_frames)
    T, D = mean_frames.shape
    if not (variance_frames.ndim == 1 and variance_frames.shape[0] == D):
        assert mean_frames.shape == variance_frames.shape
        variance_frames = variance_frames[None]
    x = mlpg_sample_batch(mean_frames[None], variance_frames, windows, None, num_samples, noise=None if noise is None else np.asarray(noise)[:, None],
                          generator=generator)
    return x[:, 0].astype(mean_frames.dtype, copy=False)


def mlpg_whiten_batch(x, means, variances, windows, lengths=None, *, cbar=None):
    """The inverse of :func:`mlpg_sample_batch`: ``z = D^1/2 L' (x - cbar)``, the trajectories ``x`` ``(K, B, Tmax, static_dim)`` (or
    ``(B, Tmax, static_dim)``: one per utterance) whitened under the model.  ``1/2 sum_t z^2`` is the quadratic term of the
    trajectory likelihood.  Arguments and result as :func:`mlpg_sample_batch`; not differentiable either."""
    from .. import _sample_calls as SC
    m, v, L, fac, _, status, is_np, out_dtype = _trajectory_factor(means, variances, windows, lengths)
    xs = _as_device_batch(x, m.device)[0].detach().to(m.dtype)
    one = xs.dim() == 3
    if one:
        xs = xs[None]
    cb = mlpg_batch(m, v, windows, L) if cbar is None else _as_device_batch(cbar, m.device)[0].detach()
    z = SC.whiten(fac, status, L, xs, cb.to(m.dtype))
    z = (z[0] if one else z).to(out_dtype)
    return z.cpu().numpy() if is_np else z


# registry of MLPG matrices handed out by unit_variance_mlpg_matrix, so that
# autograd.unit_variance_mlpg(R, means) can recover (windows, T) from R and run
# the banded O(T) kernels instead of a dense (T x nw*T) product.
import collections

_UV_REGISTRY = collections.OrderedDict()
_UV_REGISTRY_MAX = 8          # matrices remembered (each is a (T, nw*T) float32 array: 3 MB at T = 500)


def _fingerprint(R):
    """Cheap content key of an MLPG matrix: shape + a fixed sample of entries."""
    T, K = R.shape
    flat = R.reshape(-1)
    n = flat.shape[0]
    idx = (np.arange(97, dtype=np.int64) * 2654435761 + 12345) % max(n, 1)
    return (int(T), int(K)) + tuple(np.asarray(flat[idx], dtype=np.float32).tolist())


def unit_variance_mlpg_matrix(windows, T):
    """MLPG matrix ``R = (sum_w W~_w^T W_w)^-1 [W~_0^T ... W~_{nw-1}^T]``, float32 ``(T, nw*T)``.

    Drop-in for ``nnmnkwii.paramgen.unit_variance_mlpg_matrix``
    (paramgen/_mlpg.py:297-373).  Column ``w*T + t`` of ``R`` is the response to
    a unit mean at window ``w``, frame ``t``: the matrix is obtained with ONE
    unit-variance MLPG launch over ``nw*T`` one-hot "dimensions" instead of a
    dense banded inverse.  The returned array is a plain ndarray; it is also
    remembered so that ``autograd.unit_variance_mlpg`` can use the banded kernels.
    """
    torch = _hip.torch_mod()
    dev = _hip.require_gpu()
    nw = len(windows)
    K = nw * T
    E = torch.zeros((T, nw, K), dtype=torch.float64, device=dev)
    t = torch.arange(T, device=dev)
    for w in range(nw):
        E[t, w, w * T + t] = 1.0
    out, status = _hip.forward(E.view(1, T, nw * K), None, windows)
    _hip.raise_on_status(status, K)
    R = out[0].to(torch.float32).cpu().numpy()
    _UV_REGISTRY[_fingerprint(R)] = (tuple((int(l), int(u), tuple(np.asarray(c, dtype=np.float64).tolist()))
                                           for l, u, c in windows), int(T), R)
    while len(_UV_REGISTRY) > _UV_REGISTRY_MAX:      # least recently registered / looked up goes first
        _UV_REGISTRY.popitem(last=False)
    return R


def lookup_unit_variance_matrix(R_np_or_fp):
    """(windows, T, R) registered for this matrix, or None."""
    key = R_np_or_fp if isinstance(R_np_or_fp, tuple) else _fingerprint(R_np_or_fp)
    hit = _UV_REGISTRY.get(key)
    if hit is not None:
        _UV_REGISTRY.move_to_end(key)
    return hit


def reshape_means(means, static_dim):
    """``(T, D) -> (T*num_windows, static_dim)``; no-op if already reshaped
    (paramgen/_mlpg.py:376-405)."""
    T, D = means.shape
    if D == static_dim:
        return means
    return means.reshape(T, -1, static_dim).transpose(1, 0, 2).reshape(-1, static_dim)
