"""Objective metrics: the reference's ``nnmnkwii.metrics`` (metrics/__init__.py:27-183) -- ``melcd``, ``mean_squared_error``,
``lf0_mean_squared_error``, ``vuv_error`` -- plus ``batch_metrics``, which evaluates several of them over one padded batch in
one call.

Routing, for all of them: numpy arrays and CPU tensors are computed on the host, in float64 from the definitions; CUDA tensors
go through ``nnmk_metrics_batch`` (include/nnmnkwii_metrics.h) -- one launch pair over the padded batch and one
copy of 2 x nterms doubles back -- and need the built library and a GPU (``HipExtensionError`` otherwise; there is no fallback
to torch expressions).  ``melcd`` on numpy arrays is the reference's arithmetic bit for bit: ``DTWAligner(dist=melcd)`` is how
the reference's own test suite customises the alignment (tests/test_preprocessing.py:496-501), and the aligner recognises this
function and evaluates the same local cost on the GPU (include/mlpg_hip.h MLPG_HIP_DIST_SCALED_L2_NP).

Where the frames counted are none -- all lengths zero, or no frame voiced on both sides -- the new functions return ``nan``; the
reference raises ``ZeroDivisionError`` there when lengths are given (and so does ``melcd`` on numpy arrays, which is unchanged).
A ``(B, T)`` input together with ``lengths`` means one feature per frame (the reference's ``mean_squared_error`` would divide by
``T`` features there).
"""
import math

import numpy as np

_logdb_const = 10.0 / np.log(10.0) * np.sqrt(2.0)   # metrics/__init__.py:5

# kinds and flag of a term (include/nnmnkwii_metrics.h)
_FRAME_L2, _SQUARED, _VOICED_SQUARED, _MISMATCH = 0, 1, 2, 3
_FLAG_EXP = 1
_NAN = float("nan")


def _melcd_numpy(X, Y, lengths=None):
    if lengths is None:
        z = X - Y
        r = (z * z).sum(-1)
        r = math.sqrt(r) if np.isscalar(r) else np.sqrt(r)
        if not np.isscalar(r):
            r = r.mean()
        return _logdb_const * float(r)
    if len(X.shape) == 2:
        X, Y = X[:, :, None], Y[:, :, None]
    s = 0.0
    T = float(np.sum(lengths))
    for x, y, length in zip(X, Y, lengths):
        x, y = x[:length], y[:length]
        z = x - y
        s += np.sqrt((z * z).sum(-1)).sum()
    return _logdb_const * float(s) / T


# ---- routing and shapes -------------------------------------------------------------------------------------------------------
def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and hasattr(a, "is_cuda")


def _on_device(*arrays):
    """True if the arrays are CUDA tensors (all of them, or none); CPU tensors and everything else count as host data."""
    cuda = [_is_tensor(a) and a.is_cuda for a in arrays]
    if any(cuda) and not all(cuda):
        raise ValueError("metrics: CUDA tensors and host arrays in one call")
    return all(cuda)


def _host(a):
    return a.detach().numpy() if _is_tensor(a) else np.asarray(a)


def _features3d(a, lengths):
    """(D,), (T, D) or (B, T, D) -- and (B, T) with lengths: one feature -- as (B, T, D)."""
    if a.ndim == 1:
        return a[None, None, :]
    if a.ndim == 2:
        return a[:, :, None] if lengths is not None else a[None]
    if a.ndim != 3:
        raise ValueError("metrics: features must be (D,), (T, D) or (B, T, D), got %d dimensions" % a.ndim)
    return a


def _track3d(a):
    """(T,), (B, T) or (B, T, 1) as (B, T, 1)."""
    if a.ndim == 1:
        return a[None, :, None]
    if a.ndim == 2:
        return a[:, :, None]
    if a.ndim != 3 or a.shape[2] != 1:
        raise ValueError("metrics: lf0 and vuv must be (T,), (B, T) or (B, T, 1), got shape %s" % (tuple(a.shape),))
    return a


def _same_shape(*arrays):
    if any(tuple(a.shape) != tuple(arrays[0].shape) for a in arrays):
        raise ValueError("metrics: the inputs must agree in shape, got %s" % ", ".join(str(tuple(a.shape)) for a in arrays))


def _host_lengths(lengths, B, Tmax):
    if lengths is None:
        return np.full(B, Tmax, dtype=np.int64)
    n = np.asarray(_host(lengths.cpu()) if _is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    if n.shape != (B,):
        raise ValueError("metrics: %d lengths for a batch of %d" % (n.size, B))
    return np.clip(n, 0, Tmax)


# ---- the two evaluators: (per-utterance or total) pairs (sum, count) of terms over (B, T, .) arrays --------------------------------
# a term here: (kind, x_col, y_col, width, x_mask_col, y_mask_col, flags, threshold or None)
def _host_pairs(x, y, lengths, terms):
    """(B, nterms, 2) float64 on the host: the definitions of include/nnmnkwii_metrics.h, utterance by utterance."""
    B, Tmax = x.shape[:2]
    out = np.zeros((B, len(terms), 2))
    with np.errstate(all="ignore"):
        for b, n in enumerate(_host_lengths(lengths, B, Tmax)):
            xb, yb = x[b, :n], y[b, :n]
            for i, (kind, xc, yc, w, xm, ym, flags, thr) in enumerate(terms):
                u, v = xb[:, xc:xc + w].astype(np.float64), yb[:, yc:yc + w].astype(np.float64)
                if kind == _MISMATCH:
                    out[b, i] = ((u != v) if thr is None else ((u > thr) != (v > thr))).sum(), n * w
                    continue
                if kind == _VOICED_SQUARED:
                    mx, my = xb[:, xm].astype(np.float64), yb[:, ym].astype(np.float64)
                    voiced = (mx + my >= 2.0) if thr is None else ((mx > thr) & (my > thr))
                    u, v = u[voiced], v[voiced]
                    if flags & _FLAG_EXP:
                        u, v = np.exp(u), np.exp(v)
                z = u - v
                e = z * z
                out[b, i] = (np.sqrt(e.sum(-1)).sum(), n) if kind == _FRAME_L2 else (e.sum(), len(u) * w)
    return out


def _device_pairs(x, y, lengths, terms, per_utt=False):
    """The same from nnmk_metrics_batch on CUDA tensors, copied back: (nterms, 2), or (B, nterms, 2) with per_utt."""
    from . import _hip, _metrics_hip as M
    dev = _hip.require_gpu(x.device if _is_tensor(x) and x.is_cuda else None)
    torch = _hip.torch_mod()
    if lengths is not None:
        if not (_is_tensor(lengths) and lengths.device == dev and lengths.dtype == torch.int32):
            lengths = torch.as_tensor(_host(lengths.cpu()) if _is_tensor(lengths) else np.asarray(lengths), dtype=torch.int32).to(dev)
        if tuple(lengths.shape) != (x.shape[0],):
            raise ValueError("metrics: %d lengths for a batch of %d" % (lengths.numel(), x.shape[0]))
    ts = [M.term(kind, xc, yc, w, xm, ym, flags, thr) for kind, xc, yc, w, xm, ym, flags, thr in terms]
    totals, per = M.metrics_batch(x, y, ts, lengths, per_utt=per_utt)
    return (per if per_utt else totals).cpu().numpy()


def _pairs(x, y, lengths, terms, per_utt=False):
    if _on_device(x, y):
        return _device_pairs(x, y, lengths, terms, per_utt)
    per = _host_pairs(_host(x), _host(y), lengths, terms)
    return per if per_utt else per.sum(0)


def _ratio(pair):
    return float(pair[0]) / float(pair[1]) if pair[1] > 0 else _NAN


# ---- the reference's four -----------------------------------------------------------------------------------------------------
def melcd(X, Y, lengths=None):
    """Mel-cepstrum distortion in dB between time-aligned sequences of shape (D,), (T, D) or (B, T, D)
    (with ``lengths`` for padded mini-batches).  Same arithmetic as the reference for numpy arrays."""
    if not (_is_tensor(X) or _is_tensor(Y)):
        return _melcd_numpy(X, Y, lengths)
    if not _on_device(X, Y):
        return _melcd_numpy(_host(X), _host(Y), None if lengths is None else _host_lengths(lengths, X.shape[0], X.shape[1]))
    _same_shape(X, Y)
    x, y = _features3d(X, lengths), _features3d(Y, lengths)
    pair = _pairs(x, y, lengths, [(_FRAME_L2, 0, 0, x.shape[2], 0, 0, 0, None)])[0]
    return _logdb_const * _ratio(pair)


def mean_squared_error(X, Y, lengths=None):
    """The reference's ``mean_squared_error``: the ROOT of the mean squared error over the live frames' elements.  Shapes (D,),
    (T, D) or (B, T, D), or (B, T) with ``lengths`` (one feature)."""
    if not (_is_tensor(X) or _is_tensor(Y)):
        X, Y = np.asarray(X), np.asarray(Y)
    _same_shape(X, Y)
    x, y = _features3d(X, lengths), _features3d(Y, lengths)
    pair = _pairs(x, y, lengths, [(_SQUARED, 0, 0, x.shape[2], 0, 0, 0, None)])[0]
    return math.sqrt(_ratio(pair))


def _f0_and_vuv(f0, vuv):
    """CUDA (B, T, 1) f0 and vuv as columns of one (B, T, .) tensor: (tensor, f0 column, vuv column).  Two columns of one dense
    (B, T, ld) tensor are addressed where they lie; anything else is stacked into a (B, T, 2) temporary."""
    from . import _hip
    torch = _hip.torch_mod()
    B, T, _ = f0.shape
    st = f0.stride()
    if (f0.dtype == vuv.dtype and f0.device == vuv.device and vuv.stride() == st and B * T > 0
            and f0.untyped_storage().data_ptr() == vuv.untyped_storage().data_ptr()):
        ld = st[1] if T > 1 else (st[0] if B > 1 else 0)
        off = vuv.storage_offset() - f0.storage_offset()
        lo = f0 if off >= 0 else vuv
        # element [b, t] of one lies `off` elements behind that of the other, closer than a row: the span between them is a view
        if abs(off) < ld and (B == 1 or T == 1 or st[0] == T * ld):
            both = lo.as_strided((B, T, abs(off) + 1), (st[0], st[1], 1))
            return (both, 0, off) if off >= 0 else (both, -off, 0)
    return torch.cat([f0, vuv.to(f0.dtype)], dim=2), 0, 1


def lf0_mean_squared_error(src_f0, src_vuv, tgt_f0, tgt_vuv, lengths=None, linear_domain=False):
    """The reference's ``lf0_mean_squared_error``: the root of the mean squared error of log-F0 over the frames both sides mark as
    voiced (``src_vuv + tgt_vuv >= 2``), of ``exp`` of them with ``linear_domain``.  Shapes (T,), (B, T) or (B, T, 1)."""
    arrays = [a if _is_tensor(a) else np.asarray(a) for a in (src_f0, src_vuv, tgt_f0, tgt_vuv)]
    _same_shape(*arrays)
    flags = _FLAG_EXP if linear_domain else 0
    if _on_device(*arrays):
        (x, xf, xv), (y, yf, yv) = (_f0_and_vuv(_track3d(f), _track3d(v)) for f, v in (arrays[:2], arrays[2:]))
    else:
        sf, sv, tf, tv = (_track3d(_host(a)).astype(np.float64) for a in arrays)
        x, y = np.concatenate([sf, sv], axis=2), np.concatenate([tf, tv], axis=2)
        xf = yf = 0
        xv = yv = 1
    pair = _pairs(x, y, lengths, [(_VOICED_SQUARED, xf, yf, 1, xv, yv, flags, None)])[0]
    return math.sqrt(_ratio(pair))


def vuv_error(src_vuv, tgt_vuv, lengths=None):
    """The reference's ``vuv_error``: the fraction of live frames whose voiced / unvoiced flags differ.  Shapes (T,), (B, T) or
    (B, T, 1)."""
    if not (_is_tensor(src_vuv) or _is_tensor(tgt_vuv)):
        src_vuv, tgt_vuv = np.asarray(src_vuv), np.asarray(tgt_vuv)
    _same_shape(src_vuv, tgt_vuv)
    pair = _pairs(_track3d(src_vuv), _track3d(tgt_vuv), lengths, [(_MISMATCH, 0, 0, 1, 0, 0, 0, None)])[0]
    return _ratio(pair)


# ---- several metrics over one batch, one call -----------------------------------------------------------------------------------
def _columns(spec, D):
    """An int or a slice with step 1 -> (first column, width)."""
    if isinstance(spec, slice):
        start, stop, step = spec.indices(D)
        if step != 1 or stop <= start:
            raise ValueError("batch_metrics: a column slice must have step 1 and at least one column, got %s" % (spec,))
        return start, stop - start
    c = int(spec)
    c = c + D if c < 0 else c
    if not 0 <= c < D:
        raise ValueError("batch_metrics: column %s outside 0 .. %d" % (spec, D - 1))
    return c, 1


def batch_metrics(X, Y, lengths, terms, per_utterance=False, vuv_threshold=None):
    """Several metrics between the columns of two padded (B, T, D) batches -- prediction X, target Y, the same columns in both --
    in ONE evaluation: on CUDA tensors one call of ``nnmk_metrics_batch``, which reads every frame once per matrix.

    ``terms``: a dict name -> spec, for example (a Merlin acoustic feature matrix)::

        {"mcd": ("melcd", slice(1, 60)), "bap": ("mse", slice(62, 65)), "lf0": ("lf0_mse", 60, 61), "vuv": ("vuv_error", 61)}

    ``("melcd", columns)``, ``("mse", columns)``, ``("vuv_error", columns)`` with an int or a slice, and ``("lf0_mse", f0 column,
    vuv column[, linear_domain])``.  At most 8 terms.  ``vuv_threshold``: a frame is voiced where the vuv column exceeds it (0.5
    for a network's continuous output), in ``lf0_mse``'s mask and in ``vuv_error``; None: the reference's rules (the flags sum to
    at least 2; the values differ).  Returns a dict name -> float over the whole batch, or with ``per_utterance`` name ->
    float64 array (B,); ``nan`` where nothing was counted.  ``lengths`` None: every frame is live."""
    if X.ndim != 3 or Y.ndim != 3 or tuple(X.shape[:2]) != tuple(Y.shape[:2]):
        raise ValueError("batch_metrics: X and Y must be (B, T, D) batches of the same B and T, got %s and %s" % (tuple(X.shape), tuple(Y.shape)))
    D = min(X.shape[2], Y.shape[2])
    thr = None if vuv_threshold is None else float(vuv_threshold)
    names, descr, how = [], [], []
    for name, spec in terms.items():
        word = spec[0] if isinstance(spec, (tuple, list)) and spec else None
        if word in ("melcd", "mse", "vuv_error") and len(spec) == 2:
            c, w = _columns(spec[1], D)
            kind = {"melcd": _FRAME_L2, "mse": _SQUARED, "vuv_error": _MISMATCH}[word]
            descr.append((kind, c, c, w, 0, 0, 0, thr if word == "vuv_error" else None))
        elif word == "lf0_mse" and len(spec) in (3, 4):
            (c, _), (m, _) = _columns(int(spec[1]), D), _columns(int(spec[2]), D)
            descr.append((_VOICED_SQUARED, c, c, 1, m, m, _FLAG_EXP if len(spec) == 4 and spec[3] else 0, thr))
        else:
            raise ValueError("batch_metrics: term %r: expected ('melcd' | 'mse' | 'vuv_error', columns) or "
                             "('lf0_mse', f0 column, vuv column[, linear_domain]), got %r" % (name, spec))
        names.append(name)
        how.append(word)
    if not 1 <= len(descr) <= 8:
        raise ValueError("batch_metrics: 1 .. 8 terms, got %d" % len(descr))
    pairs = _pairs(X, Y, lengths, descr, per_utt=per_utterance)
    out = {}
    with np.errstate(all="ignore"):
        for i, (name, word) in enumerate(zip(names, how)):
            s, c = pairs[..., i, 0], pairs[..., i, 1]
            r = np.where(c > 0, s / np.where(c > 0, c, 1.0), np.nan)
            r = _logdb_const * r if word == "melcd" else (r if word == "vuv_error" else np.sqrt(r))
            out[name] = r if per_utterance else float(r)
    return out
