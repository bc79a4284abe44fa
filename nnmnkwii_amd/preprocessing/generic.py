"""Frame utilities on the DTW path (mirror of nnmnkwii/preprocessing/generic.py:291-332) and corpus normalisation
(:496-829: meanvar, meanstd, minmax, scale, inv_scale and the min/max scalers)."""
import collections
import itertools

import numpy as np

from .. import _hip


def trim_zeros_frames(x, eps=1e-7, trim="b"):
    """Remove leading and/or trailing zero frames of a ``(T, D)`` feature matrix.

    Drop-in for ``nnmnkwii.preprocessing.trim_zeros_frames``: a frame is zero when
    ``sum_d |x| < eps``; ``trim`` is ``"b"`` (trailing, the default -- the only
    mode DTWAligner uses), ``"f"`` (leading) or ``"fb"``.  Returns a view of ``x``.
    The frame scan runs in the HIP kernel ``mlpg_hip_trim_lengths``.
    """
    assert trim in {"f", "b", "fb"}
    torch = _hip.torch_mod()
    x = np.asarray(x)
    T, D = x.shape
    dev = _hip.require_gpu()
    xf = x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)
    xt = torch.from_numpy(np.ascontiguousarray(xf)).to(dev)
    back = T
    front = 0
    if "b" in trim:
        back = int(_hip.trim_lengths(xt[None].contiguous(), eps)[0].item())
    if "f" in trim:
        front = T - int(_hip.trim_lengths(torch.flip(xt, dims=[0])[None].contiguous(), eps)[0].item())
    if trim == "b":
        return x if back == T else x[: back]
    if trim == "f":
        return x[front:]
    return x[front:back] if back > front else x[:0]


def _same_window(window):
    """np.correlate(x, window, "same") as a (l, u, coeff) triple: out[t] = sum_k coeff[l+k] x[t+k]."""
    w = np.asarray(window, dtype=np.float64).ravel()
    L = len(w)
    u = (L - 1) // 2
    return (L - 1 - u, u, w)


def delta_features(x, windows):
    """Compute delta features and combine them, ``(T, D) -> (T, D * len(windows))``.

    Drop-in for ``nnmnkwii.preprocessing.delta_features`` (preprocessing/generic.py:250-288):
    ``windows`` is a list of ``(l, u, coeff)`` triples (the paramgen convention; like the
    reference only ``coeff`` is used) or of plain coefficient arrays; each output block is the
    "same"-mode correlation of every feature dimension with the window.  A ``(B, T, D)`` batch is
    accepted as well (optionally as a CUDA tensor).  Runs in ``mlpg_hip_delta_features``.
    """
    torch = _hip.torch_mod()
    assert len(windows) > 0
    if isinstance(windows[0], tuple):
        wins = [_same_window(w[2]) for w in windows]
    else:
        wins = [_same_window(w) for w in windows]
    if torch.is_tensor(x):
        xt = x if x.dim() == 3 else x[None]
        out = _hip.delta_features(xt.contiguous(), wins)
        return out if x.dim() == 3 else out[0]
    x = np.asarray(x)
    dev = _hip.require_gpu()
    xf = x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)
    if xf.shape[-2] < max(len(w[2]) for w in wins):
        raise ValueError("delta_features: windows longer than the sequence are not supported")
    xt = torch.from_numpy(np.ascontiguousarray(xf)).to(dev)
    out = _hip.delta_features(xt if xt.dim() == 3 else xt[None], wins)
    out = out.cpu().numpy().astype(x.dtype, copy=False)
    return out if x.ndim == 3 else out[0]


# ---- corpus normalisation (mirror of nnmnkwii/preprocessing/generic.py:496-829; csrc/colstats.hip) ------------
ColumnStats = collections.namedtuple("ColumnStats", ["count", "mean", "var", "min", "max", "state"])
# An iterable dataset is packed into padded batches of at most this many elements (B * Tmax * D, pad frames included): 2^24
# elements are 128 MiB of float64 on the device, and large enough that the kernel runs at its full rate.  An utterance that is
# larger on its own goes as a batch of one.
STATS_BATCH_ELEMS = 1 << 24


def _is_cuda_tensor(x):
    torch = _hip.torch_mod()
    return torch.is_tensor(x) and x.is_cuda


def _float_array(x):
    x = np.asarray(x)
    return x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)


def _device_lengths(lengths, B, dev, who):
    torch = _hip.torch_mod()
    if lengths is None:
        return None
    if not torch.is_tensor(lengths):
        lengths = torch.from_numpy(np.asarray(lengths).astype(np.int32))
    lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
    if lengths.shape != (B,):
        raise ValueError("%s: lengths must hold one value per utterance (B = %d)" % (who, B))
    return lengths


def _padded_batches(items, lengths):
    """Pack (T_i, D) arrays into zero-padded float batches of at most STATS_BATCH_ELEMS elements: yields (X, lengths)."""
    group, tmax, D = [], 0, None

    def flush():
        X = np.zeros((len(group), max(tmax, 1), D), dtype=np.result_type(*[g.dtype for g in group]))
        for b, g in enumerate(group):
            X[b, :len(g)] = g
        return X, np.array([len(g) for g in group], dtype=np.int32)

    for idx, u in enumerate(items):
        u = _float_array(u)
        if u.ndim != 2:
            raise ValueError("dataset items must be (T, D) arrays, got %d dimensions" % u.ndim)
        if lengths is not None:
            u = u[: lengths[idx]]
        if D is None:
            D = u.shape[1]
        if u.shape[1] != D:
            raise ValueError("dataset items must share their width (got %d and %d)" % (D, u.shape[1]))
        if group and (len(group) + 1) * max(tmax, len(u)) * D > STATS_BATCH_ELEMS:
            yield flush()
            group, tmax = [], 0
        group.append(u)
        tmax = max(tmax, len(u))
    if group:
        yield flush()


def _run_stats(dataset, lengths, state, who):
    """The state (5, D) on the device after the whole dataset, the dtype of its first item, and whether it was a tensor."""
    torch = _hip.torch_mod()
    if _is_cuda_tensor(dataset):
        if dataset.dim() != 3:
            raise ValueError("%s: a tensor dataset must be (B, Tmax, D), got %d dimensions" % (who, dataset.dim()))
        if dataset.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: float32 or float64 tensors only, got %s" % (who, dataset.dtype))
        dev = _hip.require_gpu(dataset.device)
        st = None if state is None else _state_on(state, dataset.shape[2], dev)
        return _hip.column_stats(dataset, _device_lengths(lengths, dataset.shape[0], dev, who), st), dataset.dtype, True
    if torch.is_tensor(dataset):
        dataset = dataset.numpy()
    dev = _hip.require_gpu()
    if isinstance(dataset, np.ndarray) and dataset.ndim == 3:
        dtype = dataset.dtype
        x = torch.from_numpy(np.ascontiguousarray(_float_array(dataset))).to(dev)
        st = None if state is None else _state_on(state, x.shape[2], dev)
        return _hip.column_stats(x, _device_lengths(lengths, x.shape[0], dev, who), st), dtype, False
    it = iter(dataset)
    try:
        first = next(it)
    except StopIteration:
        raise ValueError("%s: the dataset is empty" % who)
    dtype = np.asarray(first).dtype
    st = None
    for X, L in _padded_batches(itertools.chain([first], it), lengths):
        if st is None and state is not None:
            st = _state_on(state, X.shape[2], dev)
        st = _hip.column_stats(torch.from_numpy(X).to(dev), torch.from_numpy(L).to(dev), st, st)
    return st, dtype, False


def _state_on(state, D, dev):
    torch = _hip.torch_mod()
    if callable(state):
        state = state(D)
    if not torch.is_tensor(state):
        state = torch.from_numpy(np.ascontiguousarray(state, dtype=np.float64))
    state = state.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(state.shape) != (5, D):
        raise ValueError("column_stats: state must be (5, D) = (5, %d): count, mean, M2, min, max; got %s" % (D, tuple(state.shape)))
    return state


def _prior_state(mean_, var_, last_sample_count):
    """The reference's (mean_, var_, last_sample_count) as a function D -> (5, D) state, M2 = var_ * count (None when nothing was
    seen: the empty state)."""
    count = int(last_sample_count)
    if count <= 0:
        return None
    torch = _hip.torch_mod()
    mean_, var_ = (t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in (mean_, var_))

    def state(D):
        s = np.zeros((5, D))
        s[0] = count
        s[1] = np.broadcast_to(np.asarray(mean_, dtype=np.float64), (D,))
        s[2] = np.broadcast_to(np.asarray(var_, dtype=np.float64), (D,)) * float(count)
        s[3], s[4] = np.inf, -np.inf
        return s
    return state


def column_stats(X, lengths=None, state=None):
    """Count, mean, variance, min and max of every column over the live frames, in ONE pass on the device.

    ``X``: a ``(B, Tmax, D)`` numpy array, a CUDA tensor (used where it lies; a last-dimension slice of a wider dense tensor is
    fine) or any iterable of ``(T_i, D)`` arrays (packed into padded batches of at most ``STATS_BATCH_ELEMS`` elements and
    streamed through the state on the device).  ``lengths``: per utterance; frames past them are never read.  ``state``: the
    ``state`` of an earlier call (the statistics then cover both).  Returns ``ColumnStats(count, mean, var, min, max, state)``:
    float64, ``var = M2 / count`` (population variance); numpy arrays and an ``int`` count for numpy input, device tensors (the
    count a 0-dim tensor, nothing synchronised) for a CUDA tensor.  ``state`` is the ``(5, D)`` array count, mean, M2, min, max.
    A column that is constant over the live frames gives ``mean ==`` the constant and ``var == 0`` exactly."""
    st, _, is_tensor = _run_stats(X, lengths, state, "column_stats")
    if is_tensor:
        return ColumnStats(st[0, 0].to(_hip.torch_mod().int64), st[1], st[2] / st[0], st[3], st[4], st)
    s = st.cpu().numpy()
    with np.errstate(all="ignore"):
        return ColumnStats(int(s[0, 0]), s[1], s[2] / s[0], s[3], s[4], s)


def meanvar(dataset, lengths=None, mean_=0.0, var_=0.0, last_sample_count=0, return_last_sample_count=False):
    """Mean and variance of every column over a dataset with variable-length items.

    Drop-in for ``nnmnkwii.preprocessing.meanvar`` (preprocessing/generic.py:496-549), which makes one scikit-learn call per
    utterance on the host; here the dataset goes through ``mlpg_hip_column_stats`` (see :func:`column_stats` for what a dataset
    may be).  ``mean_``, ``var_`` and ``last_sample_count`` continue an earlier computation.  The results have the dtype of the
    dataset's first item, as in the reference; numpy arrays, or device tensors for a CUDA tensor.  ``ValueError`` if there is no
    live frame and no earlier count."""
    prior = _prior_state(mean_, var_, last_sample_count)
    st, dtype, is_tensor = _run_stats(dataset, lengths, prior, "meanvar")
    count = int(st[0, 0].item()) if st.shape[1] else 0
    if count <= 0:
        raise ValueError("meanvar: no live frame in the dataset and no earlier statistics")
    if is_tensor:
        mean, var = st[1].to(dtype), (st[2] / st[0]).to(dtype)
    else:
        s = st.cpu().numpy()
        mean, var = s[1].astype(dtype), (s[2] / s[0]).astype(dtype)
    return (mean, var, count) if return_last_sample_count else (mean, var)


def _zero_to_one(scale):
    """The reference's rule for scales (preprocessing/generic.py:7-21): a scale of exactly 0 becomes 1.  On a copy."""
    torch = _hip.torch_mod()
    if torch.is_tensor(scale):
        return torch.where(scale == 0, torch.ones_like(scale), scale)
    if np.isscalar(scale):
        return 1.0 if scale == 0.0 else scale
    scale = np.array(scale)
    scale[scale == 0.0] = 1.0
    return scale


def meanstd(dataset, lengths=None, mean_=0.0, var_=0.0, last_sample_count=0, return_last_sample_count=False):
    """Mean and standard deviation; a standard deviation of exactly 0 (a constant column) becomes 1.  Drop-in for
    ``nnmnkwii.preprocessing.meanstd`` (preprocessing/generic.py:552-602); see :func:`meanvar`."""
    ret = meanvar(dataset, lengths, mean_, var_, last_sample_count, return_last_sample_count)
    std = _zero_to_one(ret[1].sqrt() if _hip.torch_mod().is_tensor(ret[1]) else np.sqrt(ret[1]))
    return (ret[0], std) + tuple(ret[2:])


def minmax(dataset, lengths=None):
    """Min and max of every column (``np.minimum`` / ``np.maximum``: NaN propagates).  Drop-in for
    ``nnmnkwii.preprocessing.minmax`` (preprocessing/generic.py:605-636), from the same single pass as :func:`meanvar`.  The
    dtype of the dataset's first item."""
    st, dtype, is_tensor = _run_stats(dataset, lengths, None, "minmax")
    if is_tensor:
        return st[3].to(dtype), st[4].to(dtype)
    s = st.cpu().numpy()
    dtype = dtype if np.issubdtype(dtype, np.floating) else np.float64
    return s[3].astype(dtype), s[4].astype(dtype)


def _stat_dtype(v):
    """numpy dtype of a statistic for the promotion rule; None for Python scalars (they do not promote an array)."""
    torch = _hip.torch_mod()
    if torch.is_tensor(v):
        return np.dtype(str(v.dtype).replace("torch.", ""))
    if isinstance(v, (np.ndarray, np.generic)):
        return v.dtype
    return None


def _stat_on(v, D, dev):
    """A statistic as a float64 (D,) tensor on `dev` (the value it has in its own dtype, exactly)."""
    torch = _hip.torch_mod()
    if not torch.is_tensor(v):
        v = torch.from_numpy(np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (D,))))     # (a copy: writable)
    v = v.to(device=dev, dtype=torch.float64)
    return (v.expand(D) if v.dim() == 0 else v).contiguous()


def _affine(who, x, a, c, mode, lengths, out):
    """y = (x - c) / a (mode 0) or a x + c (mode 1) per column through mlpg_hip_column_affine."""
    torch = _hip.torch_mod()
    is_tensor = torch.is_tensor(x)
    if not is_tensor:
        x = np.asarray(x)
        if out is not None:
            raise ValueError("%s: out= is for CUDA tensors" % who)
    nd = x.dim() if is_tensor else x.ndim
    if nd not in (2, 3):
        raise ValueError("%s: x must be (T, D) or (B, Tmax, D), got %d dimensions" % (who, nd))
    if nd == 2 and lengths is not None:
        raise ValueError("%s: lengths go with a (B, Tmax, D) batch" % who)
    x_dt = _stat_dtype(x) if is_tensor else x.dtype
    res = np.result_type(x_dt, *[d for d in (_stat_dtype(a), _stat_dtype(c)) if d is not None])
    if res not in (np.float32, np.float64):
        res = np.dtype(np.float64)
    if is_tensor and not x.is_cuda:
        if out is not None:
            raise ValueError("%s: out= is for CUDA tensors" % who)
        return torch.from_numpy(_affine(who, x.numpy(), a, c, mode, lengths, None))
    if is_tensor:
        if x.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: float32 or float64 tensors only, got %s" % (who, x.dtype))
        dev = _hip.require_gpu(x.device)
        xt = x
    else:
        dev = _hip.require_gpu()
        xt = torch.from_numpy(np.ascontiguousarray(_float_array(x))).to(dev)
    x3 = xt if nd == 3 else xt[None]
    B, _, D = x3.shape
    o3 = None
    if out is not None:
        if not (torch.is_tensor(out) and out.is_cuda and out.shape == x.shape and out.dtype in (torch.float32, torch.float64)):
            raise ValueError("%s: out must be a float32 / float64 CUDA tensor of x's shape" % who)
        o3 = out if nd == 3 else out[None]
    y = _hip.column_affine(x3, _stat_on(a, D, dev), _stat_on(c, D, dev), mode, _device_lengths(lengths, B, dev, who), o3,
                           torch.float64 if res == np.float64 else torch.float32)
    if out is not None:
        return out
    y = y if nd == 3 else y[0]
    return y if is_tensor else y.cpu().numpy()


def scale(x, data_mean, data_std, lengths=None, out=None):
    """Mean/variance scaling ``(x - data_mean) / data_std``; a ``data_std`` of exactly 0 counts as 1 (on a copy).

    Drop-in for ``nnmnkwii.preprocessing.scale`` (preprocessing/generic.py:639-665).  ``x``: ``(T, D)`` or ``(B, Tmax, D)``,
    numpy (numpy out) or a CUDA tensor (a tensor out).  The result has numpy's promotion of the dtypes of ``x`` and the
    statistics; the arithmetic is float64, rounded once.  ``lengths`` (batches): frames past them are not read and come out as
    zeros.  ``out`` (tensors only): where the result goes; ``out=x`` scales in place."""
    return _affine("scale", x, _zero_to_one(data_std), data_mean, 0, lengths, out)


def inv_scale(x, data_mean, data_std, lengths=None, out=None):
    """Inverse of :func:`scale`: ``data_std * x + data_mean`` (preprocessing/generic.py:668-684).  Arguments as there."""
    return _affine("inv_scale", x, data_std, data_mean, 1, lengths, out)


def _minmax_factor(data_min, data_max, feature_range):
    return (feature_range[1] - feature_range[0]) / _zero_to_one(data_max - data_min)


def minmax_scale_params(data_min, data_max, feature_range=(0, 1)):
    """``(min_, scale_)`` with which min/max scaling is ``x * scale_ + min_`` (preprocessing/generic.py:695-731).  Host
    arithmetic on ``(D,)`` arrays (tensors stay tensors); a range of exactly 0 counts as 1."""
    scale_ = _minmax_factor(data_min, data_max, feature_range)
    return feature_range[0] - data_min * scale_, scale_


def _minmax_args(who, data_min, data_max, feature_range, scale_, min_):
    if (scale_ is None or min_ is None) and (data_min is None or data_max is None):
        raise ValueError("`data_min` and `data_max` or `scale_` and `min_` must be specified to perform %s" % who)
    if scale_ is None:
        scale_ = _minmax_factor(data_min, data_max, feature_range)
    if min_ is None:
        min_ = feature_range[0] - data_min * scale_
    return scale_, min_


def minmax_scale(x, data_min=None, data_max=None, feature_range=(0, 1), scale_=None, min_=None, lengths=None, out=None):
    """Min/max scaling ``x * scale_ + min_`` (preprocessing/generic.py:734-786): give ``data_min`` and ``data_max`` (and
    ``feature_range``), or ``scale_`` and ``min_`` from :func:`minmax_scale_params`; ``ValueError`` with neither.  ``x``,
    ``lengths`` and ``out`` as in :func:`scale`."""
    scale_, min_ = _minmax_args("minmax scale", data_min, data_max, feature_range, scale_, min_)
    return _affine("minmax_scale", x, scale_, min_, 1, lengths, out)


def inv_minmax_scale(x, data_min=None, data_max=None, feature_range=(0, 1), scale_=None, min_=None, lengths=None, out=None):
    """Inverse of :func:`minmax_scale`: ``(x - min_) / scale_`` (preprocessing/generic.py:789-828)."""
    scale_, min_ = _minmax_args("inverse of minmax scale", data_min, data_max, feature_range, scale_, min_)
    return _affine("inv_minmax_scale", x, scale_, min_, 0, lengths, out)
