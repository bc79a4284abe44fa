"""The waveform side of preprocessing on the device: mu-law companding and quantisation, pre- and de-emphasis (mirror of
nnmnkwii/preprocessing/generic.py:56-226; csrc/wave_codec.hip; tools/wave_model.py is the specification).

    C = wave_encode_batch(X, lengths, coef=0.97, mu=256, dtype=torch.uint8)      # crops -> classes, one launch
    W = wave_decode_batch(C, lengths, mu=256, coef=0.97)                         # generated classes -> waveforms, one launch

The six functions of the reference keep their signatures; each is one launch."""
import numpy as np

from .. import _hip, _wave_hip
from .generic import _device_lengths

_tables = {}


def inv_mulaw_table(mu=256):
    """``inv_mulaw_quantize(arange(mu + 1), mu)`` by the reference's literal expression, evaluated with numpy: float32
    ``(mu + 1)``.  The device looks classes up in it, so the result is the reference's bit for bit."""
    y = np.arange(int(mu) + 1).astype(np.float32)
    y = 2 * y / mu - 1
    return np.asarray(np.sign(y) * (1.0 / mu) * ((1.0 + mu) ** np.abs(y) - 1.0), dtype=np.float32)


def _device_table(mu, dev):
    key = (mu, str(dev))
    if key not in _tables:
        _tables[key] = _hip.torch_mod().from_numpy(inv_mulaw_table(mu)).to(dev)
    return _tables[key]


def _mu(mu, who):
    if isinstance(mu, bool) or not isinstance(mu, (int, float, np.integer, np.floating)) or mu != int(mu) or mu < 1 or mu > 2 ** 30:
        raise ValueError("%s: mu must be an integer of at least 1, got %r" % (who, mu))
    return int(mu)


def _class_dtype(dtype, mu, who):
    """(torch dtype, numpy dtype) of a class output; ValueError for anything but uint8 / int16 / int32 / int64 or too narrow."""
    torch = _hip.torch_mod()
    pairs = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
    if dtype is None:
        dtype = torch.int64
    if not isinstance(dtype, torch.dtype):
        try:
            dtype = next(t for t, n in pairs.items() if np.dtype(n) == np.dtype(dtype))
        except (StopIteration, TypeError):
            raise ValueError("%s: classes are uint8, int16, int32 or int64, got %r" % (who, dtype))
    if dtype not in pairs:
        raise ValueError("%s: classes are uint8, int16, int32 or int64, got %r" % (who, dtype))
    if (dtype == torch.uint8 and mu > 255) or (dtype == torch.int16 and mu > 32767):
        raise ValueError("%s: mu = %d does not fit %s classes" % (who, mu, dtype))
    return dtype


def _float_dtype(dtype, who):
    torch = _hip.torch_mod()
    if not isinstance(dtype, torch.dtype):
        try:
            dtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)]
        except (KeyError, TypeError):
            raise ValueError("%s: float32 or float64, got %r" % (who, dtype))
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: float32 or float64, got %r" % (who, dtype))
    return dtype


def _is_float(x):
    torch = _hip.torch_mod()
    return x.dtype in (torch.float32, torch.float64) if torch.is_tensor(x) else x.dtype in (np.float32, np.float64)


def _is_int(x):
    torch = _hip.torch_mod()
    if torch.is_tensor(x):
        return x.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
    return x.dtype.kind in "iu"


def _check_lengths(lengths, B, who):
    torch = _hip.torch_mod()
    if lengths is None:
        return
    if torch.is_tensor(lengths):
        bad = lengths.dtype not in (torch.int32, torch.int64) or tuple(lengths.shape) != (B,)
    else:
        lengths = np.asarray(lengths)
        bad = lengths.dtype.kind not in "iu" or lengths.shape != (B,)
    if bad:
        raise ValueError("%s: lengths must hold one integer per utterance (B = %d)" % (who, B))


def _batch_in(X, who, floats):
    """X as given (a tensor) or as a numpy array, checked: (B, Lmax) of a float (or class) dtype."""
    torch = _hip.torch_mod()
    if not torch.is_tensor(X):
        X = np.asarray(X)
    nd = X.dim() if torch.is_tensor(X) else X.ndim
    if nd != 2:
        raise ValueError("%s: needs a (B, Lmax) batch, got %d dimensions" % (who, nd))
    if floats and not _is_float(X):
        if _is_int(X):
            raise TypeError("%s: integer waveforms are not accepted (the reference truncates coef to an integer there): "
                            "convert to float32 or float64 first" % who)
        raise TypeError("%s: float32 or float64 waveforms only, got %s" % (who, X.dtype))
    return X


def _check_out(out, X, who, kinds):
    torch = _hip.torch_mod()
    if out is None:
        return
    if not (torch.is_tensor(out) and tuple(out.shape) == tuple(X.shape) and out.dtype in kinds):
        raise ValueError("%s: out must be a CUDA tensor of X's shape %s and one of %s" % (who, tuple(X.shape), ", ".join(str(k) for k in kinds)))
    if not (torch.is_tensor(X) and X.is_cuda):
        raise ValueError("%s: out= is for CUDA tensors" % who)
    if not (out.is_cuda and out.device == X.device):
        raise ValueError("%s: out must be on X's device" % who)


def wave_encode_batch(X, lengths=None, coef=None, mu=256, quantize=True, out=None, dtype=None):
    """Waveforms -> [pre-emphasis] -> [mu-law] -> [classes] over a padded batch, in one launch.

    ``X``: ``(B, Lmax)`` float32 / float64, numpy (numpy out) or a CUDA tensor (a tensor out, no synchronisation); a row slice of
    a wider tensor is fine.  ``lengths``: one integer per utterance, clamped to ``[0, Lmax]`` (None: ``Lmax`` each); samples at or
    past them are not read and come out as 0, or as the class of silence ``mu // 2``.  ``coef``: the pre-emphasis coefficient, or
    None for none; the filter runs in ``X``'s dtype and equals the reference's bit for bit.  ``mu``: None for no mu-law (then only
    pre-emphasis), else the companding runs in float64 on the filtered value; ``quantize=True`` gives classes (``dtype``: uint8,
    int16, int32 or int64, default int64), ``quantize=False`` the companded floats (``dtype``: float32 / float64, default
    ``X``'s).  ``out`` (tensors only): where the result goes; it may be ``X`` without pre-emphasis when the element sizes match.
    Integer waveforms raise ``TypeError``; other argument errors are ``ValueError``s, all raised before any device work.  There is
    no host fallback: without the extension or a GPU the call raises ``HipExtensionError``."""
    torch = _hip.torch_mod()
    who = "wave_encode_batch"
    X = _batch_in(X, who, True)
    if mu is None:
        stage, mu_i = _wave_hip.PLAIN, 1
    else:
        mu_i = _mu(mu, who)
        stage = _wave_hip.QUANTIZE if quantize else _wave_hip.MULAW
    if coef is not None:
        coef = float(coef)
        if coef != coef:
            raise ValueError("%s: coef is NaN" % who)
    _check_lengths(lengths, X.shape[0], who)
    in_dt = X.dtype if torch.is_tensor(X) else _float_dtype(X.dtype, who)
    if out is not None and dtype is None:
        dtype = out.dtype if torch.is_tensor(out) else None
    if stage == _wave_hip.QUANTIZE:
        out_dt = _class_dtype(dtype, mu_i, who)
        _check_out(out, X, who, (torch.uint8, torch.int16, torch.int32, torch.int64))
    else:
        out_dt = in_dt if dtype is None else _float_dtype(dtype, who)
        _check_out(out, X, who, (torch.float32, torch.float64))
    if out is not None and out.dtype != out_dt:
        raise ValueError("%s: out is %s, dtype asks for %s" % (who, out.dtype, out_dt))
    if not torch.is_tensor(X) or not X.is_cuda:
        dev = _hip.require_gpu()
        xt = (X if torch.is_tensor(X) else torch.from_numpy(np.ascontiguousarray(X))).to(dev)
        res = wave_encode_batch(xt, lengths, coef, mu, quantize, None, out_dt).cpu()
        return res if torch.is_tensor(X) else res.numpy()
    dev = _hip.require_gpu(X.device)
    if out is None:
        out = torch.empty(X.shape, dtype=out_dt, device=dev)
    x2 = X if (X.shape[1] <= 1 or X.stride(1) == 1) else X.contiguous()
    _wave_hip.encode(x2, _device_lengths(lengths, X.shape[0], dev, who), coef, stage, mu_i, out)
    return out


def wave_decode_batch(Y, lengths=None, mu=256, coef=None, out=None, segment=None):
    """Classes or companded floats -> [expansion] -> [de-emphasis] -> waveforms over a padded batch, in one launch.

    ``Y``: ``(B, Lmax)``, numpy (numpy out) or a CUDA tensor (a tensor out, no synchronisation).  An integer ``Y`` (uint8, int16,
    int32, int64) holds classes: the value is the reference's ``inv_mulaw_quantize``, bit for bit (float32), looked up in a table
    of ``mu + 1`` entries; classes outside ``[0, mu]`` are clamped.  A float ``Y`` holds companded values, expanded in float64
    (``mu=None``: a plain waveform, nothing to expand).  ``coef``: the de-emphasis coefficient or None; the filter is a scan in
    float64 rounded once to the output, within the bound of tools/wave_model.py of the exact recurrence (the reference runs the
    recurrence sequentially in the input's dtype; ``coef`` is rounded to that dtype here as there).  ``out`` (tensors only):
    float32 / float64; default float32 for classes, ``Y``'s dtype otherwise.  ``segment``: None or 0 lets the library split long
    utterances among workgroups, a value ``>= Lmax`` keeps one workgroup per utterance, another value is the segment length (a
    multiple of 1024; ``ValueError`` when ``coef`` does not decay fast enough for it).  Samples at or past ``lengths`` come out
    as 0."""
    torch = _hip.torch_mod()
    who = "wave_decode_batch"
    Y = _batch_in(Y, who, False)
    classes = _is_int(Y)
    if not classes and not _is_float(Y):
        raise TypeError("%s: classes (uint8, int16, int32, int64) or float32 / float64 values, got %s" % (who, Y.dtype))
    if classes or mu is not None:
        mu_i = _mu(mu, who)
        stage = _wave_hip.QUANTIZE if classes else _wave_hip.MULAW
    else:
        stage, mu_i = _wave_hip.PLAIN, 1
    _check_lengths(lengths, Y.shape[0], who)
    _check_out(out, Y, who, (torch.float32, torch.float64))
    if torch.is_tensor(Y):
        out_dt = out.dtype if out is not None else (torch.float32 if classes else Y.dtype)
    else:
        out_dt = torch.float32 if classes or Y.dtype == np.float32 else torch.float64
    segment = 0 if segment is None else int(segment)
    if coef is not None:
        y_f32 = Y.dtype == (torch.float32 if torch.is_tensor(Y) else np.float32)
        coef = float((np.float32 if classes or y_f32 else np.float64)(coef))   # the dtype the reference would filter in
        if coef != coef:
            raise ValueError("%s: coef is NaN" % who)
        _wave_hip.plan(Y.shape[1], coef, segment)                    # (ValueError for a segment that does not fit)
    if not torch.is_tensor(Y) or not Y.is_cuda:
        dev = _hip.require_gpu()
        if not torch.is_tensor(Y) and Y.dtype.kind in "iu" and Y.dtype not in (np.uint8, np.int16, np.int32, np.int64):
            Y = Y.astype(np.int64)
        yt = (Y if torch.is_tensor(Y) else torch.from_numpy(np.ascontiguousarray(Y))).to(dev)
        res = wave_decode_batch(yt, lengths, mu, coef, None, segment).cpu()
        return res if torch.is_tensor(Y) else res.numpy()
    dev = _hip.require_gpu(Y.device)
    if Y.dtype == torch.int8:
        Y = Y.to(torch.int16)
    if out is None:
        out = torch.empty(Y.shape, dtype=out_dt, device=dev)
    y2 = Y if (Y.shape[1] <= 1 or Y.stride(1) == 1) else Y.contiguous()
    table = _device_table(mu_i, dev) if classes else None
    _wave_hip.decode(y2, _device_lengths(lengths, Y.shape[0], dev, who), stage, mu_i, table, coef, segment, out)
    return out


# ---- the reference's six functions ----------------------------------------------------------------------------------------------

def _flat(x, who, floats, one_d=False):
    """(x as a (1, N) array or tensor, a function that gives a (1, N) result the shape and kind of x)."""
    torch = _hip.torch_mod()
    if torch.is_tensor(x):
        if one_d and x.dim() != 1:
            raise ValueError("%s: 1-D input only, got %d dimensions" % (who, x.dim()))
        if floats and not _is_float(x):
            if _is_int(x) and not one_d:
                x = x.to(torch.float64)
            else:
                raise TypeError("%s: integer waveforms are not accepted (the reference truncates coef to an integer there): "
                                "convert to float32 or float64 first" % who)
        shape = tuple(x.shape)
        return x.reshape(1, -1), lambda r: r.reshape(shape)
    scalar = np.isscalar(x)
    a = np.asarray(x)
    if one_d and a.ndim != 1:
        raise ValueError("%s: 1-D input only, got %d dimensions" % (who, a.ndim))
    if floats and a.dtype not in (np.float32, np.float64):
        if a.dtype.kind in "iub" and one_d:
            raise TypeError("%s: integer waveforms are not accepted (the reference truncates coef to an integer there): "
                            "convert to float32 or float64 first" % who)
        if a.dtype.kind not in "iubf":
            raise TypeError("%s: numbers only, got %s" % (who, a.dtype))
        a = a.astype(np.float64)
    shape = a.shape
    return a.reshape(1, -1), lambda r: (r.reshape(shape)[()] if scalar else r.reshape(shape))


def mulaw(x, mu=256):
    """Mu-law companding, ``sign(x) log1p(mu |x|) / log1p(mu)``.

    Drop-in for ``nnmnkwii.preprocessing.mulaw``: scalars, arrays of any shape and tensors; CUDA tensors stay on the device.
    Evaluated in float64 on the value as read and rounded once to the input's dtype (float32 in, float32 out: under numpy >= 2
    the reference returns float64 for a float32 array; integers are taken as float64).  Within 11 ulp of the numpy evaluation."""
    x2, back = _flat(x, "mulaw", True)
    return back(wave_encode_batch(x2, None, None, _mu(mu, "mulaw"), False))


def inv_mulaw(y, mu=256):
    """Inverse of mu-law companding, ``sign(y) (1 / mu) ((1 + mu)^|y| - 1)``.

    Drop-in for ``nnmnkwii.preprocessing.inv_mulaw``; evaluated in float64 and rounded once to the input's dtype (see
    :func:`mulaw` for the deviation from the reference's result dtype)."""
    y2, back = _flat(y, "inv_mulaw", True)
    return back(wave_decode_batch(y2, None, _mu(mu, "inv_mulaw"), None))


def mulaw_quantize(x, mu=256):
    """Mu-law companding and quantisation: classes in ``[0, mu]`` for ``x`` in ``[-1, 1]``, int64.

    Drop-in for ``nnmnkwii.preprocessing.mulaw_quantize``.  The class is ``(mulaw(x) + 1) / 2 * mu`` in float64, truncated; on
    16-bit audio (``k / 32768``) it equals the reference's class at every point for ``mu`` 255 and 256, and -1, +1 and 0 give
    0, ``mu`` and ``mu // 2``.  No clamp: ``|x| > 1`` leaves ``[0, mu]`` as in the reference."""
    x2, back = _flat(x, "mulaw_quantize", True)
    r = back(wave_encode_batch(x2, None, None, _mu(mu, "mulaw_quantize"), True))
    return int(r) if np.isscalar(x) else r


def inv_mulaw_quantize(y, mu=256):
    """Inverse of mu-law companding and quantisation: float32, the reference's values bit for bit.

    Drop-in for ``nnmnkwii.preprocessing.inv_mulaw_quantize``; ``y`` holds integers (``TypeError`` otherwise)."""
    torch = _hip.torch_mod()
    y2, back = _flat(y, "inv_mulaw_quantize", False)
    if not _is_int(y2):
        raise TypeError("inv_mulaw_quantize: classes are integers, got %s" % y2.dtype)
    if torch.is_tensor(y2) and y2.dtype == torch.int8:
        y2 = y2.to(torch.int16)
    return back(wave_decode_batch(y2, None, _mu(mu, "inv_mulaw_quantize"), None))


def preemphasis(x, coef=0.97):
    """Pre-emphasis, ``y[n] = x[n] - coef x[n-1]``: 1-D float32 / float64, the reference's values bit for bit
    (``scipy.signal.lfilter([1, -coef], [1], x)`` in ``x``'s dtype).  Integer input raises ``TypeError``."""
    x2, back = _flat(x, "preemphasis", True, one_d=True)
    return back(wave_encode_batch(x2, None, coef, None))


def inv_preemphasis(x, coef=0.97):
    """De-emphasis, ``y[n] = x[n] + coef y[n-1]``: 1-D float32 / float64.  A scan in float64 rounded once to ``x``'s dtype: not the
    bits of the reference's sequential recurrence in ``x``'s dtype, but within the bound of tools/wave_model.py of the exact
    values (for float32, half an ulp).  Integer input raises ``TypeError``."""
    x2, back = _flat(x, "inv_preemphasis", True, one_d=True)
    return back(wave_decode_batch(x2, None, None, coef))
