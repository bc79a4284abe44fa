"""Modulation spectrum of parameter trajectories on MI355X.

Host-side mirror of /root/reference/nnmnkwii/preprocessing/modspec.py (``modspec`` :6-53,
``modphase`` :57-58, ``inv_modspec`` :62-100, ``modspec_smoothing`` :103-167).  The reference
calls numpy's rfft / irfft along the time axis; here every feature column is one workgroup
of the LDS-resident FFT kernels behind ``include/mlpg_hip.h`` (``mlpg_hip_modspec*``), and a
``(B, T, D)`` batch is accepted wherever the reference takes ``(T, D)``.

Arithmetic is float64 on the device; results are cast to what numpy would return for the input
dtype (float32 in -> float32 / complex64 out).  Every DFT length ``n >= 2`` is taken, as numpy's
rfft / irfft take it, on one of three routes chosen by ``n`` alone (``_hip.modspec_route(n)``):

* a power of two up to 4096 (the reference's defaults and tests): the in-LDS FFT;
* any other ``n`` up to 2048: the chirp-z (Bluestein) transform on that FFT at length
  ``2^ceil(log2(2n - 1))``, the same one workgroup per utterance and pair of columns;
* everything else (no power of two above 2048, or ``n > 4096``): the direct O(n^2) transform.

For an odd ``n``, ``modspec_smoothing`` inverts at ``n - 1`` as the reference does; each of its two
legs takes the route of its own length.  There is no CPU fallback.
"""
import numpy as np

from .. import _hip


def _norm_flag(norm):
    if norm is None or norm == "backward":
        return False
    if norm == "ortho":
        return True
    raise ValueError('Invalid norm value {}; should be None, "backward" or "ortho".'.format(norm))


def _check_n(n):
    n = int(n)
    if n < 2:
        raise ValueError("the DFT length must be at least 2, got %d" % n)
    return n


def _to_dev(x):
    """numpy (T, D) / (B, T, D) or CUDA tensor -> (float64 CUDA (B, T, D), was_numpy, had_batch, real dtype)."""
    torch = _hip.torch_mod()
    if torch.is_tensor(x):
        t = x
        rdt = np.float32 if x.dtype == torch.float32 else np.float64
        is_np = False
    else:
        x = np.asarray(x)
        rdt = np.float32 if x.dtype == np.float32 else np.float64
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(_hip.require_gpu())
        is_np = True
    batched = t.dim() == 3
    if not batched:
        assert t.dim() == 2
        t = t[None]
    return t, is_np, batched, rdt


def modspec(x, n=4096, norm=None, return_phase=False):
    """Modulation spectrum: power of the n-point DFT of the trajectory along time,
    ``(T, D) -> (n//2 + 1, D)`` (and the unit phasors ``exp(1j * angle)`` if ``return_phase``)."""
    torch = _hip.torch_mod()
    n = _check_n(n)
    t, is_np, batched, rdt = _to_dev(x)
    if t.shape[1] > n:
        t = t[:, :n]                                   # numpy's rfft(x, n) crops a longer input
    ms, ph = _hip.modspec(t, n, _norm_flag(norm), want_phase=return_phase)
    if not batched:
        ms = ms[0]
        ph = ph[0] if ph is not None else None
    if is_np:
        ms = ms.cpu().numpy().astype(rdt, copy=False)
        if return_phase:
            ph = ph.cpu().numpy()
            ph = (ph[..., 0] + 1j * ph[..., 1]).astype(np.complex64 if rdt == np.float32 else np.complex128, copy=False)
    elif return_phase:
        ph = torch.view_as_complex(ph)
    return (ms, ph) if return_phase else ms


def modphase(x, n=4096, norm=None):
    return modspec(x, n, norm, return_phase=True)[1]


def inv_modspec(ms, phase, norm=None):
    """Inverse of :func:`modspec`: ``irfft(sqrt(ms) * phase)``, ``(n//2 + 1, D) -> (n, D)``."""
    torch = _hip.torch_mod()
    is_np = not torch.is_tensor(ms)
    if is_np:
        ms_h = np.asarray(ms)
        rdt = np.float32 if ms_h.dtype == np.float32 else np.float64
        dev = _hip.require_gpu()
        ms_t = torch.from_numpy(np.ascontiguousarray(ms_h, dtype=np.float64)).to(dev)
        ph_h = np.asarray(phase).astype(np.complex128, copy=False)
        ph_t = torch.from_numpy(np.ascontiguousarray(np.stack([ph_h.real, ph_h.imag], axis=-1))).to(dev)
    else:
        rdt = np.float32 if ms.dtype == torch.float32 else np.float64
        ms_t = ms
        ph_t = torch.view_as_real(phase.to(torch.complex128).contiguous())
    batched = ms_t.dim() == 3
    if not batched:
        ms_t, ph_t = ms_t[None], ph_t[None]
    _check_n((ms_t.shape[1] - 1) * 2)
    out = _hip.inv_modspec(ms_t, ph_t, _norm_flag(norm))
    if not batched:
        out = out[0]
    return out.cpu().numpy().astype(rdt, copy=False) if is_np else out


def modspec_smoothing(x, modfs, n=4096, norm=None, cutoff=50, log_domain=True):
    """Smooth a trajectory by removing the modulation-frequency bands above ``cutoff`` Hz
    (forward DFT, band removal and inverse DFT fused in one launch; ``(T, D) -> (T, D)``)."""
    t, is_np, batched, rdt = _to_dev(x)
    T = t.shape[1]
    if cutoff is not None and cutoff > modfs // 2:          # modspec.py:145-150
        raise ValueError("Cutoff frequency {} hz must be larger than Nyquist freqeuency {}. hz".format(cutoff, modfs // 2))
    if n < T:                                               # modspec.py:151-154
        raise RuntimeError("DFT length {} must be larger than time length {}".format(n, T))
    n = _check_n(n)
    nb = n // 2 + 1
    limit_bin = nb if cutoff is None else min(int(n * cutoff / modfs) + 1, nb)   # :160-163
    if n % 2:
        # the reference inverts through inv_modspec, i.e. at length 2 (K - 1) = n - 1 for an odd n: same here,
        # composed from the three steps (the fused launch transforms back at n)
        ms, ph = _hip.modspec(t, n, _norm_flag(norm), want_phase=True)
        if limit_bin < nb:
            ms[:, limit_bin:] = 1.0 if log_domain else 0.0     # exp(0) / 0
        out = _hip.inv_modspec(ms, ph, _norm_flag(norm))[:, :T].contiguous()
    else:
        out = _hip.modspec_smoothing(t, n, limit_bin, log_domain, _norm_flag(norm))
    if not batched:
        out = out[0]
    return np.ascontiguousarray(out.cpu().numpy().astype(rdt, copy=False)) if is_np else out


def limit_bin_of(n, modfs, cutoff):
    """First removed bin of ``modspec_smoothing`` (modspec.py:145-150, :160-163); ``cutoff=None`` removes nothing."""
    nb = n // 2 + 1
    if cutoff is None:
        return nb
    if modfs is None:
        raise ValueError("a cutoff frequency needs the modulation sampling frequency modfs")
    if cutoff > modfs // 2:
        raise ValueError("Cutoff frequency {} hz must be larger than Nyquist freqeuency {}. hz".format(cutoff, modfs // 2))
    return min(int(n * cutoff / modfs) + 1, nb)


def _composed_filter(x, live, n, ortho, A, C, limit_bin, log_domain):
    """The filter at a DFT length mlpg_hip_modspec_filter does not take, from the float64 entries: modspec with phase, the table /
    removal in torch, inv_modspec.  x (B, T, D) CUDA of any float dtype, live (B) int64 CUDA; returns float64 (B, T, D)."""
    torch = _hip.torch_mod()
    B, T, D = x.shape
    rows = torch.arange(T, device=x.device)[None, :, None] < live[:, None, None]
    xz = torch.where(rows, x.to(torch.float64), torch.zeros((), dtype=torch.float64, device=x.device))   # padding never reaches the transform
    ms, ph = _hip.modspec(xz, n, ortho, want_phase=True)
    nb = n // 2 + 1
    if A is not None:
        kept = ms[:, :limit_bin]
        ms[:, :limit_bin] = torch.where(kept > 0, torch.exp(A[:limit_bin] * torch.log(kept) + C[:limit_bin]), kept)
    if limit_bin < nb:
        ms[:, limit_bin:] = 1.0 if log_domain else 0.0     # exp(0) / 0
    y = _hip.inv_modspec(ms, ph, ortho)                    # (B, 2 (nb - 1), D): n, or n - 1 for an odd n as the 2-D function
    out = torch.zeros((B, T, D), dtype=torch.float64, device=x.device)
    Ty = min(T, y.shape[1])
    out[:, :Ty] = torch.where(rows[:, :Ty], y[:, :Ty], out[:, :Ty])
    return out


def filter_batch(who, X, A, C, n, norm, lengths, limit_bin, log_domain, out):
    """What modspec_smoothing_batch and postfilters.modspec_post_filter_batch share: a padded (B, Tmax, D) batch, numpy or CUDA
    tensor, float32 / float64, through one launch of mlpg_hip_modspec_filter where it takes n, else composed in float64."""
    torch = _hip.torch_mod()
    ortho = _norm_flag(norm)
    is_tensor = torch.is_tensor(X)
    if not is_tensor:
        X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("%s: X must be (B, Tmax, D), got %d dimensions" % (who, X.ndim))
    B, T, D = (int(s) for s in X.shape)
    if n < T:                                               # modspec.py:151-154
        raise RuntimeError("DFT length {} must be larger than time length {}".format(n, T))
    nb = n // 2 + 1
    if is_tensor:
        if not X.is_cuda:
            if out is not None:
                raise ValueError("%s: out= is for CUDA tensors" % who)
            dev = _hip.require_gpu()
            return filter_batch(who, X.to(dev), A, C, n, norm, lengths, limit_bin, log_domain, None).to(X.device)
        if X.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: float32 or float64 tensors only, got %s" % (who, X.dtype))
        dev = _hip.require_gpu(X.device)
        x = X
    else:
        if out is not None:
            raise ValueError("%s: out= is for CUDA tensors" % who)
        dev = _hip.require_gpu()
        rdt = X.dtype if X.dtype in (np.float32, np.float64) else np.float64
        x = torch.from_numpy(np.ascontiguousarray(X, dtype=rdt)).to(dev)
    if lengths is not None:
        if not torch.is_tensor(lengths):
            lengths = torch.from_numpy(np.asarray(lengths).astype(np.int32))
        lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
        if lengths.shape != (B,):
            raise ValueError("%s: lengths must hold one value per utterance (B = %d)" % (who, B))
    if A is not None:
        A, C = (t.to(device=dev, dtype=torch.float64).contiguous() if torch.is_tensor(t)
                else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(dev) for t in (A, C))
        if A.shape != (nb, D) or C.shape != (nb, D):
            raise ValueError("%s: the tables must be (n/2 + 1, D) = (%d, %d), got %s and %s"
                             % (who, nb, D, tuple(A.shape), tuple(C.shape)))
    if _hip.modspec_filter_form(n):
        y = _hip.modspec_filter(x, n, A, C, limit_bin, log_domain, ortho, lengths=lengths, out=out if is_tensor else x)
    else:
        live = torch.full((B,), T, dtype=torch.int64, device=dev) if lengths is None else lengths.to(torch.int64).clamp(0, T)
        y = _composed_filter(x, live, n, ortho, A, C, limit_bin, log_domain).to(x.dtype)
        if out is not None:
            out.copy_(y)
            y = out
    return y if is_tensor else y.cpu().numpy()


def modspec_smoothing_batch(X, modfs, n=4096, norm=None, cutoff=50, log_domain=True, lengths=None, out=None):
    """``modspec_smoothing`` over a padded batch ``(B, Tmax, D)`` in one launch (``mlpg_hip_modspec_filter``).

    ``X``: a numpy array (float32 / float64 keep their dtype; others are computed as float64) or a CUDA tensor (float32 /
    float64), which may be a slice of the last dimension of a wider dense tensor.  ``lengths``: utterance b's rows at or past
    ``min(max(lengths[b], 0), Tmax)`` are never read and come out as exact zeros.  ``out`` (tensors only): where the result
    goes; ``out=X`` smooths in place.  A DFT length that is no power of two, is above 4096 or odd is composed from the float64
    calls (an odd ``n`` inverts at ``n - 1``, as the 2-D function)."""
    n = _check_n(n)
    return filter_batch("modspec_smoothing_batch", X, None, None, n, norm, lengths, limit_bin_of(n, modfs, cutoff), log_domain, out)
