"""Helpers the autograd nodes share (_mlpg.py, _modspec.py)."""
import numpy as np
import torch


def _to_gpu(t, dev):
    t = t.detach()
    if t.device != dev:
        t = t.to(dev)
    return t if t.is_contiguous() else t.contiguous()


def _lengths_on(lengths, B, T, dev):
    """``lengths`` (None, a sequence, an ndarray or a tensor) as an int32 (B,) tensor on ``dev``.  Host values are checked
    against [0, T]; a tensor already on the GPU is taken as it is (no synchronisation: the kernels clamp it)."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths):
        L = lengths.detach().reshape(-1)
        if not L.is_cuda:
            host = L.numpy()
    else:
        host = np.asarray(lengths).reshape(-1)
        L = None
    if L is None or not L.is_cuda:
        if host.shape != (B,) or not np.issubdtype(host.dtype, np.integer) or (host < 0).any() or (host > T).any():
            raise ValueError("lengths must hold %d integers in [0, %d], got %r" % (B, T, host))
        L = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32))
    elif L.shape != (B,):
        raise ValueError("lengths must have shape (%d,), got %s" % (B, tuple(L.shape)))
    if L.dtype != torch.int32:
        L = L.to(torch.int32)
    return _to_gpu(L, dev)
