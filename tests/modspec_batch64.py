"""TEST INFRASTRUCTURE ONLY -- float64 reference for the modulation spectrum of a padded minibatch and for the MS loss.

Written for the tests of ``autograd.modspec_batch`` / ``autograd.modspec_mse_loss``; numpy's ``rfft`` / ``irfft`` per utterance
on ``x[b, :min(len_b, n)]`` are the algorithm.  Pinned on the CPU by tests/test_modspec_batch64_cpu.py (against
oracle/modspec.py per utterance, and by central differences of its own loss); the kernels are compared with it, never the
other way round.

    ms[b]    = |rfft(x[b, :live_b], n, norm)|^2,            live_b = min(len_b, n, Tmax)
    grad[b]  = d sum(grad_ms[b] * ms[b]) / d x[b]:  C sum_{k <= n/2} g_k Re(S_k e^{+2 pi i k t / n}) for t < live_b, 0 from there on,
               C = 2 (2 / sqrt(n) with norm="ortho", on the ortho-scaled S) -- evaluated as n * irfft(H, n) with H_k = g_k S_k / 2
               at the bins irfft counts twice and g_k Re S_k at those it counts once (k = 0, and k = n/2 for even n)
    loss     = sum (f(ms) - f(target_ms))^2 / n_elems,      f = log(. + eps) | identity
    d loss / d x = grad with grad_ms = 2 (f(ms) - f(target_ms)) f'(ms) / n_elems
"""
import numpy as np


def live_frames(lengths, B, T, n):
    """Frames of every utterance that reach the transform."""
    L = np.full(B, T, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    assert L.shape == (B,)
    return np.clip(L, 0, min(T, n))


def make_batch(rng, B, T, D, lengths=None, pad=np.nan):
    """The tests' trajectories: 0.1 * cumsum(randn) + rand along time; rows at and past each length hold `pad`."""
    x = 0.1 * np.cumsum(rng.randn(B, T, D), axis=1) + rng.rand(B, T, D)
    if lengths is not None:
        for b, n_b in enumerate(lengths):
            x[b, int(n_b):] = pad
    return x


def _spectrum(xb, live, n, norm):
    return np.fft.rfft(xb[:live], n=n, axis=0, norm=norm)


def modspec(x, n, norm=None, lengths=None):
    """(B, T, D) -> (B, n//2+1, D)."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    live = live_frames(lengths, B, T, n)
    out = np.empty((B, n // 2 + 1, D))
    for b in range(B):
        s = _spectrum(x[b], live[b], n, norm)
        out[b] = s.real ** 2 + s.imag ** 2
    return out


def modspec_grad(x, grad_ms, n, norm=None, lengths=None):
    """d sum(grad_ms * modspec(x)) / d x, (B, T, D); exactly 0 at and past each utterance's live frames."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(grad_ms, dtype=np.float64)
    B, T, D = x.shape
    nb = n // 2 + 1
    assert g.shape == (B, nb, D)
    live = live_frames(lengths, B, T, n)
    C = 2.0 / np.sqrt(n) if norm == "ortho" else 2.0
    once = np.zeros(nb, dtype=bool)
    once[0] = True
    if n % 2 == 0:
        once[n // 2] = True
    out = np.zeros_like(x)
    for b in range(B):
        s = _spectrum(x[b], live[b], n, norm)
        h = g[b] * s
        h = np.where(once[:, None], h.real + 0.0j, 0.5 * h)
        out[b, :live[b]] = C * n * np.fft.irfft(h, n=n, axis=0)[:live[b]]
    return out


def _f(p, log_domain, eps):
    return np.log(p + eps) if log_domain else p


def loss(x, target_ms, n, norm=None, lengths=None, log_domain=True, eps=1e-10, n_elems=None):
    ms = modspec(x, n, norm, lengths)
    r = _f(ms, log_domain, eps) - _f(np.asarray(target_ms, dtype=np.float64), log_domain, eps)
    return float((r * r).sum() / (r.size if n_elems is None else n_elems))


def loss_and_grad(x, target_ms, n, norm=None, lengths=None, log_domain=True, eps=1e-10, n_elems=None):
    """(loss, d loss / d x)."""
    ms = modspec(x, n, norm, lengths)
    r = _f(ms, log_domain, eps) - _f(np.asarray(target_ms, dtype=np.float64), log_domain, eps)
    ne = float(r.size if n_elems is None else n_elems)
    g = 2.0 * r / ne
    if log_domain:
        g = g / (ms + eps)
    return float((r * r).sum() / ne), modspec_grad(x, g, n, norm, lengths)
