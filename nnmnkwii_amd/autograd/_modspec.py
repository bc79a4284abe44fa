"""Differentiable modulation spectrum on PyTorch-ROCm tensors.

Host-side mirror of /root/reference/nnmnkwii/autograd/_impl/modspec.py:9-72.  Forward =
``mlpg_hip_modspec``; backward = ``mlpg_hip_modspec_backward`` (forward FFT, multiply by the incoming
gradient, one-sided inverse FFT -- instead of the reference's Python loop over feature dimensions
with dense ``(n/2+1, T)`` cosine / sine tables).
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _hip
from ..preprocessing.modspec import _check_n, _norm_flag
from ._common import _lengths_on, _to_gpu


class ModSpec(Function):
    """Modulation spectrum computation ``f : (T, D) -> (N//2+1, D)``; gradient w.r.t. ``y`` only."""

    @staticmethod
    def forward(ctx, y, n, norm):
        assert y.dim() == 2
        ctx.n = _check_n(n)
        ctx.norm = norm
        ctx.save_for_backward(y)
        dev = _hip.require_gpu(y.device if y.is_cuda else None)
        # np.fft.rfft(y, n) crops a longer signal to its first n frames (autograd/_impl/modspec.py:30-35)
        ms, _ = _hip.modspec(y.detach()[:ctx.n].to(dev)[None], ctx.n, _norm_flag(norm))
        return ms[0].to(device=y.device, dtype=y.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        (y,) = ctx.saved_tensors
        T, D = y.size()
        assert grad_output.size() == torch.Size((ctx.n // 2 + 1, D))
        dev = _hip.require_gpu(y.device if y.is_cuda else None)
        Tc = min(T, ctx.n)
        g = _hip.modspec_backward(y.detach()[:Tc].to(dev)[None], grad_output.detach().to(dev)[None], ctx.n, _norm_flag(ctx.norm))
        g = g[0].to(device=y.device, dtype=y.dtype)
        if Tc < T:  # frames beyond the DFT length do not reach the spectrum: zero gradient
            g = torch.cat([g, g.new_zeros((T - Tc, D))], dim=0)
        return g, None, None


def modspec(y, n=2048, norm=None):
    """Modulation spectrum of a ``(T, D)`` tensor (autograd/_impl/modspec.py:63-72)."""
    return ModSpec.apply(y, n, norm)


def _batch_input(y, what="y"):
    if y.dim() not in (2, 3):
        raise ValueError("%s must be (B, Tmax, D) or (T, D), got %s" % (what, tuple(y.shape)))
    if y.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s must be float32 or float64, got %s" % (what, y.dtype))


class ModSpecBatch(Function):
    """Modulation spectrum of a padded minibatch, ``f : (B, Tmax, D) -> (B, N//2+1, D)``; gradient w.r.t. ``y`` only.

    What the reference's node cannot take (autograd/_impl/modspec.py:9-72: one ``(T, D)`` tensor): a ``(B, Tmax, D)`` batch --
    or ``(T, D)`` -- of float32 or float64 with per-utterance ``lengths``.  Utterance ``b`` is ``rfft(y[b, :len_b], n)``, crop at
    ``n`` included; what lies in the padding is never read, and its gradient is exactly 0.  The tensors are used in place
    (``mlpg_hip_modspec_batch`` / ``mlpg_hip_modspec_batch_backward``: float64 arithmetic on typed loads and stores); the
    output keeps the dtype and device of ``y``.  CPU tensors are staged through the current GPU.
    """

    @staticmethod
    def forward(ctx, y, n, norm, lengths=None):
        _batch_input(y)
        ctx.n, ctx.ortho = _check_n(n), _norm_flag(norm)
        dev = _hip.require_gpu(y.device if y.is_cuda else None)
        yg = _to_gpu(y, dev)
        y3 = yg if y.dim() == 3 else yg[None]
        ctx.lengths = _lengths_on(lengths, y3.shape[0], y3.shape[1], dev)
        ctx.dev = dev
        ctx.save_for_backward(y)
        ms = _hip.modspec_batch(y3, ctx.n, ctx.ortho, ctx.lengths)
        ms = ms if y.dim() == 3 else ms[0]
        return ms if ms.device == y.device else ms.to(y.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        (y,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        yg = _to_gpu(y, ctx.dev)
        go = _to_gpu(grad_output, ctx.dev).to(y.dtype)
        three = y.dim() == 3
        g = _hip.modspec_batch_backward(yg if three else yg[None], go if three else go[None], ctx.n, ctx.ortho, ctx.lengths)
        g = g if three else g[0]
        return (g if g.device == y.device else g.to(y.device)), None, None, None


def modspec_batch(y, n=2048, norm=None, lengths=None):
    """Differentiable modulation spectrum of a padded minibatch (:class:`ModSpecBatch`): ``y`` ``(B, Tmax, D)`` or ``(T, D)``,
    float32 or float64; ``lengths`` None / a sequence / an ndarray / a tensor of valid frames per utterance.  Returns
    ``(B, n//2+1, D)`` or ``(n//2+1, D)`` with the dtype and device of ``y``."""
    return ModSpecBatch.apply(y, n, norm, lengths)


class ModSpecMSELoss(Function):
    """The modulation-spectrum loss as ONE node whose forward already holds ``d loss / d y``:
    ``mean((f(MS(y)) - f(target_ms))**2)`` over the ``(B, n//2+1, D)`` elements, ``f = log(. + eps)`` or the identity.

    One launch of ``mlpg_hip_modspec_loss_step`` keeps the spectrum on the chip -- forward FFT, residual, inverse FFT -- and a
    second small one adds the workgroups' partial sums in a fixed order, so the value repeats bit for bit.  Takes the DFT lengths
    ``mlpg_hip_modspec_loss_form`` answers 1 for; :func:`modspec_mse_loss` composes the rest.
    """

    @staticmethod
    def forward(ctx, y, target_ms, n, norm, lengths, log_domain, eps):
        _batch_input(y)
        n, ortho = _check_n(n), _norm_flag(norm)
        dev = _hip.require_gpu(y.device if y.is_cuda else None)
        yg = _to_gpu(y, dev)
        tg = _to_gpu(target_ms, dev).to(y.dtype)
        if y.dim() == 2:
            yg, tg = yg[None], tg[None]
        L = _lengths_on(lengths, yg.shape[0], yg.shape[1], dev)
        loss, grad = _hip.modspec_loss_step(yg, tg, n, ortho, L, log_domain, eps)
        grad = grad if y.dim() == 3 else grad[0]
        ctx.save_for_backward(grad if grad.device == y.device else grad.to(y.device))
        return loss.to(device=y.device, dtype=y.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        g = grad * grad_loss.to(device=grad.device, dtype=grad.dtype) if ctx.needs_input_grad[0] else None
        return g, None, None, None, None, None, None


def modspec_mse_loss(y, target_ms, n=2048, norm=None, lengths=None, log_domain=True, eps=1e-10):
    """Modulation-spectrum loss of a padded minibatch: the mean over the ``(B, n//2+1, D)`` elements of
    ``(f(MS(y)) - f(target_ms))**2`` with ``f(P) = log(P + eps)`` (``log_domain``) or ``P``.

    ``y`` ``(B, Tmax, D)`` or ``(T, D)``, float32 or float64; ``target_ms`` what ``modspec_batch(target, n, norm, lengths)``
    returns (cast to ``y.dtype``); ``lengths`` as in :func:`modspec_batch`.  Returns a 0-dim tensor of ``y.dtype`` on
    ``y.device``.  A DFT length ``mlpg_hip_modspec_loss_form`` answers 1 for (a power of two up to 4096) takes the fused node
    :class:`ModSpecMSELoss`; any other length, an empty batch, or a ``target_ms`` that requires a gradient composes
    :func:`modspec_batch` with torch operations in float64 -- the same value and the same gradient.  Works in plain eager use on
    any stream; capturing it into a CUDA graph is not supported (the fused step's workspace is allocated on first use)."""
    _batch_input(y)
    nb = _check_n(n) // 2 + 1
    if tuple(target_ms.shape) != tuple(y.shape[:-2]) + (nb, y.shape[-1]):
        raise ValueError("target_ms must be %s, got %s" % (tuple(y.shape[:-2]) + (nb, y.shape[-1]), tuple(target_ms.shape)))
    if _hip.modspec_loss_form(n) == 1 and not target_ms.requires_grad and y.numel() > 0 and target_ms.numel() > 0:
        return ModSpecMSELoss.apply(y, target_ms, n, norm, lengths, bool(log_domain), float(eps))
    ms = modspec_batch(y, n, norm, lengths).to(torch.float64)
    tm = target_ms.to(device=y.device, dtype=y.dtype).to(torch.float64)
    if log_domain:
        ms, tm = torch.log(ms + eps), torch.log(tm + eps)
    return ((ms - tm) ** 2).mean().to(y.dtype)
