"""The trajectory likelihood as a training criterion: ``- log N(c; cbar, R^-1)`` of natural trajectories under
the distribution MLPG generates from, with gradients for the means and the variances (trajectory training: Zen, Tokuda, Kitamura
2007; Hashimoto et al. 2015 for DNNs)."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _hip
from .. import _trajectory_calls as TH
from ..paramgen._mlpg import raise_on_trajectory_status
from . import _mlpg as A
from ._common import _lengths_on, _to_gpu

REDUCTIONS = ("none", "sum", "mean")


class TrajectoryNLL(Function):
    """``nll[b, d] = 1/2 (c - cbar)' R (c - cbar) - 1/2 log det R + T / 2 log 2 pi`` per (utterance, static dim) as ONE node whose
    forward already holds both gradients.  Forward is three launches: the batched MLPG forward for ``cbar``
    (``mlpg_hip_forward``, any route), ``nnmk_traj_covariance`` for ``log det R`` and -- when the variances want a gradient --
    the band of ``R^-1``, and ``nnmk_traj_nll`` for the likelihood and the gradients (a fourth, small one adds up a global
    variance's gradient over the utterances).  With nothing requiring a gradient the covariance launch runs its forward sweep
    alone.  Backward multiplies the stored gradients by the incoming one."""

    @staticmethod
    def forward(ctx, means, variances, windows, target, lengths, reduction):
        three = means.dim() == 3
        D = means.shape[-1]
        pw = _hip.cached_windows(windows)
        nw = pw[3]
        sd = D // nw
        dev = _hip.require_gpu(means.device if means.is_cuda else None)
        m = _to_gpu(means, dev)
        v = None if variances is None else _to_gpu(variances, dev)
        c = _to_gpu(target, dev).to(means.dtype)
        if not three:
            m, c = m[None], c[None]
            v = v if v is None or v.dim() == 1 else v[None]
        B, Tmax = m.shape[:2]
        L = _lengths_on(lengths, B, Tmax, dev)
        need_m = ctx.needs_input_grad[0]
        need_v = variances is not None and ctx.needs_input_grad[1]
        cbar, status = _hip.forward(m, v, pw, L, want_status=A.CHECK_STATUS)
        if A.CHECK_STATUS:
            _hip.raise_on_status(status, sd)
        band, logdet, tstatus = TH.covariance(v, pw, L, B, Tmax, D, dtype=m.dtype, device=dev, want_band=need_v)
        if A.CHECK_STATUS:
            raise_on_trajectory_status(tstatus)
        mode = _hip.VAR_UNIT if v is None else (_hip.VAR_GLOBAL if v.dim() == 1 else _hip.VAR_FRAME)
        work = None
        if need_v and mode == _hip.VAR_GLOBAL:
            work = torch.empty((B, D), dtype=torch.float64, device=dev)     # the utterances' sums: reduction "none" weighs them
        nll, gm, gv = TH.nll(m, v, pw, cbar, c, L, band, logdet, want_grad_means=need_m, want_grad_vars=need_v, workspace=work)
        if reduction == "none":
            out = nll if three else nll[0]
            scale = None
        else:
            out = nll.sum()
            scale = None
            if reduction == "mean":
                frames = (L.clamp(0, Tmax).sum().to(torch.float64) if L is not None else torch.tensor(float(B * Tmax), dtype=torch.float64, device=dev))
                scale = 1.0 / (frames * sd)
                out = out * scale
        ctx.three, ctx.nw, ctx.sd, ctx.reduction, ctx.mode = three, nw, sd, reduction, mode
        ctx.save_for_backward(*[t if t is not None else torch.empty(0, device=dev) for t in (gm, gv, work, scale)])
        ctx.have = (gm is not None, gv is not None, work is not None, scale is not None)
        return out.to(device=means.device, dtype=means.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        gm, gv, work, scale = (t if h else None for t, h in zip(ctx.saved_tensors, ctx.have))
        dev = ctx.saved_tensors[0].device
        go = grad_out.detach().to(device=dev, dtype=torch.float64)
        if scale is not None:
            go = go * scale
        res_m = res_v = None
        if ctx.reduction == "none":
            go = go if ctx.three else go[None]                      # (B, sd)
            col = go.repeat(1, ctx.nw)                               # (B, D): window-major columns
            if gm is not None and ctx.needs_input_grad[0]:
                res_m = (gm.to(torch.float64) * col[:, None, :]).to(gm.dtype)
            if gv is not None and ctx.needs_input_grad[1]:
                res_v = ((work * col).sum(dim=0) if ctx.mode == _hip.VAR_GLOBAL else gv.to(torch.float64) * col[:, None, :]).to(gv.dtype)
        else:
            if gm is not None and ctx.needs_input_grad[0]:
                res_m = (gm.to(torch.float64) * go).to(gm.dtype)
            if gv is not None and ctx.needs_input_grad[1]:
                res_v = (gv.to(torch.float64) * go).to(gv.dtype)
        if not ctx.three:
            res_m = None if res_m is None else res_m[0]
            res_v = None if res_v is None or ctx.mode == _hip.VAR_GLOBAL else res_v[0]
        return res_m, res_v, None, None, None, None


def trajectory_nll(means, variances, windows, target, lengths=None, reduction="mean"):
    """The negative log-likelihood of natural static trajectories ``target`` under MLPG's trajectory distribution
    ``N(c; cbar, R^-1)`` of (``means``, ``variances``): ``cbar`` is what ``mlpg_batch`` generates, ``R = sum_w W_w' diag(1 / var_w)
    W_w``.  ``means`` ``(B, Tmax, D)`` or ``(T, D)``, float32 or float64; ``variances`` of the same shape and dtype, a global
    ``(D,)`` or ``None`` (unit); ``target`` ``(B, Tmax, D // num_windows)`` or ``(T, ...)``; ``lengths`` as in ``mlpg_batch``.
    ``reduction``: ``"none"`` gives the ``(B, static_dim)`` likelihoods, ``"sum"`` their sum, ``"mean"`` the sum divided by
    ``sum(lengths) * static_dim``.  Both the means and the variances may require a gradient; ``target`` may not (``ValueError``).
    Window extents of at most 1.  The result keeps ``means.dtype`` and ``means.device``; the arithmetic is float64."""
    if reduction not in REDUCTIONS:
        raise ValueError("reduction must be one of %r, got %r" % (REDUCTIONS, reduction))
    if not torch.is_tensor(means) or means.dim() not in (2, 3) or means.dtype not in (torch.float32, torch.float64):
        raise ValueError("means must be a float32 / float64 (B, Tmax, D) or (T, D) tensor")
    if torch.is_tensor(target) and target.requires_grad:
        raise ValueError("trajectory_nll: a gradient for the target is out of scope (target.requires_grad is set)")
    D = means.shape[-1]
    nw = _hip.cached_windows(windows)[3]
    if nw < 1 or D % nw:
        raise ValueError("D=%d is not a multiple of the %d windows" % (D, nw))
    if not torch.is_tensor(target) or tuple(target.shape) != tuple(means.shape[:-1]) + (D // nw,):
        raise ValueError("target must be %s" % (tuple(means.shape[:-1]) + (D // nw,),))
    if variances is not None:
        if not torch.is_tensor(variances) or variances.dtype != means.dtype:
            raise TypeError("means and variances must share one dtype")
        if not (variances.shape == means.shape or (variances.dim() == 1 and variances.shape[0] == D)):
            raise ValueError("variances must have the shape of means, be (%d,) or None, got %s" % (D, tuple(variances.shape)))
    return TrajectoryNLL.apply(means, variances, windows, target, lengths, reduction)
