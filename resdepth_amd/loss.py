"""Masked, de-normalised L1 loss of the reference trainer as one fused HIP reduction
(Trainer._compute_denormalized_loss, lib/Trainer.py:87-100; denormalize_torch,
lib/data_normalization.py:29-38).

    p_i = y_pred_i * std_i + mean_i ; t_i = y_i * std_i + mean_i      (per sample, two roundings)
    both zeroed where loss_mask == 0 ; L1Loss(mean) over all elements ; * numel / sum(mask)

Data-parallel: the normaliser sum(mask) and numel are GLOBAL (all ranks), so the two partial sums are
all-reduced between the reduction and the finishing kernel.

`masked_loss` / `MaskedLoss` are the same chain for the other criteria the reference's generic expression takes -- nn.MSELoss,
nn.HuberLoss, nn.SmoothL1Loss -- plus an optional slope-consistency term on the residual's first differences, with the masked
MAE reported beside the loss (include/resdepth_hip_loss.h).  Both take an optional per-pixel weight plane
(include/resdepth_hip_wloss.h).
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops


class _MaskedL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pred, y, mask_u8, mean, std, grad_sync):
        with _lib.device_of(y_pred):
            sums = ops.masked_l1_partial(y_pred, y, mask_u8, mean, std)
            numel = y_pred.numel()
            if grad_sync is not None:
                numel = grad_sync.allreduce_loss_sums(sums, numel)
            loss, _ = ops.masked_l1_finish(y_pred, y, mask_u8, mean, std, sums, numel, want_loss=True, want_grad=False)
        ctx.save_for_backward(y_pred, y, mask_u8, mean, std, sums)
        ctx.numel = numel
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        y_pred, y, mask_u8, mean, std, sums = ctx.saved_tensors
        # gout stays on the device: the kernel reads it through a pointer (no host sync)
        g = gout.detach().to(torch.float32).contiguous()
        with _lib.device_of(y_pred):
            _, dyp = ops.masked_l1_finish(y_pred, y, mask_u8, mean, std, sums, ctx.numel, gout=g, want_loss=False,
                                          want_grad=True)
        return dyp, None, None, None, None, None


def _to_device_f32(v, dev):
    """Host values go through a pinned staging buffer and an ASYNCHRONOUS copy: a pageable `.to(device)` would block the
    host until everything already enqueued on the stream (the whole forward) has finished."""
    t = torch.as_tensor(v).flatten().to(torch.float32)
    if not t.is_cuda:
        t = t.pin_memory().to(dev, non_blocking=True)
    return t.contiguous()


def _prep(y_pred, y, loss_mask, mean, std):
    dev = y_pred.device
    if not y_pred.is_cuda:
        raise RuntimeError("resdepth_amd.masked_l1_loss runs on a HIP device only (no CPU fallback)")
    n = y_pred.shape[0]
    y = y.to(dev, torch.float32).contiguous()
    m = loss_mask.to(dev)
    if m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8) if m.dtype != torch.bool else m.view(torch.uint8)
    # mean/std arrive as CPU tensors in the reference (batch['dsm_mean'|'dsm_std'], lib/Trainer.py:174-175) and
    # are converted with .tolist() -> python floats -> fp32 scalars
    mean32, std32 = _to_device_f32(mean, dev), _to_device_f32(std, dev)
    if mean32.numel() != n or std32.numel() != n:
        raise ValueError("dsm_mean / dsm_std must hold one value per sample")
    return y_pred.contiguous(), y, m.contiguous(), mean32, std32


def masked_l1_loss(y_pred, y, loss_mask, mean, std, grad_sync=None):
    """Functional form; returns a 0-dim device tensor with autograd to y_pred."""
    yp, y, m, mean32, std32 = _prep(y_pred, y, loss_mask, mean, std)
    return _MaskedL1.apply(yp, y, m, mean32, std32, grad_sync)


class MaskedL1Loss(torch.nn.Module):
    """Module form (drop-in for the `criterion` + denormalisation pair of the reference Trainer)."""

    def __init__(self, grad_sync=None):
        super().__init__()
        self.grad_sync = grad_sync

    def forward(self, y_pred, y, loss_mask, mean, std):
        return masked_l1_loss(y_pred, y, loss_mask, mean, std, self.grad_sync)


# ---- L2 / Huber / smooth-L1 data terms and the slope-consistency term -------------------------------------------------------
KINDS = ("l1", "l2", "huber", "smooth_l1")


def _check_spec(kind, delta, slope_weight):
    """Host-side validation (no device use); returns the canonical (kind, delta, slope_weight)."""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: expected one of {', '.join(KINDS)}")
    delta, slope_weight = float(delta), float(slope_weight)
    if kind == "smooth_l1" and delta == 0.0:
        kind, delta = "l1", 1.0                  # nn.SmoothL1Loss(beta=0) is L1
    if kind in ("huber", "smooth_l1") and not (delta > 0.0 and math.isfinite(delta)):
        raise ValueError(f"delta={delta!r}: the {kind} threshold must be positive and finite")
    if not (slope_weight >= 0.0 and math.isfinite(slope_weight)):
        raise ValueError(f"slope_weight={slope_weight!r}: must be finite and >= 0")
    return kind, delta, slope_weight


def _kernel_args(kind, delta):
    """(kind code, delta, scale) of the C ABI: smooth_l1(beta) is huber(beta) / beta."""
    if kind == "smooth_l1":
        return _lib.LOSS_KINDS["huber"], delta, 1.0 / delta
    return _lib.LOSS_KINDS[kind], delta, 1.0


class _MaskedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_pred, y, mask_u8, mean, std, grad_sync, kind, delta, scale, slope_weight):
        with _lib.device_of(y_pred):
            sums = ops.masked_loss_partial(y_pred, y, mask_u8, mean, std, kind, delta, scale)
            numel = y_pred.numel()
            if grad_sync is not None:
                numel = grad_sync.allreduce_loss_sums(sums, numel)
            loss, mae, _ = ops.masked_loss_finish(y_pred, y, mask_u8, mean, std, sums, numel, kind, delta, scale, slope_weight,
                                                  want_grad=False)
        ctx.save_for_backward(y_pred, y, mask_u8, mean, std, sums)
        ctx.spec = (numel, kind, delta, scale, slope_weight)
        loss, mae = loss.reshape(()), mae.reshape(())
        ctx.mark_non_differentiable(mae)
        return loss, mae

    @staticmethod
    def backward(ctx, gout, _gmae):
        y_pred, y, mask_u8, mean, std, sums = ctx.saved_tensors
        numel, kind, delta, scale, slope_weight = ctx.spec
        g = gout.detach().to(torch.float32).contiguous()      # stays on the device: the kernel reads it through a pointer
        with _lib.device_of(y_pred):
            _, _, dyp = ops.masked_loss_finish(y_pred, y, mask_u8, mean, std, sums, numel, kind, delta, scale, slope_weight,
                                               gout=g, want_loss=False, want_mae=False)
        return (dyp,) + (None,) * 9


class _WeightedLoss(torch.autograd.Function):
    """_MaskedLoss with a per-pixel weight plane (include/resdepth_hip_wloss.h): the same eight sums go through the all-reduce."""

    @staticmethod
    def forward(ctx, y_pred, y, mask_u8, weight, mean, std, grad_sync, kind, delta, scale, slope_weight):
        with _lib.device_of(y_pred):
            sums = ops.weighted_loss_partial(y_pred, y, mask_u8, weight, mean, std, kind, delta, scale)
            numel = y_pred.numel()
            if grad_sync is not None:
                numel = grad_sync.allreduce_loss_sums(sums, numel)
            loss, mae, _ = ops.weighted_loss_finish(y_pred, y, mask_u8, weight, mean, std, sums, numel, kind, delta, scale,
                                                    slope_weight, want_grad=False)
        ctx.save_for_backward(y_pred, y, mask_u8, weight, mean, std, sums)
        ctx.spec = (numel, kind, delta, scale, slope_weight)
        loss, mae = loss.reshape(()), mae.reshape(())
        ctx.mark_non_differentiable(mae)
        return loss, mae

    @staticmethod
    def backward(ctx, gout, _gmae):
        y_pred, y, mask_u8, weight, mean, std, sums = ctx.saved_tensors
        numel, kind, delta, scale, slope_weight = ctx.spec
        g = gout.detach().to(torch.float32).contiguous()      # stays on the device: the kernel reads it through a pointer
        with _lib.device_of(y_pred):
            _, _, dyp = ops.weighted_loss_finish(y_pred, y, mask_u8, weight, mean, std, sums, numel, kind, delta, scale,
                                                 slope_weight, gout=g, want_loss=False, want_mae=False)
        return (dyp,) + (None,) * 10


def _prep_weight(weight, y_pred):
    """The weight plane as the kernels read it: fp32, contiguous, on y_pred's device, one value per pixel of [N,1,H,W]."""
    if not isinstance(weight, torch.Tensor):
        raise TypeError(f"weight: expected a tensor, got {type(weight).__name__}")
    if not weight.is_cuda:
        raise RuntimeError("resdepth_amd.masked_loss: weight must be on the HIP device (it is read by the loss kernels; no "
                           "CPU fallback)")
    if not (y_pred.dim() == 4 and y_pred.shape[1] == 1):
        raise ValueError(f"y_pred of shape {tuple(y_pred.shape)}: a weight needs a 4-D [N,1,H,W] input")
    n, _, h, w = y_pred.shape
    if tuple(weight.shape) not in ((n, 1, h, w), (n, h, w)):
        raise ValueError(f"weight of shape {tuple(weight.shape)}: expected {(n, 1, h, w)} or {(n, h, w)}")
    if weight.device != y_pred.device:
        raise RuntimeError(f"weight on {weight.device}, y_pred on {y_pred.device}")
    return weight.detach().to(torch.float32).contiguous()


def masked_loss(y_pred, y, loss_mask, mean, std, kind="l1", delta=1.0, slope_weight=0.0, grad_sync=None, return_mae=False,
                weight=None):
    """loss = sum(m rho(r)) / sum(m) + slope_weight * sum|r_a - r_b| / #pairs over the valid horizontal and vertical neighbour
    pairs, r the de-normalised residual; rho by `kind`: "l1", "l2", "huber" (delta, in metres), "smooth_l1" (beta = delta).
    Returns the 0-dim device loss with autograd to y_pred; with return_mae also the masked MAE (0-dim, no gradient).
    kind="l1" with slope_weight=0 IS masked_l1_loss (its kernels, its bits).

    weight: optional per-pixel weights, [N,1,H,W] or [N,H,W] fp32 on the device, finite and >= 0 (not tested here):
    loss = sum(m w rho(r)) / sum(m w) + slope_weight * sum(omega |r_a - r_b|) / sum(omega), omega the mean of a pair's two
    weights.  The MAE stays the plain masked MAE.  weight=None is the unweighted path in every respect."""
    kind, delta, slope_weight = _check_spec(kind, delta, slope_weight)
    if slope_weight > 0.0 and not (y_pred.dim() == 4 and y_pred.shape[1] == 1):
        raise ValueError(f"y_pred of shape {tuple(y_pred.shape)}: slope_weight > 0 needs a 4-D [N,1,H,W] input (neighbour "
                         "pairs are taken inside one single-channel image)")
    if weight is not None:
        if not y_pred.is_cuda:
            raise RuntimeError("resdepth_amd.masked_loss runs on a HIP device only (no CPU fallback)")
        wt = _prep_weight(weight, y_pred)
        yp, y, m, mean32, std32 = _prep(y_pred, y, loss_mask, mean, std)
        code, delta, scale = _kernel_args(kind, delta)
        loss, mae = _WeightedLoss.apply(yp, y, m, wt, mean32, std32, grad_sync, code, delta, scale, slope_weight)
        return (loss, mae) if return_mae else loss
    if kind == "l1" and slope_weight == 0.0:
        loss = masked_l1_loss(y_pred, y, loss_mask, mean, std, grad_sync)
        return (loss, loss.detach()) if return_mae else loss
    yp, y, m, mean32, std32 = _prep(y_pred, y, loss_mask, mean, std)
    code, delta, scale = _kernel_args(kind, delta)
    loss, mae = _MaskedLoss.apply(yp, y, m, mean32, std32, grad_sync, code, delta, scale, slope_weight)
    return (loss, mae) if return_mae else loss


class MaskedLoss(torch.nn.Module):
    """Module form of masked_loss; usable as the Trainer's `criterion` and as the `loss` of GraphedTrainStep /
    PlannedTrainStep.  After a call `last_mae` holds the masked MAE of that batch (0-dim device tensor)."""

    def __init__(self, kind="l1", delta=1.0, slope_weight=0.0, grad_sync=None):
        super().__init__()
        _check_spec(kind, delta, slope_weight)
        self.kind, self.delta, self.slope_weight = kind, float(delta), float(slope_weight)
        self.grad_sync = grad_sync
        self.last_mae = None

    def extra_repr(self):
        return f"kind={self.kind!r}, delta={self.delta}, slope_weight={self.slope_weight}"

    def forward(self, y_pred, y, loss_mask, mean, std, weight=None):
        loss, self.last_mae = masked_loss(y_pred, y, loss_mask, mean, std, self.kind, self.delta, self.slope_weight,
                                          self.grad_sync, return_mae=True, weight=weight)
        return loss


_ACCEPTED = "nn.L1Loss, nn.MSELoss, nn.HuberLoss, nn.SmoothL1Loss (each with reduction='mean') or resdepth_amd.MaskedLoss"


def criterion_spec(criterion):
    """(kind, delta, slope_weight) of a criterion object the fused loss can stand in for."""
    nn = torch.nn
    if isinstance(criterion, MaskedLoss):
        return _check_spec(criterion.kind, criterion.delta, criterion.slope_weight)
    table = ((nn.HuberLoss, "huber", "delta"), (nn.SmoothL1Loss, "smooth_l1", "beta"), (nn.MSELoss, "l2", None),
             (nn.L1Loss, "l1", None))
    for cls, kind, attr in table:
        if type(criterion) is cls:
            if criterion.reduction != "mean":
                raise NotImplementedError(f"{cls.__name__}(reduction={criterion.reduction!r}): the fused loss implements "
                                          f"reduction='mean' only; accepted: {_ACCEPTED}")
            return _check_spec(kind, getattr(criterion, attr) if attr else 1.0, 0.0)
    raise NotImplementedError(f"criterion {type(criterion).__name__} has no fused form; accepted: {_ACCEPTED}")
