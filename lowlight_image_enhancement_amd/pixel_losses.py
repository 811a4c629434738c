"""basicsr.models.losses on MI355X: the `pixel_opt` branch of ImageRestorationModel.optimize_parameters
(NAFNet_base/basicsr/models/image_restoration_model.py:57-63,264-269).

Same names, constructor arguments, call signatures and error behaviour as the reference's
basicsr/models/losses/{losses,loss_util,__init__}.py: L1Loss, MSELoss, CharbonnierLoss, PSNRLoss, the functional
l1_loss / mse_loss / charbonnier_loss(pred, target, weight=None, reduction='mean') and build_loss(opt).  Every value
and gradient is computed by the HIP kernels of csrc/pixel_loss.hip (nbp_pixel_loss, nbp_psnr_loss in include/nbp.h);
scalars and the weighted mean's denominator stay on the device.  Inputs are float32 tensors on the GPU (anything else
raises, as the other loss terms do); a gradient w.r.t. `weight` is not provided.

`fused_value_and_grad` is the training step's entry: value and d/d pred from one pass, the upstream gradient read from
device memory (NBPTrainer's `pixel_loss` term).
"""
from __future__ import annotations

import math
from copy import deepcopy
from typing import Optional

import torch
from torch import nn as nn

from . import _lib
from ._lib import call, query

_reduction_modes = ["none", "mean", "sum"]
_KIND = {"l1": 0, "mse": 1, "charbonnier": 2}
_RED = {"mean": 0, "sum": 1, "none": 2}


def _check_reduction(reduction):
    if reduction not in _reduction_modes:
        raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: {_reduction_modes}")


def _geometry(t: torch.Tensor):
    """(N, C, HW) of a contiguous tensor read as [N][C][the rest]."""
    if t.dim() >= 2:
        return t.shape[0], t.shape[1], max(1, math.prod(t.shape[2:]))
    return 1, 1, t.numel()


class _PixelLossFn(torch.autograd.Function):
    """nbp_pixel_loss.  The forward takes the value alone; the backward, where the upstream gradient exists, runs the
    fused value + gradient launch once per input that needs one (d/d target: the inputs swapped)."""

    @staticmethod
    def forward(ctx, pred, target, weight, kind, eps, red, loss_weight):
        _lib.require_cuda(pred, target, weight)
        if pred.shape != target.shape:
            raise ValueError(f"shape mismatch {tuple(pred.shape)} vs {tuple(target.shape)}")
        pred, target = pred.contiguous(), target.contiguous()
        N, C, HW = _geometry(pred)
        wc = 0
        if weight is not None:
            weight = weight.contiguous()
            wc = weight.shape[1]
        ws = (torch.empty(query("pixel_loss_workspace_doubles", pred.numel()), dtype=torch.float64, device=pred.device)
              if red != 2 else None)
        out = torch.empty_like(pred) if red == 2 else torch.empty((), device=pred.device)
        call("pixel_loss", pred, target, weight, N, C, HW, wc, kind, eps, red, loss_weight, 0, None, ws, out, None)
        ctx.save_for_backward(pred, target, weight)
        ctx.args = (N, C, HW, wc, kind, eps, red, loss_weight)
        return out

    @staticmethod
    def backward(ctx, up):
        pred, target, weight = ctx.saved_tensors
        N, C, HW, wc, kind, eps, red, loss_weight = ctx.args
        up = up.float().contiguous()
        ws = (torch.empty(query("pixel_loss_workspace_doubles", pred.numel()), dtype=torch.float64, device=pred.device)
              if red != 2 else None)
        scratch = torch.empty_like(pred) if red == 2 else torch.empty((), device=pred.device)
        gp = gt = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty_like(pred)
            call("pixel_loss", pred, target, weight, N, C, HW, wc, kind, eps, red, loss_weight, 1, up, ws, scratch, gp)
        if ctx.needs_input_grad[1]:
            gt = torch.empty_like(target)
            call("pixel_loss", target, pred, weight, N, C, HW, wc, kind, eps, red, loss_weight, 1, up, ws, scratch, gt)
        return gp, gt, None, None, None, None, None


def _weighted(kind: str, pred, target, weight, reduction, eps=0.0, loss_weight=1.0):
    """loss_util.weighted_loss / weight_reduce_loss around one elementwise kind."""
    _check_reduction(reduction)
    red = _RED[reduction]
    if weight is None:
        return _PixelLossFn.apply(pred, target, None, _KIND[kind], float(eps), red, float(loss_weight))
    assert weight.dim() == pred.dim()
    assert weight.size(1) == 1 or weight.size(1) == pred.size(1)
    if weight.requires_grad:
        raise NotImplementedError("pixel losses: a gradient with respect to `weight` is not implemented")
    direct = tuple(weight.shape) in (tuple(pred.shape), (pred.shape[0], 1) + tuple(pred.shape[2:]))
    if direct:
        return _PixelLossFn.apply(pred, target, weight, _KIND[kind], float(eps), red, float(loss_weight))
    # broadcastable, but neither [N,C,...] nor [N,1,...]: the kernel gets the materialised weight; the 'mean'
    # denominator is the reference's, taken from the weight as it was given (a device scalar: no host read)
    _lib.require_cuda(weight)
    full = weight.expand_as(pred).contiguous()
    if red != 0:
        return _PixelLossFn.apply(pred, target, full, _KIND[kind], float(eps), red, float(loss_weight))
    denom = weight.sum() if weight.size(1) > 1 else weight.sum() * pred.size(1)
    return _PixelLossFn.apply(pred, target, full, _KIND[kind], float(eps), 1, float(loss_weight)) / denom


def l1_loss(pred, target, weight=None, reduction="mean"):
    return _weighted("l1", pred, target, weight, reduction)


def mse_loss(pred, target, weight=None, reduction="mean"):
    return _weighted("mse", pred, target, weight, reduction)


def charbonnier_loss(pred, target, weight=None, reduction="mean", eps=1e-12):
    return _weighted("charbonnier", pred, target, weight, reduction, eps=eps)


class _PixelLoss(nn.Module):
    kind = ""

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        _check_reduction(reduction)
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.eps = 0.0

    def forward(self, pred, target, weight=None, **kwargs):
        """pred, target: (N, C, H, W); weight (optional): (N, C, H, W) or (N, 1, H, W) element-wise weights."""
        return _weighted(self.kind, pred, target, weight, self.reduction, eps=self.eps, loss_weight=self.loss_weight)


class L1Loss(_PixelLoss):
    """L1 (mean absolute error) loss, losses.py:34-62."""
    kind = "l1"


class MSELoss(_PixelLoss):
    """MSE (L2) loss, losses.py:64-92."""
    kind = "mse"


class CharbonnierLoss(_PixelLoss):
    """Robust Charbonnier loss sqrt(d^2 + eps), losses.py:95-110."""
    kind = "charbonnier"

    def __init__(self, loss_weight=1.0, reduction="mean", eps=1e-12):
        super().__init__(loss_weight, reduction)
        self.eps = eps


class _PSNRLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, toY, loss_weight):
        _lib.require_cuda(pred, target)
        if pred.shape != target.shape:
            raise ValueError(f"shape mismatch {tuple(pred.shape)} vs {tuple(target.shape)}")
        pred, target = pred.contiguous(), target.contiguous()
        N, C, H, W = pred.shape
        ws = torch.empty(query("psnr_loss_workspace_doubles", N, C, H * W, toY), dtype=torch.float64, device=pred.device)
        loss = torch.empty((), device=pred.device)
        call("psnr_loss", pred, target, N, C, H * W, toY, loss_weight, 0, None, ws, loss, None)
        ctx.save_for_backward(pred, target)
        ctx.args = (toY, loss_weight)
        return loss

    @staticmethod
    def backward(ctx, up):
        pred, target = ctx.saved_tensors
        toY, loss_weight = ctx.args
        N, C, H, W = pred.shape
        up = up.float().contiguous()
        ws = torch.empty(query("psnr_loss_workspace_doubles", N, C, H * W, toY), dtype=torch.float64, device=pred.device)
        scratch = torch.empty((), device=pred.device)
        gp = gt = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty_like(pred)
            call("psnr_loss", pred, target, N, C, H * W, toY, loss_weight, 1, up, ws, scratch, gp)
        if ctx.needs_input_grad[1]:
            gt = torch.empty_like(target)
            call("psnr_loss", target, pred, N, C, H * W, toY, loss_weight, 1, up, ws, scratch, gt)
        return gp, gt, None, None


class PSNRLoss(nn.Module):
    """loss_weight * 10/ln 10 * mean over images of log(mse_n + 1e-8), losses.py:112-138; toY: on the BT.601 luma."""

    def __init__(self, loss_weight=1.0, reduction="mean", toY=False):
        super().__init__()
        assert reduction == "mean"
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.scale = 10 / math.log(10)
        self.toY = toY
        self.coef = torch.tensor([65.481, 128.553, 24.966]).reshape(1, 3, 1, 1)

    def forward(self, pred, target):
        assert len(pred.size()) == 4
        if self.toY and pred.size(1) != 3:
            raise ValueError(f"PSNRLoss(toY=True) expects three channels, got {pred.size(1)}")
        return _PSNRLossFn.apply(pred, target, int(bool(self.toY)), float(self.loss_weight))


def fused_value_and_grad(loss: nn.Module, pred, target, up, value, grad):
    """value[0] = loss(pred, target) and grad = up[0] * d loss / d pred in one call of the loss's kernel entry: the
    elementwise kinds read pred and target once for both; PSNRLoss runs its two passes and the finish kernel.  `up`,
    `value` (one float each) and `grad` (like pred) are device tensors the caller owns; pred and target contiguous."""
    if isinstance(loss, PSNRLoss):
        N, C, H, W = pred.shape
        toY = int(bool(loss.toY))
        ws = torch.empty(query("psnr_loss_workspace_doubles", N, C, H * W, toY), dtype=torch.float64, device=pred.device)
        call("psnr_loss", pred, target, N, C, H * W, toY, float(loss.loss_weight), 1, up, ws, value, grad)
        return
    if not isinstance(loss, _PixelLoss) or loss.reduction == "none":
        raise ValueError("fused_value_and_grad: an L1Loss / MSELoss / CharbonnierLoss with reduction 'mean' or 'sum', "
                         "or a PSNRLoss")
    N, C, HW = _geometry(pred)
    ws = torch.empty(query("pixel_loss_workspace_doubles", pred.numel()), dtype=torch.float64, device=pred.device)
    call("pixel_loss", pred, target, None, N, C, HW, 0, _KIND[loss.kind], float(loss.eps), _RED[loss.reduction],
         float(loss.loss_weight), 1, up, ws, value, grad)


_LOSSES = {"L1Loss": L1Loss, "MSELoss": MSELoss, "CharbonnierLoss": CharbonnierLoss, "PSNRLoss": PSNRLoss}


def __getattr__(name):  # HybridLossPlus, as the reference's package exports it (imported on first use)
    if name == "HybridLossPlus":
        from .NewBP_model.losses import HybridLossPlus
        return HybridLossPlus
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def build_loss(opt):
    """Create a loss instance from a configuration dict (basicsr/models/losses/__init__.py:19-37)."""
    if opt is None:
        raise ValueError("Loss config must not be None.")
    opt_copy = deepcopy(opt)
    loss_type = opt_copy.pop("type", None)
    if not loss_type:
        raise KeyError('Loss config must contain the key "type".')
    loss_cls: Optional[type] = _LOSSES.get(loss_type)
    if loss_cls is None and loss_type == "HybridLossPlus":
        loss_cls = __getattr__("HybridLossPlus")
    if loss_cls is None:
        raise KeyError(f"Loss type {loss_type} is not registered.")
    return loss_cls(**opt_copy)


__all__ = ["L1Loss", "MSELoss", "PSNRLoss", "CharbonnierLoss", "build_loss", "HybridLossPlus", "l1_loss", "mse_loss",
           "charbonnier_loss", "fused_value_and_grad"]
