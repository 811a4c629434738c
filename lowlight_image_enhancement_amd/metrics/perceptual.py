"""metrics.perceptual on MI355X (reference: metrics/perceptual.py) — LPIPS between sRGB tensors.

lpips_srgb (:96-208) with the reference's validation (float32/64 only, C in {1, 3}, H and W >= 16, finite values,
`spatial` only with reduction='none'), gray replication, clamp (True -> [0, 1], a float -> [0, clamp]), the
[0,1] -> [-1,1] mapping, the model(pred, target) argument order and the negative-value RuntimeWarning, around the
MI355X LPIPS (lpips.py; `spatial=True` gives the per-pixel map [N,H,W]).  Every check that does not need the model
runs before anything moves to the device.  CPU inputs are moved to `device` (default: cuda; there is no CPU model).

_LPIPS_CACHE is the reference's module-level cache keyed (net, version, spatial, torch.device) (:21, :68-92).

Weights follow metrics.lpips_metric.LPIPSEvaluator's rule: `weights=` or $NBP_LPIPS_WEIGHTS_{ALEX,VGG}; without them a
RuntimeError unless `allow_synthetic=True` or $NBP_LPIPS_ALLOW_SYNTHETIC=1.
"""
from __future__ import annotations

import warnings
from typing import Dict, Literal, Optional, Tuple, Union

import torch
from torch import Tensor

__all__ = ["lpips_srgb"]

_Reduction = Literal["mean", "sum", "none"]
_Backbone = Literal["alex", "vgg", "squeeze"]

_LPIPS_CACHE: Dict[Tuple[str, str, bool, torch.device], torch.nn.Module] = {}


def _ensure_nchw(pred: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    """perceptual.py:24-53."""
    if not isinstance(pred, Tensor) or not isinstance(target, Tensor):
        raise TypeError("lpips_srgb expects torch.Tensor inputs.")
    if pred.shape != target.shape:
        raise ValueError(f"pred and target must share identical shape, got {tuple(pred.shape)} vs "
                         f"{tuple(target.shape)}.")
    if pred.device != target.device:
        raise ValueError("pred and target must be on the same device.")
    if pred.ndim == 3:
        pred, target = pred.unsqueeze(0), target.unsqueeze(0)
    elif pred.ndim != 4:
        raise ValueError("Inputs must have 3 (C,H,W) or 4 (N,C,H,W) dimensions; "
                         f"received tensor with shape {tuple(pred.shape)}.")
    if pred.shape[0] == 0:
        raise ValueError("Batch size must be positive.")
    if pred.dtype not in {torch.float32, torch.float64}:
        raise TypeError(f"lpips_srgb expects float32/float64 tensors, received dtype={pred.dtype}.")
    if not torch.isfinite(pred).all():
        raise ValueError("pred contains NaN or Inf values.")
    if not torch.isfinite(target).all():
        raise ValueError("target contains NaN or Inf values.")
    return pred.detach(), target.detach()


def _reduce(values: Tensor, reduction: _Reduction) -> Tensor:
    if reduction == "none":
        return values
    if reduction == "mean":
        return values.mean(dim=0, keepdim=False)
    if reduction == "sum":
        return values.sum(dim=0, keepdim=False)
    raise ValueError(f"Unsupported reduction '{reduction}'. Choose from 'mean', 'sum', 'none'.")


def _get_lpips_model(net: str, version: str, device: torch.device, spatial: bool, weights=None,
                     allow_synthetic: Optional[bool] = None) -> torch.nn.Module:
    """The cached LPIPS module of a configuration (perceptual.py:68-92); its device weights are uploaded on first use."""
    key = (net, version, spatial, device)
    if key in _LPIPS_CACHE:
        return _LPIPS_CACHE[key]
    from ..lpips import LPIPS
    from .lpips_metric import resolve_weights
    if net not in ("alex", "vgg") or version != "0.1":
        raise NotImplementedError(f"lpips_srgb on MI355X implements net 'alex' / 'vgg' at version '0.1', got "
                                  f"net={net!r}, version={version!r}")
    weights, synthetic = resolve_weights(net, weights, allow_synthetic)
    model = LPIPS(net=net, version=version, spatial=spatial, weights=weights)
    model.synthetic = synthetic
    model.eval()
    for param in model.parameters():
        param.requires_grad_(False)
    _LPIPS_CACHE[key] = model
    return model


@torch.no_grad()
def lpips_srgb(pred_srgb: Tensor, target_srgb: Tensor, *, net: _Backbone = "alex", version: str = "0.1",
               reduction: _Reduction = "mean", normalize_to_minus1_1: bool = True, clamp: Union[bool, float] = False,
               safe_gray: bool = True, spatial: bool = False, device=None, weights=None,
               allow_synthetic: Optional[bool] = None) -> Tensor:
    """LPIPS between two sRGB tensors in [0, 1] (lower is better): [N] reduced by `reduction`, or with spatial=True
    (and reduction='none') the per-pixel map [N,H,W]."""
    pred, target = _ensure_nchw(pred_srgb, target_srgb)
    batch, channels, height, width = pred.shape
    if channels not in {1, 3}:
        raise ValueError(f"lpips_srgb expects 1 or 3 channels; received C={channels}. Enable safe_gray=True to "
                         "broadcast grayscale inputs or expand channels manually.")
    if height < 16 or width < 16:
        raise ValueError("lpips_srgb requires spatial dimensions >= 16x16 to reach the deepest feature maps. "
                         f"Received H={height}, W={width}.")
    if channels == 1 and not safe_gray:
        raise ValueError("lpips_srgb received single-channel inputs while safe_gray=False. Replicate to three channels "
                         "before calling the metric or pass safe_gray=True.")
    if spatial and reduction != "none":
        raise ValueError("LPIPS spatial maps require reduction='none'.")
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"Unsupported reduction '{reduction}'. Choose from 'mean', 'sum', 'none'.")
    if device is not None:
        lpips_device = torch.device(device)
    else:
        lpips_device = pred.device if pred.is_cuda else torch.device("cuda")
    model = _get_lpips_model(net, version, lpips_device, spatial, weights, allow_synthetic)

    pred = pred.to(device=lpips_device, dtype=torch.float32)
    target = target.to(device=lpips_device, dtype=torch.float32)
    if channels == 1:
        pred, target = pred.repeat(1, 3, 1, 1), target.repeat(1, 3, 1, 1)
    if clamp:
        upper = float(clamp) if isinstance(clamp, (int, float)) else 1.0
        pred, target = pred.clamp(0.0, upper), target.clamp(0.0, upper)
    if normalize_to_minus1_1:
        pred, target = pred.mul(2.0).sub(1.0), target.mul(2.0).sub(1.0)

    outputs = model(pred.contiguous(), target.contiguous()).to(torch.float32)
    if spatial:
        if outputs.ndim == 4:
            outputs = outputs.squeeze(1)
        if torch.any(outputs < 0):
            warnings.warn("LPIPS returned negative values; ensure inputs are properly normalised. Negative responses "
                          "can occur because of the learned channel weights.", RuntimeWarning)
        return outputs
    outputs = outputs.view(outputs.shape[0])
    if torch.any(outputs < 0):
        warnings.warn("LPIPS returned negative values; ensure inputs are properly normalised. This is occasionally "
                      "observed due to learned channel weighting.", RuntimeWarning)
    return _reduce(outputs, reduction)
