"""metrics.channelwise on MI355X (reference: metrics/channelwise.py) — per-channel RGB PSNR, CPSNR and RGB SSIM.

Same names, keyword arguments, return shapes, dtypes, `meta=True` results and exception types as the reference.
rgb_psnr (:111-168) and cpsnr_rgb (:170-222) each make one call of nbp_rgb_psnr (channelwise.hip): a single pass over
both images with float64 per-plane error sums, then the three PSNRs, their mean and CPSNR in a finish launch; the batch
reduction happens in torch.  Two of the reference's semantics, kept:

  * `clamp=True` clamps to [0, 1.0], not to data_range: bool is an int, so _clamp_opt (:104-108) takes float(True);
    a float clamps to [0, clamp]; False or 0 does not clamp;
  * there is no +inf: identical inputs give 10 log10(data_range^2 / eps), 120 dB at the defaults.

rgb_ssim (:224-302) is nbp_ssim_linear's per-plane means (metrics.linear.ssim_plane_means) with the reference's
rounding: each channel's score cast to float32, the channel mean taken in float32.

channel_stats is the device-valued form for the validation pass: float64 [N, 5] with no host read (it skips the
finiteness test, which reads the device); register_channelwise_metrics() makes it available to validation.Validator.
"""
from __future__ import annotations

from typing import Dict, Literal, Tuple, TypedDict, Union

import torch
from torch import Tensor

from .. import _lib
from .._lib import call, query
from . import linear as _linear

__all__ = ["rgb_psnr", "cpsnr_rgb", "rgb_ssim", "channel_stats", "register_channelwise_metrics"]

_Reduction = Literal["mean", "sum", "none"]


class MetricMeta(TypedDict):
    domain: Literal["linear", "srgb"]
    data_range: float


class PSNRResult(TypedDict):
    R: Tensor
    G: Tensor
    B: Tensor
    mean: Tensor
    meta: MetricMeta


class CPSNRResult(TypedDict):
    cpsnr: Tensor
    meta: MetricMeta


class SSIMResult(TypedDict):
    R: Tensor
    G: Tensor
    B: Tensor
    mean: Tensor
    meta: MetricMeta


def _shape_checks(pred: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    """channelwise.py:64-86: type, shape, device, rank and channel count; [3,H,W] promoted to [1,3,H,W]."""
    if not isinstance(pred, Tensor) or not isinstance(target, Tensor):
        raise TypeError("Expected torch.Tensor inputs for rgb metrics.")
    if pred.shape != target.shape:
        raise ValueError(f"`pred` and `target` must share identical shape, got {tuple(pred.shape)} vs "
                         f"{tuple(target.shape)}.")
    if pred.device != target.device:
        raise ValueError("`pred` and `target` must reside on the same device.")
    if pred.ndim == 3:
        pred, target = pred.unsqueeze(0), target.unsqueeze(0)
    elif pred.ndim != 4:
        raise ValueError("Inputs must have 3 (C,H,W) or 4 (N,C,H,W) dimensions; "
                         f"received tensor with shape {tuple(pred.shape)}.")
    if pred.shape[1] != 3:
        raise ValueError(f"Channel-wise metrics require exactly 3 channels (RGB). Received {pred.shape[1]}.")
    return pred.detach(), target.detach()


def _ensure_rgb(pred: Tensor, target: Tensor) -> Tuple[Tensor, Tensor]:
    """channelwise.py:64-91, the finiteness test (a device read, as the reference's) included."""
    pred, target = _shape_checks(pred, target)
    if not torch.isfinite(pred).all():
        raise ValueError("`pred` contains NaN or Inf values.")
    if not torch.isfinite(target).all():
        raise ValueError("`target` contains NaN or Inf values.")
    return pred, target


def _check_reduction(reduction: str) -> None:
    if reduction not in ("none", "mean", "sum"):
        raise ValueError(f"Unsupported reduction '{reduction}'. Choose from 'mean', 'sum', 'none'.")


def _reduce(values: Tensor, reduction: _Reduction) -> Tensor:
    if reduction == "none":
        return values
    if reduction == "mean":
        return values.mean(dim=0, keepdim=False)
    if reduction == "sum":
        return values.sum(dim=0, keepdim=False)
    raise ValueError(f"Unsupported reduction '{reduction}'. Choose from 'mean', 'sum', 'none'.")


def _clamp_arg(clamp, data_range: float) -> Tuple[int, float]:
    """_clamp_opt (:104-108) as (on, upper bound): a bool is an int, so True clamps to [0, 1.0]."""
    if not clamp:
        return 0, 0.0
    return 1, float(clamp) if isinstance(clamp, (int, float)) else float(data_range)


def _check_range_eps(data_range, eps) -> None:
    if data_range <= 0:
        raise ValueError(f"`data_range` must be positive; received {data_range}.")
    if eps <= 0:
        raise ValueError(f"`eps` must be positive; received {eps}.")


def _stats(pred: Tensor, target: Tensor, data_range: float, clamp, eps: float) -> Tensor:
    """float64 [N, 5] = PSNR_R, PSNR_G, PSNR_B, their mean, CPSNR of two checked [N,3,H,W] tensors — nbp_rgb_psnr."""
    for t in (pred, target):
        if not t.is_cuda:
            raise _lib.NBPError(f"expected a tensor on the GPU, got {t.device}")
    p, t = pred.to(torch.float32).contiguous(), target.to(torch.float32).contiguous()
    N, L = p.shape[0], p.shape[2] * p.shape[3]
    if N == 0 or L == 0:
        raise ValueError(f"Empty input of shape {tuple(p.shape)}.")
    on, hi = _clamp_arg(clamp, data_range)
    with torch.cuda.device(p.device):
        ws = torch.empty(query("rgb_psnr_workspace_doubles", N, L), dtype=torch.float64, device=p.device)
        out = torch.empty(N, 5, dtype=torch.float64, device=p.device)
        call("rgb_psnr", p, t, N, L, float(data_range), float(eps), on, hi, ws, out)
    return out


@torch.no_grad()
def channel_stats(pred: Tensor, gt: Tensor, data_range: float = 1.0, clamp: Union[bool, float] = False,
                  eps: float = 1e-12) -> Tensor:
    """float64 [N, 5] on the device, columns PSNR_R, PSNR_G, PSNR_B, their mean (rgb_psnr's 'mean') and CPSNR
    (cpsnr_rgb) per image, `reduction='none'` values of the wrappers, with no host read: the reference's finiteness
    test is left out (as metrics.valstats.color_stats leaves it out), a non-finite input shows as NaN."""
    _check_range_eps(data_range, eps)
    pred, gt = _shape_checks(pred, gt)
    return _stats(pred, gt, data_range, clamp, eps)


@torch.no_grad()
def rgb_psnr(pred: Tensor, target: Tensor, *, data_range: float = 1.0, reduction: _Reduction = "mean",
             domain: Literal["linear", "srgb"] = "linear", clamp: Union[bool, float] = False, meta: bool = False,
             eps: float = 1e-12) -> Union[Dict[str, Tensor], PSNRResult]:
    """Per-channel PSNR (channelwise.py:111-168): {"R", "G", "B", "mean"} float64, and "meta" when asked."""
    _check_range_eps(data_range, eps)
    pred_n, target_n = _ensure_rgb(pred, target)
    _check_reduction(reduction)
    st = _stats(pred_n, target_n, data_range, clamp, eps)
    base = {"R": _reduce(st[:, 0], reduction), "G": _reduce(st[:, 1], reduction), "B": _reduce(st[:, 2], reduction),
            "mean": _reduce(st[:, 3], reduction)}
    if not meta:
        return base
    return PSNRResult(**base, meta={"domain": domain, "data_range": float(data_range)})


@torch.no_grad()
def cpsnr_rgb(pred: Tensor, target: Tensor, *, data_range: float = 1.0, reduction: _Reduction = "mean",
              domain: Literal["linear", "srgb"] = "linear", clamp: Union[bool, float] = False, meta: bool = False,
              eps: float = 1e-12) -> Union[Tensor, CPSNRResult]:
    """Colour PSNR (channelwise.py:170-222): the three channel MSEs averaged before the logarithm; float64."""
    _check_range_eps(data_range, eps)
    pred_n, target_n = _ensure_rgb(pred, target)
    _check_reduction(reduction)
    metric = _reduce(_stats(pred_n, target_n, data_range, clamp, eps)[:, 4], reduction)
    if not meta:
        return metric
    return CPSNRResult(cpsnr=metric, meta={"domain": domain, "data_range": float(data_range)})


def _ssim_checks(pred: Tensor, data_range, kernel_size, k1, k2, padding, eps) -> None:
    """ssim_linear's validation (metrics/linear.py:218-324), which the reference reaches per channel."""
    if data_range <= 0:
        raise ValueError(f"`data_range` must be positive, received {data_range}.")
    if eps <= 0:
        raise ValueError(f"`eps` must be positive, received {eps}.")
    if k1 < 0 or k2 < 0:
        raise ValueError("k1 and k2 must be non-negative.")
    n, _, h, w = pred.shape
    if n == 0:
        raise ValueError("Batch dimension cannot be zero.")
    if h == 0 or w == 0:
        raise ValueError("Spatial dimensions must be strictly positive.")
    if h < kernel_size or w < kernel_size:
        raise ValueError("Spatial dimensions must be >= kernel_size. "
                         f"Got H={h}, W={w}, kernel_size={kernel_size}.")
    if kernel_size <= 0 or kernel_size % 2 == 0:
        raise ValueError(f"kernel_size must be a positive odd integer; received {kernel_size}.")
    if padding not in _linear._PAD_CODE:
        raise ValueError(f"Unsupported padding mode '{padding}'.")


_WINDOWS: Dict[Tuple[int, float, bool, str], Tensor] = {}


def _window(kernel_size: int, sigma: float, gaussian: bool, device: torch.device) -> Tensor:
    """linear.ssim_plane_means' 1-D window on the device, uploaded once per (size, sigma, shape, device): a later call
    with the same window copies nothing from the host."""
    key = (int(kernel_size), float(sigma), bool(gaussian), str(device))
    if key not in _WINDOWS:
        _WINDOWS[key] = torch.tensor(_linear._window_1d(*key[:3]), dtype=torch.float32, device=device)
    return _WINDOWS[key]


def _ssim_scores(pred: Tensor, target: Tensor, data_range, kernel_size, sigma, k1, k2, gaussian, padding, eps) -> Tensor:
    """float32 [N, 3]: each channel's ssim_linear score (float64 plane mean cast to float32, as ssim_linear returns it
    for float32 inputs)."""
    c1, c2 = (k1 * float(data_range)) ** 2, (k2 * float(data_range)) ** 2
    p, t = _linear._f32(pred), _linear._f32(target)
    N, C, H, W = p.shape
    with torch.cuda.device(p.device):
        ws = torch.empty(query("ssim_linear_workspace_floats", N, C, H, W), device=p.device)
        out = torch.empty(N * C, dtype=torch.float64, device=p.device)
        call("ssim_linear", p, t, N, C, H, W, _window(kernel_size, sigma, gaussian, p.device), int(kernel_size),
             _linear._PAD_CODE[padding], float(c1), float(c2), float(eps), 1, 0, ws, out)
    return out.view(N, C).to(torch.float32)


@torch.no_grad()
def rgb_ssim(pred: Tensor, target: Tensor, *, data_range: float = 1.0, kernel_size: int = 11, sigma: float = 1.5,
             k1: float = 0.01, k2: float = 0.03, gaussian: bool = True, reduction: _Reduction = "mean",
             channel_aggregate: Literal["none", "mean"] = "none",
             padding: Literal["reflect", "replicate", "circular", "constant"] = "reflect",
             domain: Literal["linear", "srgb"] = "linear", meta: bool = False,
             eps: float = 1e-12) -> Union[Dict[str, Tensor], SSIMResult]:
    """Per-channel SSIM (channelwise.py:224-302): {"R", "G", "B", "mean"} float32; channel_aggregate='mean' repeats
    the aggregated value under all four keys."""
    pred_n, target_n = _ensure_rgb(pred, target)
    _ssim_checks(pred_n, data_range, kernel_size, k1, k2, padding, eps)
    _check_reduction(reduction)
    stack = _ssim_scores(pred_n, target_n, data_range, kernel_size, sigma, k1, k2, gaussian, padding, eps)
    mean_scores = stack.mean(dim=1)
    aggregated = _reduce(mean_scores, reduction)
    if channel_aggregate == "mean":
        base = {"R": aggregated, "G": aggregated, "B": aggregated, "mean": aggregated}
    else:
        base = {"R": _reduce(stack[:, 0], reduction), "G": _reduce(stack[:, 1], reduction),
                "B": _reduce(stack[:, 2], reduction), "mean": aggregated}
    if not meta:
        return base
    return SSIMResult(**base, meta={"domain": domain, "data_range": float(data_range)})


def register_channelwise_metrics() -> None:
    """Opt in: make three metric types available to validation.Validator, each a 0-d device tensor per item (the mean
    over the item's images) with no host synchronisation:

      cpsnr_rgb   channel_stats' CPSNR                          kwargs: data_range, clamp, eps
      rgb_psnr    channel_stats' channel mean, or one channel   kwargs: data_range, clamp, eps, channel: R | G | B
      rgb_ssim    the mean of the three channels' SSIM          kwargs: data_range, kernel_size, sigma, k1, k2,
                                                                        gaussian, padding, eps

    Nothing is registered unless this is called."""
    from ..validation import register_metric

    def _cpsnr(pred, gt, data_range=1.0, clamp=False, eps=1e-12):
        return channel_stats(pred, gt, data_range, clamp, eps)[:, 4].mean()

    def _psnr(pred, gt, data_range=1.0, clamp=False, eps=1e-12, channel=None):
        if channel not in (None, "R", "G", "B"):
            raise ValueError(f"rgb_psnr: channel must be R, G or B (or absent for the channel mean), got {channel!r}")
        col = 3 if channel is None else "RGB".index(channel)
        return channel_stats(pred, gt, data_range, clamp, eps)[:, col].mean()

    def _ssim(pred, gt, data_range=1.0, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03, gaussian=True, padding="reflect",
              eps=1e-12):
        p, t = _shape_checks(pred, gt)
        _ssim_checks(p, data_range, kernel_size, k1, k2, padding, eps)
        return _ssim_scores(p, t, data_range, kernel_size, sigma, k1, k2, gaussian, padding, eps).mean(dim=1).mean()

    register_metric("cpsnr_rgb", _cpsnr)
    register_metric("rgb_psnr", _psnr)
    register_metric("rgb_ssim", _ssim)
