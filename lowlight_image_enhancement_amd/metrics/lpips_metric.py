"""metrics.lpips_metric on MI355X (reference: metrics/lpips_metric.py:34-117, LPIPSEvaluator over lpips==0.1.4).

LPIPSEvaluator(net='alex' | 'vgg', device)(img_true, img_pred) -> float (.distance(...) gives the same value as a
device tensor, with the range test on the device too): the reference's input handling (shape checks,
[C,H,W] promoted to [1,C,H,W], [0,255] -> [0,1] when max > 1.5, [0,1] -> [-1,1] when the values lie in [0,1]) around
the MI355X LPIPS (lpips.py).  Parity unpinned: the lpips package and its pretrained weights are absent here.

Weights: `weights` (an lpips-style state_dict or a path), else the path in $NBP_LPIPS_WEIGHTS_ALEX / _VGG.  A metric
computed with the deterministic synthetic model would not be comparable with the reference's pretrained-weight LPIPS,
so without weights the evaluator raises -- unless `allow_synthetic=True` (or $NBP_LPIPS_ALLOW_SYNTHETIC=1) is given
explicitly, and then `synthetic` is True on the evaluator.

LPIPSMetric (:117-306) and evaluate_pairs (:309-337) are the reference's general evaluator: the same constructor
arguments (plus `weights`, `allow_synthetic`), input handling and statistics dict; the statistics are computed on the
device and read once, and the resize policy runs through nbp_resize_planes.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, List, Optional, Tuple

import torch

from ..lpips import LPIPS

__all__ = ["LPIPSEvaluator", "LPIPSMetric", "evaluate_pairs"]


class LPIPSEvaluator:
    """lpips_metric.py:34-117: callable average LPIPS distance over two image batches."""

    def __init__(self, net: str = "alex", device=None, weights=None, allow_synthetic: Optional[bool] = None) -> None:
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device)
        if weights is None:
            weights = os.environ.get(f"NBP_LPIPS_WEIGHTS_{net.upper()}") or None
        if allow_synthetic is None:
            allow_synthetic = os.environ.get("NBP_LPIPS_ALLOW_SYNTHETIC") == "1"
        if weights is None and not allow_synthetic:
            raise RuntimeError(f"LPIPS metric (net={net!r}): pretrained weights are required (pass weights=<lpips "
                               f"state_dict or path> or set NBP_LPIPS_WEIGHTS_{net.upper()}); the offline synthetic "
                               "model gives numbers not comparable with lpips 0.1.4 -- opt in with allow_synthetic=True")
        self.synthetic = weights is None
        self.loss_fn = LPIPS(net=net, weights=weights)
        self.loss_fn.eval()

    @staticmethod
    def _to_minus1_1(x: torch.Tensor) -> torch.Tensor:
        """lpips_metric.py:96-105."""
        if x.numel() == 0:
            return x
        mx, mn = float(x.max().item()), float(x.min().item())
        if mx > 1.5:  # treat as [0, 255]
            x = x / 255.0
        if mn >= 0.0 and mx <= 1.0:
            x = x * 2.0 - 1.0
        return x

    @staticmethod
    def _to_minus1_1_device(x: torch.Tensor) -> torch.Tensor:
        """_to_minus1_1 with the range test on the device: the same two rescalings, chosen by torch.where on the
        device-resident min / max instead of two host reads."""
        if x.numel() == 0:
            return x
        mx, mn = x.max(), x.min()
        x = torch.where(mx > 1.5, x / 255.0, x)  # treat as [0, 255]
        return torch.where((mn >= 0.0) & (mx <= 1.0), x * 2.0 - 1.0, x)

    def distance(self, img_true: torch.Tensor, img_pred: torch.Tensor) -> torch.Tensor:
        """__call__'s value as a 0-d tensor on the device, without a host synchronisation."""
        if img_true.shape != img_pred.shape:
            raise ValueError(f"Input shapes must match exactly, got {img_true.shape=} and {img_pred.shape=}.")
        if img_true.ndim not in (3, 4):
            raise ValueError(f"Inputs must be 3D (C,H,W) or 4D (N,C,H,W) tensors, received ndim={img_true.ndim}.")
        if img_true.ndim == 3:
            img_true, img_pred = img_true.unsqueeze(0), img_pred.unsqueeze(0)
        img_true = img_true.to(self.device, dtype=torch.float32)
        img_pred = img_pred.to(self.device, dtype=torch.float32)
        with torch.no_grad():
            d = self.loss_fn(self._to_minus1_1_device(img_pred).contiguous(),
                             self._to_minus1_1_device(img_true).contiguous())
        return d.mean()

    def __call__(self, img_true: torch.Tensor, img_pred: torch.Tensor) -> float:
        if img_true.shape != img_pred.shape:
            raise ValueError(f"Input shapes must match exactly, got {img_true.shape=} and {img_pred.shape=}.")
        if img_true.ndim not in (3, 4):
            raise ValueError(f"Inputs must be 3D (C,H,W) or 4D (N,C,H,W) tensors, received ndim={img_true.ndim}.")
        if img_true.ndim == 3:
            img_true, img_pred = img_true.unsqueeze(0), img_pred.unsqueeze(0)
        img_true = img_true.to(self.device, dtype=torch.float32)
        img_pred = img_pred.to(self.device, dtype=torch.float32)
        with torch.no_grad():
            d = self.loss_fn(self._to_minus1_1(img_pred).contiguous(), self._to_minus1_1(img_true).contiguous())
        return float(d.mean().item())


def resolve_weights(net: str, weights, allow_synthetic: Optional[bool]):
    """LPIPSEvaluator's weight rule for every metric entry point: `weights`, else $NBP_LPIPS_WEIGHTS_<NET>; without
    either a RuntimeError unless allow_synthetic (or $NBP_LPIPS_ALLOW_SYNTHETIC=1).  Returns (weights, synthetic)."""
    if weights is None:
        weights = os.environ.get(f"NBP_LPIPS_WEIGHTS_{net.upper()}") or None
    if allow_synthetic is None:
        allow_synthetic = os.environ.get("NBP_LPIPS_ALLOW_SYNTHETIC") == "1"
    if weights is None and not allow_synthetic:
        raise RuntimeError(f"LPIPS metric (net={net!r}): pretrained weights are required (pass weights=<lpips "
                           f"state_dict or path> or set NBP_LPIPS_WEIGHTS_{net.upper()}); the offline synthetic "
                           "model gives numbers not comparable with lpips 0.1.4 -- opt in with allow_synthetic=True")
    return weights, weights is None


def _resize_planes(x: torch.Tensor, size: Tuple[int, int], mode: str) -> torch.Tensor:
    """F.interpolate(x, size, mode='bilinear' | 'bicubic', align_corners=False) of [N,C,H,W] fp32 -- nbp_resize_planes."""
    from .._lib import call, require_cuda
    if mode not in ("bilinear", "bicubic"):
        raise NotImplementedError(f"resize_mode {mode!r}: the device resize implements 'bilinear' and 'bicubic'")
    x = x.contiguous()
    require_cuda(x)
    N, C, H, W = x.shape
    y = torch.empty(N, C, size[0], size[1], device=x.device)
    with torch.cuda.device(x.device):
        call("resize_planes", x, N * C, H, W, size[0], size[1], int(mode == "bicubic"), y)
    return y


def _stats_vector(d: torch.Tensor) -> torch.Tensor:
    """[mean, std (population), p50 = median, p95 = kthvalue(max(1, int(0.95 n)))] of the [n] scores, on their device."""
    n = d.numel()
    if n > 1:
        std = d.std(unbiased=False)
        p95 = d.kthvalue(max(1, int(0.95 * n)))[0]
    else:
        std, p95 = torch.zeros((), dtype=d.dtype, device=d.device), d.reshape(())
    return torch.stack([d.mean(), std, d.median(), p95])


class LPIPSMetric:
    """lpips_metric.py:117-306: model-agnostic LPIPS evaluation -- inputs in [0,255] / [0,1] / [-1,1] mapped to [-1,1]
    (the range test on the device: _to_minus1_1_device), gray replicated to three channels, C outside {1, 3} refused,
    sizes strict by default or aligned by `resize_policy` ('resize' with `keep_ratio` through nbp_resize_planes,
    'center_crop'); returns the per-image scores and mean / std / p50 / p95, computed on the device and read once.
    `weights` / `allow_synthetic` follow LPIPSEvaluator's rule (resolved when the model is first built)."""

    def __init__(self, net: str = "alex", version: str = "0.1", device=None, resize_policy: Optional[str] = None,
                 resize_mode: str = "bilinear", keep_ratio: bool = True, use_amp: bool = False, reduce: str = "mean",
                 eps: float = 1e-12, weights=None, allow_synthetic: Optional[bool] = None) -> None:
        self.net = net
        self.version = version
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device)
        self.resize_policy = resize_policy
        self.resize_mode = resize_mode
        self.keep_ratio = keep_ratio
        self.use_amp = use_amp
        self.reduce = reduce
        self.eps = eps
        self._weights = weights
        self._allow_synthetic = allow_synthetic
        self.synthetic: Optional[bool] = None
        self._lpips = None  # lazy init

    def _build_lpips(self):
        weights, self.synthetic = resolve_weights(self.net, self._weights, self._allow_synthetic)
        loss_fn = LPIPS(net=self.net, version=self.version, weights=weights)
        loss_fn.eval()
        return loss_fn

    def _resize_or_crop_pair(self, img_true, img_pred, policy: str, mode: str = "bilinear", keep_ratio: bool = True):
        """lpips_metric.py:161-221."""
        n, c, ht, wt = img_true.shape
        n2, c2, hp, wp = img_pred.shape
        if (n != n2) or (c != c2):
            raise ValueError(f"Batch/Channel mismatch for LPIPS: true {img_true.shape} vs pred {img_pred.shape}.")
        if policy == "resize":
            if (hp, wp) != (ht, wt):
                if keep_ratio:  # cover the ground truth keeping the aspect ratio, then centre-crop to its size
                    scale = max(ht / float(hp), wt / float(wp))
                    new_h, new_w = max(1, int(round(hp * scale))), max(1, int(round(wp * scale)))
                    tmp = _resize_planes(img_pred, (new_h, new_w), mode)
                    top, left = max((new_h - ht) // 2, 0), max((new_w - wt) // 2, 0)
                    img_pred = tmp[:, :, top:top + ht, left:left + wt]
                else:
                    img_pred = _resize_planes(img_pred, (ht, wt), mode)
            return img_true, img_pred
        if policy == "center_crop":
            h, w = min(ht, hp), min(wt, wp)

            def _center_crop(x):
                _, _, H, W = x.shape
                top, left = max((H - h) // 2, 0), max((W - w) // 2, 0)
                return x[:, :, top:top + h, left:left + w]

            return _center_crop(img_true), _center_crop(img_pred)
        raise ValueError(f"Unknown resize_policy: {policy}. Use None, 'resize', or 'center_crop'.")

    def _prepare_images(self, img_true: torch.Tensor, img_pred: torch.Tensor):
        """lpips_metric.py:223-273; the shape, channel and size checks come before anything moves to the device."""
        if img_true.ndim == 3:
            img_true = img_true.unsqueeze(0)
        if img_pred.ndim == 3:
            img_pred = img_pred.unsqueeze(0)
        if img_true.ndim != 4 or img_pred.ndim != 4:
            raise ValueError("LPIPS expects 4D tensors (N,C,H,W) or 3D that we can batch.")
        c_true, c_pred = img_true.shape[1], img_pred.shape[1]
        if c_true != c_pred:
            raise ValueError(f"LPIPS requires same channels for both inputs. Got C_true={c_true}, C_pred={c_pred}.")
        if c_true not in (1, 3):
            raise ValueError(f"LPIPS expects RGB 3-channel (or 1-channel to replicate). Got C={c_true}.")
        if self.resize_policy is None:
            if img_true.shape[-2:] != img_pred.shape[-2:]:
                raise ValueError(f"Image size mismatch {img_true.shape[-2:]} vs {img_pred.shape[-2:]}. Enable "
                                 "resize_policy to align.")
        elif self.resize_policy not in ("resize", "center_crop"):
            raise ValueError(f"Unknown resize_policy: {self.resize_policy}. Use None, 'resize', or 'center_crop'.")
        img_true = img_true.to(self.device, dtype=torch.float32)
        img_pred = img_pred.to(self.device, dtype=torch.float32)
        if c_true == 1:
            img_true, img_pred = img_true.repeat(1, 3, 1, 1), img_pred.repeat(1, 3, 1, 1)
        if self.resize_policy is not None:
            img_true, img_pred = self._resize_or_crop_pair(img_true, img_pred, self.resize_policy,
                                                           mode=self.resize_mode, keep_ratio=self.keep_ratio)
        to = LPIPSEvaluator._to_minus1_1_device
        return to(img_true).contiguous(), to(img_pred).contiguous()

    @torch.no_grad()
    def __call__(self, img_true: torch.Tensor, img_pred: torch.Tensor) -> Dict[str, object]:
        t, p = self._prepare_images(img_true, img_pred)
        lpips_model = self._lpips or self._build_lpips()
        self._lpips = lpips_model
        # use_amp: lpips under torch.cuda.amp.autocast runs its convs in half precision; here it selects the 16-bit
        # trunk the LPIPS module's `precision='auto'` resolves under autocast
        ctx = torch.autocast("cuda") if self.use_amp and t.is_cuda else contextlib.nullcontext()
        with ctx:
            d = lpips_model.forward(p, t).float().view(-1)
        n = d.numel()
        vec = _stats_vector(d)
        host = (torch.cat([vec, d]) if self.reduce == "none" else vec).cpu().tolist()  # the one read
        return {
            "per_image": host[4:] if self.reduce == "none" else None,
            "mean": host[0], "std": host[1], "p50": host[2], "p95": host[3],
            "net": self.net, "version": self.version, "resize_policy": self.resize_policy, "amp": self.use_amp,
            "count": int(n),
        }


def evaluate_pairs(pairs: List[Tuple[torch.Tensor, torch.Tensor]], **kwargs) -> Dict[str, object]:
    """lpips_metric.py:309-337: a list of (ground truth, prediction) pairs under one LPIPS configuration; each pair
    contributes its mean."""
    metric = LPIPSMetric(**kwargs)
    scores = [metric(gt, pred)["mean"] for gt, pred in pairs]
    tail = {"net": kwargs.get("net", "alex"), "version": kwargs.get("version", "0.1")}
    if not scores:
        nan = float("nan")
        return {"per_image": [], "mean": nan, "std": nan, "p50": nan, "p95": nan, "count": 0, **tail}
    x = torch.tensor(scores, dtype=torch.float32)
    m, s, p50, p95 = _stats_vector(x).tolist()
    return {"per_image": [float(v) for v in x.tolist()], "mean": m, "std": s, "p50": p50, "p95": p95,
            "count": int(x.numel()), **tail}


_CACHE: Dict[Tuple[str, str], LPIPSEvaluator] = {}


def evaluator(net: str, device: Optional[str]) -> LPIPSEvaluator:
    """One evaluator per (net, device): the reference rebuilds lpips.LPIPS on every lpips_distance call; the MI355X
    build keeps the device weights resident (same values)."""
    key = (net, str(device))
    if key not in _CACHE:
        _CACHE[key] = LPIPSEvaluator(net=net, device=device)
    return _CACHE[key]
