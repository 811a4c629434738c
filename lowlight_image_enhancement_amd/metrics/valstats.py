"""Device-valued statistics for the validation pass (validation.py) on MI355X — valstats.hip.

The float-returning wrappers of metrics.color_error / metrics.lowlight_metrics synchronise the host several times per
frame and sort the ΔE00 and Sobel maps with torch.quantile (capped at 2^24 elements).  The functions here return
device tensors and never read one back:

  * quantile_rank / quantile_rows: torch.quantile's linear interpolation with the two order statistics taken by an
    exact radix select (nbp_quantile_select: three reads of the data, no sort, no size cap below 2^31 per row);
  * color_stats: the ΔE00 summary of metrics.lowlight_metrics (deltae2000_mean, deltae2000_p95,
    edge_deltae2000_mean) from one fused pass over the two images (nbp_val_color_maps), the per-image Sobel
    threshold by quantile_rows and the edge mean by nbp_masked_mean.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _lib
from .._lib import call, query
from .color_error import _whitepoint_warning

__all__ = ["quantile_rank", "quantile_select", "quantile_rows", "color_maps", "masked_mean", "color_stats"]


def quantile_rank(n: int, q: float) -> Tuple[int, int, float]:
    """(k_lo, k_hi, weight) of torch.quantile(x, q) (interpolation 'linear') over n fp32 values, in torch's own fp32
    arithmetic: rank = float32(q) * float32(n - 1), k_lo = floor(rank), k_hi = ceil(rank), weight = rank - k_lo, so that
    quantile = lerp(sorted[k_lo], sorted[k_hi], weight).  Above 2^24 elements (where torch.quantile refuses) the same
    arithmetic is used; float32(n - 1) may then round up, so the ranks are kept within [0, n - 1]."""
    n = int(n)
    if n < 1:
        raise ValueError(f"quantile_rank needs at least one element, got n={n}.")
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"q must lie within [0, 1]; received {q}.")
    rank = np.float32(q) * np.float32(n - 1)
    below = np.floor(rank)
    weight = np.float32(rank - below)
    k_lo = min(int(below), n - 1)
    k_hi = min(int(np.ceil(rank)), n - 1)
    return k_lo, k_hi, float(weight)


def _rows_f32(x: Tensor) -> Tensor:
    if not isinstance(x, Tensor):
        raise TypeError("expected a torch.Tensor.")
    if x.dim() != 2:
        raise ValueError(f"expected a [rows, n] tensor, got shape {tuple(x.shape)}.")
    _lib.require_cuda(x)
    return x.detach().contiguous()


def quantile_select(x: Tensor, k_lo: int, k_hi: int) -> Tensor:
    """[rows, 2] fp32: the k_lo-th and k_hi-th smallest value (zero-based) of each row of x [rows, n] — exact
    (nbp_quantile_select).  A row holding a NaN gives NaN in both slots."""
    x = _rows_f32(x)
    rows, n = x.shape
    if rows < 1 or n < 1:
        raise ValueError(f"quantile_select needs a non-empty [rows, n] tensor, got {tuple(x.shape)}.")
    if not 0 <= k_lo <= k_hi < n:
        raise ValueError(f"ranks must satisfy 0 <= k_lo <= k_hi < n={n}; received {k_lo}, {k_hi}.")
    ws = torch.empty(query("quantile_workspace_bytes", rows), dtype=torch.uint8, device=x.device)
    out = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    call("quantile_select", x, rows, n, int(k_lo), int(k_hi), ws, out)
    return out


def quantile_rows(x: Tensor, q: float) -> Tensor:
    """torch.quantile(x, q, dim=1) of x [rows, n] fp32 as a [rows] device tensor, without the sort and without
    torch.quantile's 2^24-element cap: two exact order statistics and the same torch.lerp."""
    x = _rows_f32(x)
    k_lo, k_hi, weight = quantile_rank(x.shape[1], q)
    v = quantile_select(x, k_lo, k_hi)
    return torch.lerp(v[:, 0], v[:, 1], weight)


def _ensure_nchw(rgb1: Tensor, rgb2: Tensor) -> Tuple[Tensor, Tensor]:
    """color_error._ensure_nchw's checks of type, shape, device and channels.  Its finiteness test reads the device, so
    it is left out here: a non-finite input shows as NaN in the statistics."""
    if not isinstance(rgb1, Tensor) or not isinstance(rgb2, Tensor):
        raise TypeError("deltaE2000 functions expect torch.Tensor inputs.")
    if rgb1.shape != rgb2.shape:
        raise ValueError(f"pred_srgb and target_srgb must share identical shape, got {tuple(rgb1.shape)} vs "
                         f"{tuple(rgb2.shape)}.")
    if rgb1.device != rgb2.device:
        raise ValueError("pred_srgb and target_srgb must reside on the same device.")
    if rgb1.ndim == 3:
        rgb1, rgb2 = rgb1.unsqueeze(0), rgb2.unsqueeze(0)
    elif rgb1.ndim != 4:
        raise ValueError("Expected tensors with 3 (C,H,W) or 4 (N,C,H,W) dimensions; "
                         f"received tensor with shape {tuple(rgb1.shape)}.")
    if rgb1.shape[1] != 3:
        raise ValueError(f"sRGB inputs must have 3 channels. Received {rgb1.shape[1]}.")
    if rgb1.shape[0] == 0 or rgb1.shape[2] == 0 or rgb1.shape[3] == 0:
        raise ValueError(f"Empty input of shape {tuple(rgb1.shape)}.")
    for t in (rgb1, rgb2):
        if not t.is_cuda:
            raise _lib.NBPError(f"expected a tensor on the GPU, got {t.device}")
    return rgb1.detach().to(torch.float32).contiguous(), rgb2.detach().to(torch.float32).contiguous()


@torch.no_grad()
def color_maps(pred: Tensor, target: Tensor, *, clamp: bool = True, kL: float = 1.0, kC: float = 1.0, kH: float = 1.0,
               eps: float = 1e-12) -> Tuple[Tensor, Tensor, Tensor]:
    """(de [N,H,W] fp32, grad [N,H,W] fp32, de_mean [N] float64): the ΔE00 map of deltaE2000_map, the Sobel magnitude
    of the prediction's L as edge_deltaE2000 computes it, and the per-image mean of the map — one kernel pass
    (nbp_val_color_maps), inputs clamped to [0, 1] first when `clamp`."""
    if eps <= 0:
        raise ValueError(f"`eps` must be positive, received {eps}.")
    pred, target = _ensure_nchw(pred, target)
    N, _, H, W = pred.shape
    dev = pred.device
    de = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    grad = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    de_mean = torch.empty(N, dtype=torch.float64, device=dev)
    ws = torch.empty(query("val_color_workspace_doubles", N, H, W), dtype=torch.float64, device=dev)
    call("val_color_maps", pred, target, N, H, W, int(bool(clamp)), float(kL), float(kC), float(kH), float(eps), ws, de,
         grad, de_mean)
    return de, grad, de_mean


def masked_mean(val: Tensor, key: Tensor, thr: Tensor) -> Dict[str, Tensor]:
    """Over val, key [rows, n] fp32 and thr [rows] fp32: float64 `sum` [rows] and int64 `count` [rows] of val where
    key >= thr[row], and `pooled_sum` / `pooled_count` (0-d) over all rows — nbp_masked_mean, fixed-order."""
    val, key = _rows_f32(val), _rows_f32(key)
    if val.shape != key.shape:
        raise ValueError(f"val and key must share one shape, got {tuple(val.shape)} vs {tuple(key.shape)}.")
    rows, n = val.shape
    _lib.require_cuda(thr)
    thr = thr.detach().contiguous()
    if thr.numel() != rows:
        raise ValueError(f"thr must hold one threshold per row ({rows}), got shape {tuple(thr.shape)}.")
    dev = val.device
    ws = torch.empty(query("masked_mean_workspace_doubles", rows, n), dtype=torch.float64, device=dev)
    s = torch.empty(rows + 1, dtype=torch.float64, device=dev)
    c = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    call("masked_mean", val, key, thr, rows, n, ws, s, c, s[rows:], c[rows:])
    return {"sum": s[:rows], "count": c[:rows], "pooled_sum": s[rows], "pooled_count": c[rows]}


@torch.no_grad()
def color_stats(pred: Tensor, target: Tensor, *, q: float = 0.85, whitepoint: str = "D65-2", clamp: bool = True,
                want_p95: bool = False) -> Dict[str, Tensor]:
    """The ΔE00 statistics of the validation metrics as 0-d float64 device tensors, without a host synchronisation:

      mean       the mean over images of the per-image ΔE00 mean                      (deltae2000_mean)
      edge_mean  the mean of ΔE00 over the pixels, pooled over the batch, whose Sobel |grad L| of the prediction is
                 >= that image's q-quantile of it                                       (edge_deltae2000_mean)
      p95        with want_p95: the 0.95 quantile of the pooled map                     (deltae2000_p95)

    `clamp` clamps both images to [0, 1] first, as those wrappers do."""
    if not 0.0 < q < 1.0:
        raise ValueError(f"q must lie within (0,1); received {q}.")
    _whitepoint_warning(whitepoint)
    de, grad, de_mean = color_maps(pred, target, clamp=clamp)
    N = de.shape[0]
    de2, grad2 = de.view(N, -1), grad.view(N, -1)
    thr = quantile_rows(grad2, q)
    m = masked_mean(de2, grad2, thr)
    out = {"mean": de_mean.mean(), "edge_mean": m["pooled_sum"] / m["pooled_count"]}
    if want_p95:
        out["p95"] = quantile_rows(de2.reshape(1, -1), 0.95)[0].to(torch.float64)
    return out
