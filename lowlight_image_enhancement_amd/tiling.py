"""Tiled full-frame inference: the reference validation loop's `val.grids` mode on the device
(NAFNet_base/basicsr/models/image_restoration_model.py: grids() :167-219, test() :324-342, grids_inverse() :221-245,
the switch :366-372).

A frame is cut into overlapping crops of the training size, the network runs on the crops in `max_minibatch` chunks, and
the overlapping outputs are averaged back into one frame.  Every SCA then pools over exactly the map it was trained on,
and the activation memory is that of one chunk whatever the frame.  The cut and the average are one HIP launch each
(nbp_grid_gather per chunk, nbp_grid_blend once; include/nbp.h).

The reference's grids_inverse() reads `self.outs`, which nothing there assigns (test() writes `self.output`), so
`val.grids: true` raises in the reference as written.  What is reproduced here is its evident intent: `outs` is test()'s
output, the tile outputs in tile order.

    from lowlight_image_enhancement_amd import tiled_forward, val_forward
    restored = tiled_forward(net, lq, {"crop_size_h": 256, "crop_size_w": 256, "max_minibatch": 16})
    restored = val_forward(net, lq, opt["val"])      # tiles when opt['val']['grids'] is set
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Mapping, Tuple

__all__ = ["grid_plan", "tiled_forward", "val_forward"]


def _crop_size(h: int, w: int, val_opt: Mapping) -> Tuple[int, int]:
    """crop_size_h / crop_size_w, or the ratio keys times the frame (:172-180); KeyError when an axis has neither"""
    crop_h = val_opt["crop_size_h"] if "crop_size_h" in val_opt else int(val_opt["crop_size_h_ratio"] * h)
    crop_w = val_opt["crop_size_w"] if "crop_size_w" in val_opt else int(val_opt["crop_size_w_ratio"] * w)
    return crop_h, crop_w


def grid_plan(h: int, w: int, val_opt: Mapping, scale: int = 1) -> Tuple[int, int, List[Dict[str, int]]]:
    """The reference's tile plan for an h x w frame: (crop_h, crop_w, idxes), idxes = [{'i': row origin, 'j': column
    origin}] in its order (row-major).  Pure Python, the loop of grids() :183-215 at scale 1."""
    if scale != 1:
        raise ValueError(f"grid_plan serves scale 1 only (NAFNet restores at the input size), got {scale}")
    crop_h, crop_w = _crop_size(h, w, val_opt)
    if not (1 <= crop_h <= h and 1 <= crop_w <= w):
        raise ValueError(f"crop {crop_h} x {crop_w} does not fit the {h} x {w} frame")
    num_row = (h - 1) // crop_h + 1
    num_col = (w - 1) // crop_w + 1
    step_j = crop_w if num_col == 1 else math.ceil((w - crop_w) / (num_col - 1) - 1e-8)
    step_i = crop_h if num_row == 1 else math.ceil((h - crop_h) / (num_row - 1) - 1e-8)
    idxes = []
    i, last_i = 0, False
    while i < h and not last_i:
        j = 0
        if i + crop_h >= h:
            i, last_i = h - crop_h, True
        last_j = False
        while j < w and not last_j:
            if j + crop_w >= w:
                j, last_j = w - crop_w, True
            idxes.append({"i": i, "j": j})
            j += step_j
        i += step_i
    return crop_h, crop_w, idxes


def _device_plan(h: int, w: int, crop_h: int, crop_w: int) -> Tuple[int, int, int, int]:
    """nbp_grid_plan: (n_rows, step_i, n_cols, step_j), the arguments of the two kernels"""
    from . import _lib
    out = (ctypes.c_int * 4)()
    base = ctypes.addressof(out)
    _lib.host_call("grid_plan", h, w, crop_h, crop_w, base, base + 4, base + 8, base + 12)
    return out[0], out[1], out[2], out[3]


def tiled_forward(net, lq, val_opt: Mapping):
    """grids() -> test() -> grids_inverse() for one frame: lq [1, C, H, W] fp32 on the device -> restored [1, C', H, W]
    fp32.  `net` maps a batch of tiles [n, C, crop_h, crop_w] to [n, C', crop_h, crop_w] (NAFNet in any precision,
    NAFNetLocal, the NewBP wrapper); val_opt carries the reference's opt['val'] keys crop_size_h / crop_size_w (or
    crop_size_h_ratio / crop_size_w_ratio) and max_minibatch (default: all tiles at once).  Runs under no_grad on the
    current stream, without a host synchronisation; the extra memory is one chunk of input tiles and the buffer of all
    tile outputs."""
    import torch

    from . import _lib
    if lq.dim() != 4 or lq.shape[0] != 1:
        raise ValueError(f"tiled_forward takes one frame [1, C, H, W] (the reference asserts b == 1), got "
                         f"{tuple(lq.shape)}")
    _lib.require_cuda(lq)
    _, C, H, W = lq.shape
    crop_h, crop_w, idxes = grid_plan(H, W, val_opt)
    plan = _device_plan(H, W, crop_h, crop_w)
    T = plan[0] * plan[2]
    if T != len(idxes):
        raise _lib.NBPError(f"nbp_grid_plan gives {T} tiles, the reference's loop {len(idxes)}")
    m = val_opt.get("max_minibatch", T)
    if m < 1:
        raise ValueError(f"max_minibatch must be at least 1, got {m}")
    with torch.no_grad():
        img = lq.detach().contiguous()
        outs = None
        for t0 in range(0, T, m):
            n = min(m, T - t0)
            tiles = torch.empty(n, C, crop_h, crop_w, device=lq.device, dtype=torch.float32)
            _lib.call("grid_gather", img, tiles, C, H, W, crop_h, crop_w, *plan, t0, n)
            pred = net(tiles)
            if isinstance(pred, list):
                pred = pred[-1]
            if pred.dim() != 4 or pred.shape[0] != n or tuple(pred.shape[2:]) != (crop_h, crop_w):
                raise ValueError(f"net mapped tiles {tuple(tiles.shape)} to {tuple(pred.shape)}; tiling needs the tile "
                                 "size kept")
            if outs is None:
                outs = torch.empty(T, pred.shape[1], crop_h, crop_w, device=lq.device, dtype=torch.float32)
            outs[t0:t0 + n].copy_(pred)
            del tiles, pred
        out = torch.empty(1, outs.shape[1], H, W, device=lq.device, dtype=torch.float32)
        _lib.call("grid_blend", outs, out, outs.shape[1], H, W, crop_h, crop_w, *plan)
    return out


def val_forward(net, lq, val_opt: Mapping):
    """The `grids` switch of the validation loop (:366-372): tiled_forward when val_opt['grids'] is set, else test()'s
    plain path, net over lq in max_minibatch chunks along the batch, concatenated."""
    import torch
    if val_opt.get("grids", False):
        return tiled_forward(net, lq, val_opt)
    n = len(lq)
    m = val_opt.get("max_minibatch", n)
    if m < 1:
        raise ValueError(f"max_minibatch must be at least 1, got {m}")
    outs = []
    with torch.no_grad():
        for i in range(0, n, m):
            pred = net(lq[i:i + m])
            if isinstance(pred, list):
                pred = pred[-1]
            outs.append(pred)
        return torch.cat(outs, dim=0)
