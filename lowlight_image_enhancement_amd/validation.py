"""The validation pass on the device (reference: ImageRestorationModel.nondist_validation / dist_validation,
NAFNet_base/basicsr/models/image_restoration_model.py:344-524, the tensor path `use_image: false`).

    val = Validator(opt["val"])                       # the reference's opt['val'], unchanged
    metrics = val.run(net, val_loader)                # OrderedDict name -> float, the mean over the loader's items

One forward per loader item (val_forward: plain or `grids`), every configured metric of basicsr.metrics.lowlight_metrics
added to a float64 vector on the device, `idx % world_size` sharding across ranks, one all_reduce and ONE device-to-host
read per pass.  The float-returning wrappers read the device five or more times per frame; here PSNR and SSIM call
their kernels directly (nbp_psnr, nbp_ssim_linear with a cached window), the colour metrics share one fused pass
(metrics.valstats.color_stats) and LPIPS stays on the device (LPIPSEvaluator.distance).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from typing import Callable, Dict, Mapping, Optional, Tuple

import torch
from torch import Tensor

__all__ = ["Validator", "register_metric", "SUPPORTED_METRICS", "image_name", "save_paths"]

SUPPORTED_METRICS = ("linear_psnr", "linear_ssim", "lpips_distance", "deltae2000_mean", "deltae2000_p95",
                     "edge_deltae2000_mean")
_ALLOWED_KW = {"linear_psnr": {"data_range"}, "linear_ssim": {"data_range"}, "lpips_distance": {"net", "device"},
               "deltae2000_mean": {"whitepoint"}, "deltae2000_p95": {"whitepoint"},
               "edge_deltae2000_mean": {"whitepoint", "q"}}
# further metric types: name -> fn(pred, gt, **kwargs) returning a 0-d tensor on the validator's device
_EXTRA: Dict[str, Callable[..., Tensor]] = {}
_WINDOWS: Dict[Tuple[int, float, str], Tensor] = {}


def register_metric(type_name: str, fn: Callable[..., Tensor]) -> None:
    """Make `type: type_name` available to Validator: fn(pred, gt, **kwargs) -> 0-d tensor on the device (it must not
    read the device back if update() is to stay free of host synchronisations)."""
    _EXTRA[type_name] = fn


def _window(kernel_size: int, sigma: float, device: torch.device) -> Tensor:
    """the 1-D SSIM window on the device, uploaded once per (kernel size, sigma, device)"""
    key = (int(kernel_size), float(sigma), str(device))
    if key not in _WINDOWS:
        from .metrics.linear import _window_1d
        _WINDOWS[key] = torch.tensor(_window_1d(key[0], key[1], True), dtype=torch.float32, device=device)
    return _WINDOWS[key]


def _evaluator(net: str, device: str):
    """the LPIPS evaluator lowlight_metrics.lpips_distance uses: one per (net, device), weights resident"""
    from .metrics.lpips_metric import evaluator
    return evaluator(net, device)


def _psnr(pred: Tensor, gt: Tensor, data_range: float) -> Tensor:
    """lowlight_metrics.linear_psnr -> calculate_psnr(gt, pred): the whole tensor as one sample, the difference in
    float64 (nbp_psnr), +inf when the mse is within 1e-12 of zero."""
    from .metrics.linear import psnr_per_sample
    if gt.shape != pred.shape:
        raise ValueError(f"Input shapes must match exactly, got {gt.shape=} and {pred.shape=}.")
    return psnr_per_sample(gt.reshape(1, -1), pred.reshape(1, -1), data_range, 1e-12, diff_double=True)[0]


def _ssim(pred: Tensor, gt: Tensor, data_range: float) -> Tensor:
    """lowlight_metrics.linear_ssim -> calculate_ssim(gt, pred) with its defaults (window 11 adjusted to the image,
    sigma 1.5, rgb, no resize policy): nbp_ssim_linear in the torchmetrics form, the window from the cache."""
    from ._lib import call, query
    from .metrics.ssim import _valid_kernel_size
    if pred.dim() == 3:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"SSIM expects two tensors of one [N,C,H,W] shape, got {tuple(gt.shape)} and "
                         f"{tuple(pred.shape)}.")
    p, t = pred.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    N, C, H, W = p.shape
    k = _valid_kernel_size(H, W, 11)
    c1, c2 = (0.01 * float(data_range)) ** 2, (0.03 * float(data_range)) ** 2
    ws = torch.empty(query("ssim_linear_workspace_floats", N, C, H, W), device=p.device)
    out = torch.empty(N * C, dtype=torch.float64, device=p.device)
    call("ssim_linear", p, t, N, C, H, W, _window(k, 1.5, p.device), k, 0, float(c1), float(c2), 0.0, 0, 1, ws, out)
    return out.view(N, C).mean(dim=1).mean()


def image_name(data: Mapping) -> str:
    """The reference's img_name of a loader item: the basename of its `lq_path` (a str, or the one-element list a
    DataLoader of batch size 1 makes of it) without the extension."""
    p = data.get("lq_path") if hasattr(data, "get") else None
    if isinstance(p, (list, tuple)):
        if len(p) != 1:
            raise ValueError(f"lq_path names {len(p)} files; images are saved one item at a time")
        p = p[0]
    if not isinstance(p, (str, os.PathLike)):
        raise ValueError("saving images needs every item's 'lq_path' (a str or a one-element list): it names the files")
    return os.path.splitext(os.path.basename(os.fspath(p)))[0]


def save_paths(save_dir: str, img_name: str, dataset_name: str = "val", current_iter=None) -> Tuple[str, str]:
    """Where the reference writes an item's restored frame and its ground truth (image_restoration_model.py:498-506):
    {save_dir}/{dataset_name}/{img_name}.png and ..._gt.png when testing (current_iter None), and
    {save_dir}/{img_name}/{img_name}_{current_iter}.png and ..._gt.png while training."""
    if current_iter is None:
        stem = os.path.join(save_dir, dataset_name, img_name)
    else:
        stem = os.path.join(save_dir, img_name, f"{img_name}_{current_iter}")
    return stem + ".png", stem + "_gt.png"


class Validator:
    """Accumulates the metrics of the reference's opt['val'] over a validation set, on the device.

    val_opt: `metrics: {name: {type: <one of SUPPORTED_METRICS>, **kwargs}}` with the keyword arguments of
    basicsr.metrics.lowlight_metrics (data_range; net, device; whitepoint; q), and the keys val_forward reads (grids,
    crop_size_h / crop_size_w or their _ratio forms, max_minibatch).  The keys `use_image` / `save_img` are rejected:
    the metrics run on the restored tensor, and images are saved by run(save_dir=...)."""

    def __init__(self, val_opt: Mapping, *, device=None) -> None:
        self.opt = val_opt
        for key in ("use_image", "save_img"):
            if val_opt.get(key, False):
                raise NotImplementedError(f"val.{key}: true is not supported: the metrics run on the restored tensor "
                                          "(use_image: false); to save the restored frames pass "
                                          "run(save_dir=...) instead of val.save_img")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.names = []
        self._simple = []   # (slot, fn(pred, gt) -> 0-d tensor)
        self._color = []    # (whitepoint, q, want_p95, {slot: key of color_stats' result})
        pending = []        # colour metrics: (slot, type, whitepoint, q)
        for slot, (name, cfg) in enumerate((val_opt.get("metrics") or {}).items()):
            kw = dict(cfg)
            typ = kw.pop("type", None)
            self.names.append(name)
            if typ in _EXTRA:
                self._simple.append((slot, lambda p, g, fn=_EXTRA[typ], kw=kw: fn(p, g, **kw)))
                continue
            if typ not in SUPPORTED_METRICS:
                raise ValueError(f"val.metrics.{name}: unknown metric type {typ!r}; supported types: "
                                 f"{', '.join(SUPPORTED_METRICS + tuple(_EXTRA))}")
            extra = set(kw) - _ALLOWED_KW[typ]
            if extra:
                raise TypeError(f"val.metrics.{name}: {typ} takes no argument {sorted(extra)}")
            if typ == "linear_psnr":
                dr = float(kw.get("data_range", 1.0))
                if dr <= 0:
                    raise ValueError(f"`data_range` must be positive, received {dr}.")
                self._simple.append((slot, lambda p, g, dr=dr: _psnr(p, g, dr)))
            elif typ == "linear_ssim":
                dr = float(kw.get("data_range", 1.0))
                if dr <= 0:
                    raise ValueError(f"data_range must be positive, received {dr}.")
                self._simple.append((slot, lambda p, g, dr=dr: _ssim(p, g, dr)))
                if self.device.type == "cuda":
                    _window(11, 1.5, self.device)  # the usual window, uploaded before the first update()
            elif typ == "lpips_distance":
                net_name, ev_dev = kw.get("net", "vgg"), kw.get("device") or str(self.device)
                if torch.device(ev_dev).type == "cuda":  # build and upload now: update() never waits for a copy
                    z = torch.zeros(1, 3, 32, 32, device=ev_dev)
                    _evaluator(net_name, ev_dev).distance(z, z)
                self._simple.append((slot, lambda p, g, n=net_name, d=ev_dev: _evaluator(n, d).distance(g, p)))
            else:
                wp = kw.get("whitepoint", "D65-2")
                q = float(kw.get("q", 0.85))
                if not 0.0 < q < 1.0:
                    raise ValueError(f"q must lie within (0,1); received {q}.")
                pending.append((slot, typ, wp, q))
        # colour metrics of one whitepoint share a fused pass; every further edge quantile needs a pass of its own
        groups: Dict[Tuple[str, float], Dict] = {}
        for slot, typ, wp, q in pending:
            if typ == "edge_deltae2000_mean":
                groups.setdefault((wp, q), {"p95": False, "slots": {}})["slots"][slot] = "edge_mean"
        for slot, typ, wp, q in pending:
            if typ != "edge_deltae2000_mean":
                key = next((k for k in groups if k[0] == wp), (wp, q))
                grp = groups.setdefault(key, {"p95": False, "slots": {}})
                grp["slots"][slot] = "mean" if typ == "deltae2000_mean" else "p95"
                grp["p95"] = grp["p95"] or typ == "deltae2000_p95"
        for (wp, q), grp in groups.items():
            self._color.append((wp, q, grp["p95"], grp["slots"]))
        self._acc: Optional[Tensor] = None
        self.reset()

    # ------------------------------------------------------------------ accumulation
    def reset(self) -> None:
        """forget every item seen"""
        self._acc = torch.zeros(len(self.names) + 1, dtype=torch.float64, device=self.device)  # metrics..., count

    @torch.no_grad()
    def update(self, pred: Tensor, gt: Tensor) -> None:
        """Add one loader item (restored output and ground truth, on the device): each configured metric of the item,
        as the reference's loop adds one float per item whatever the batch size.  No host synchronisation."""
        from .metrics.valstats import color_stats
        acc = self._acc
        for slot, fn in self._simple:
            acc[slot] += fn(pred, gt).to(torch.float64)
        for wp, q, want_p95, slots in self._color:
            st = color_stats(pred, gt, q=q, whitepoint=wp, clamp=True, want_p95=want_p95)
            for slot, key in slots.items():
                acc[slot] += st[key]
        acc[-1] += 1.0

    def result(self) -> "OrderedDict[str, float]":
        """The mean of every metric over the items seen (by all ranks when torch.distributed is initialised: one
        all_reduce(SUM) of the vector with its count), read from the device in one copy.  Empty without items."""
        import torch.distributed as dist
        v = self._acc
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            v = v.clone()
            dist.all_reduce(v, op=dist.ReduceOp.SUM)
        host = v.cpu()
        cnt = float(host[-1])
        out: "OrderedDict[str, float]" = OrderedDict()
        if cnt == 0:
            return out
        for i, name in enumerate(self.names):
            out[name] = float(host[i]) / cnt
        return out

    # ------------------------------------------------------------------ the pass
    def run(self, net, loader, *, rank: Optional[int] = None, world_size: Optional[int] = None,
            save_dir: Optional[str] = None, dataset_name: str = "val", current_iter=None, rgb2bgr: bool = True,
            writer=None) -> "OrderedDict[str, float]":
        """One validation pass: for every item of `loader` with idx % world_size == rank (a dict carrying 'lq' / 'gt' or
        'short' / 'long', CPU tensors are moved to the device), val_forward(net, lq, val_opt) under no_grad in eval mode
        (the previous mode is restored), then update(); returns result().  rank / world_size default to
        torch.distributed's when it is initialised, else 0 / 1.

        With `save_dir`, every item's restored frame and ground truth are also written as PNG files at save_paths(
        save_dir, image_name(item), dataset_name, current_iter) -- the reference's save_img -- through `writer` (an
        imgout.ImageWriter; by default one made for the pass), which takes the frames off the stream without a host
        synchronisation; the files are complete when run() returns, and the metrics are those of a pass without
        saving.  rgb2bgr is the reference's argument of that name (false reverses the channel order of the files)."""
        import torch.distributed as dist

        from .tiling import val_forward
        if rank is None or world_size is None:
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world_size = (dist.get_world_size() if on else 1) if world_size is None else world_size
        if world_size < 1 or not 0 <= rank < world_size:
            raise ValueError(f"rank {rank} / world_size {world_size}")
        own_writer = None
        if save_dir is not None and writer is None:
            from .imgout import ImageWriter
            writer = own_writer = ImageWriter()
        self.reset()
        was_training = bool(getattr(net, "training", False))
        if hasattr(net, "eval"):
            net.eval()
        try:
            with torch.no_grad():
                for idx, data in enumerate(loader):
                    if idx % world_size != rank:
                        continue
                    lq, gt = self._unpack(data)
                    pred = val_forward(net, lq, self.opt)
                    self.update(pred, gt)
                    if save_dir is not None:
                        img_path, gt_path = save_paths(save_dir, image_name(data), dataset_name, current_iter)
                        writer.write(pred, img_path, rgb2bgr=rgb2bgr)
                        writer.write(gt, gt_path, rgb2bgr=rgb2bgr)
            if save_dir is not None:
                writer.flush()
        finally:
            if own_writer is not None:
                own_writer.close()
            if hasattr(net, "train"):
                net.train(was_training)
        return self.result()

    def _unpack(self, data: Mapping) -> Tuple[Tensor, Tensor]:
        """LowlightModel.feed_data: ('lq', 'gt') or ('short', 'long')"""
        if "lq" in data and "gt" in data:
            lq, gt = data["lq"], data["gt"]
        elif "short" in data and "long" in data:
            lq, gt = data["short"], data["long"]
        else:
            raise ValueError(f"Validator.run expects items with ('lq','gt') or ('short','long'), got {list(data.keys())}")
        return lq.to(self.device), gt.to(self.device)
