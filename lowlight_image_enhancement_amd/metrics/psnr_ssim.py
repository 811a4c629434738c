"""The image-domain PSNR and SSIM of BasicSR on the device (reference: NAFNet_base/basicsr/metrics/psnr_ssim.py, the
two numbers NAFNet's tables quote; the validation loop reaches them through `use_image: true`) -- psnr_ssim.hip.

    p = calculate_psnr(img1, img2, crop_border=0, input_order='HWC', test_y_channel=False)
    s = calculate_ssim(img1, img2, crop_border=0, input_order='HWC', test_y_channel=False, ssim3d=True)
    p = psnr_tensor(pred, gt); s = ssim_tensor(pred, gt)   # restored [1,3,H,W] tensors: tensor2img's bytes, then the metric
    register_image_metrics()                               # opt-in: `type: calculate_psnr` / `calculate_ssim` for Validator

The images are BGR, values in [0, 255] (or [0, 1]: max_value follows the data, as in the reference), numpy arrays
(uploaded) or tensors (a device tensor is read in place through its strides; crop_border and the stereo halves are
views).  uint8 and float32 are computed from exactly; any other type, float64 included, is cast to float32 first.
Two launches per call, no host synchronisation; the result is a 0-d float64 device tensor and is bitwise repeatable.

These are not metrics.psnr.calculate_psnr / metrics.ssim.calculate_ssim (the reference's top-level float-tensor
metrics, a different SSIM): import this module, not the bare names, from the metrics package.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .._lib import NBPError, call, query

__all__ = ["calculate_psnr", "calculate_psnr_left", "calculate_ssim", "calculate_ssim_left", "calculate_skimage_ssim",
           "calculate_skimage_ssim_left", "reorder_image", "to_y_channel", "psnr_tensor", "ssim_tensor",
           "register_image_metrics", "gaussian_window", "MODE_3D", "MODE_VALID", "MODE_Y"]

MODE_3D, MODE_VALID, MODE_Y = 0, 1, 2   # nbp_bsr_ssim's modes: _ssim_3d, _ssim, _ssim_cly
_WINDOWS: Dict[str, Tensor] = {}        # device -> the 11-tap window, float64


# ---------------------------------------------------------------------------------------------- host helpers
def gaussian_window(ksize: int = 11, sigma: float = 1.5) -> np.ndarray:
    """cv2.getGaussianKernel(ksize, sigma) for ksize > 7 as a flat float64 array: exp(-x^2 / (2 sigma^2)) over
    x = i - (ksize - 1) / 2, scaled by the reciprocal of its sum."""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return t * (1.0 / t.sum())


def reorder_image(img, input_order: str = "HWC"):
    """The reference's metric_util.reorder_image: (h, w) -> (h, w, 1); 'CHW' -> (h, w, c); 'HWC' unchanged.  A view."""
    if input_order not in ["HWC", "CHW"]:
        raise ValueError(f"Wrong input_order {input_order}. Supported input_orders are 'HWC' and 'CHW'")
    if len(img.shape) == 2:
        img = img[..., None]
    if input_order == "CHW":
        img = img.transpose(1, 2, 0)
    return img


def to_y_channel(img) -> np.ndarray:
    """The reference's metric_util.to_y_channel on the host, a numpy array in [0, 255] (HWC, BGR) -> float32
    [H, W, 1] (any other channel count: only x / 255 * 255 in float32), by the rounding chain the kernels use:
    v = fl32(x / 255), d = b 24.966 + g 128.553 + r 65.481 + 16 in float64, Y = fl32(fl32(d / 255) * 255)."""
    v = np.asarray(img).astype(np.float32) / np.float32(255.0)
    if v.ndim == 3 and v.shape[2] == 3:
        b, g, r = (v[..., k].astype(np.float64) for k in range(3))
        d = ((b * 24.966 + g * 128.553) + r * 65.481) + 16.0
        v = (d / 255.0).astype(np.float32)[..., None]
    return v * np.float32(255.0)


# ---------------------------------------------------------------------------------------------- the views
def _device_of(*imgs) -> torch.device:
    for x in imgs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise NBPError("the image metrics run on the GPU and none is available; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _hwc(img, input_order: str, who: str):
    """the image as (rows, columns, channels), still on its side of the bus: the reference's argument handling"""
    if type(img) == Tensor or torch.is_tensor(img):
        if input_order == "CHW":
            # the reference transposes a tensor to HWC and then applies input_order again: a double transpose
            raise ValueError(f"{who}: a torch.Tensor is CHW already and is taken so; with input_order='CHW' the "
                             "reference transposes it twice, which is not reproduced.  Pass input_order='HWC'")
        t = img.detach()
        if t.dim() == 4:
            t = t.squeeze(0)
        if t.dim() != 3:
            raise ValueError(f"{who}: a torch.Tensor is [C,H,W] or [1,C,H,W], got {tuple(img.shape)}")
        return t.permute(1, 2, 0)
    if not isinstance(img, np.ndarray):
        raise TypeError(f"{who}: img must be a numpy array or a torch.Tensor, got {type(img)}")
    if img.ndim == 2:
        return img[..., None]  # input_order has no effect on (h, w)
    if img.ndim != 3:
        raise ValueError(f"{who}: expected a 2-D or 3-D image, got shape {img.shape}")
    return img.transpose(1, 2, 0) if input_order == "CHW" else img


def _upload(x, dev: torch.device, as_float: bool) -> Tensor:
    """a [H, W, C] view on the device, uint8 or float32, strides kept where the data is there already"""
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint8 and not as_float:
            x = np.ascontiguousarray(x)
        else:
            x = np.ascontiguousarray(x, dtype=np.float32)
        return torch.from_numpy(x).to(dev)
    if x.device != dev:
        x = x.to(dev)
    if x.dtype == torch.uint8 and not as_float:
        return x
    return x if x.dtype == torch.float32 else x.to(torch.float32)


def _is_u8(x) -> bool:
    return x.dtype == (np.uint8 if isinstance(x, np.ndarray) else torch.uint8)


def _pair(img1, img2, crop_border: int, input_order: str, who: str) -> Tuple[Tensor, Tensor]:
    """both images as cropped [H, W, C] device views of one type (the reference's checks, in its order)"""
    assert img1.shape == img2.shape, (f'Image shapes are differnet: {img1.shape}, {img2.shape}.')
    if input_order not in ['HWC', 'CHW']:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are "HWC" and "CHW"')
    a, b = _hwc(img1, input_order, who), _hwc(img2, input_order, who)
    if tuple(a.shape) != tuple(b.shape):
        raise AssertionError(f'Image shapes are differnet: {tuple(a.shape)}, {tuple(b.shape)}.')
    cb = int(crop_border)
    if cb < 0:
        raise ValueError(f"crop_border must not be negative, got {crop_border}")
    H, W, C = a.shape
    if C not in (1, 3, 6):
        raise ValueError(f"{who}: 1 or 3 channels (BGR), or 6 (a stereo pair), got {C}")
    if H - 2 * cb < 1 or W - 2 * cb < 1:
        raise ValueError(f"{who}: nothing is left of a {H} x {W} image after crop_border {cb}")
    dev = _device_of(img1, img2)
    as_float = not (_is_u8(a) and _is_u8(b))
    a, b = _upload(a, dev, as_float), _upload(b, dev, as_float)
    if cb:
        a, b = a[cb:H - cb, cb:W - cb], b[cb:H - cb, cb:W - cb]
    return a, b


def _window(dev: torch.device) -> Tensor:
    key = str(dev)
    if key not in _WINDOWS:
        _WINDOWS[key] = torch.from_numpy(gaussian_window(11, 1.5)).to(dev)
    return _WINDOWS[key]


def _strides(t: Tensor):
    return t.stride(0), t.stride(1), t.stride(2)


def _psnr_view(a: Tensor, b: Tensor, y: bool) -> Tensor:
    H, W, C = a.shape
    dev = a.device
    with torch.cuda.device(dev):
        ws = torch.empty(query("bsr_psnr_workspace_bytes", H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)
        call("bsr_psnr", a, b, int(a.dtype == torch.uint8), H, W, C, *_strides(a), *_strides(b), int(y), ws, out)
    return out[0]


def _ssim_view(a: Tensor, b: Tensor, mode: int) -> Tensor:
    H, W, C = a.shape
    dev = a.device
    win = _window(dev)
    with torch.cuda.device(dev):
        ws = torch.empty(query("bsr_ssim_workspace_bytes", H, W, mode), dtype=torch.uint8, device=dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)
        call("bsr_ssim", a, b, int(a.dtype == torch.uint8), H, W, C, *_strides(a), *_strides(b), mode, win, ws, out)
    return out[0]


def _stereo(fn, a: Tensor, b: Tensor, arg) -> Tensor:
    """a 6-channel image is a stereo pair: the mean of the two 3-channel results"""
    if a.shape[2] == 6:
        return (fn(a[:, :, :3], b[:, :, :3], arg) + fn(a[:, :, 3:], b[:, :, 3:], arg)) / 2
    return fn(a, b, arg)


# ---------------------------------------------------------------------------------------------- the reference's names
@torch.no_grad()
def calculate_psnr(img1, img2, crop_border, input_order: str = 'HWC', test_y_channel: bool = False) -> Tensor:
    """The reference's calculate_psnr as a 0-d float64 device tensor: 20 log10(max_value / sqrt(mse)), the mse in
    float64 over the cropped image (over its Y plane with test_y_channel), max_value 1 if img1 (its Y plane) has no
    value above 1, else 255; +inf when the mse is 0; six channels: the mean over the stereo halves.

    numpy arrays follow input_order ('HWC' or 'CHW'; 2-D is one channel).  A torch.Tensor is [C,H,W] or [1,C,H,W], as
    the reference takes it; with input_order='CHW' the reference transposes it a second time, so that combination
    raises ValueError here.  Nothing waits for the device."""
    a, b = _pair(img1, img2, crop_border, input_order, "calculate_psnr")
    return _stereo(_psnr_view, a, b, bool(test_y_channel))


def calculate_psnr_left(img1, img2, crop_border, input_order: str = 'HWC', test_y_channel: bool = False) -> Tensor:
    """The reference's calculate_psnr_left: the left view of a stereo pair right of its first 64 columns."""
    assert input_order == 'HWC'
    assert crop_border == 0
    return calculate_psnr(img1=img1[:, 64:, :3], img2=img2[:, 64:, :3], crop_border=0, input_order=input_order,
                          test_y_channel=test_y_channel)


@torch.no_grad()
def calculate_ssim(img1, img2, crop_border, input_order: str = 'HWC', test_y_channel: bool = False,
                   ssim3d: bool = True) -> Tensor:
    """The reference's calculate_ssim as a 0-d float64 device tensor: the mean of the SSIM map under the 11-tap
    sigma-1.5 Gaussian.  ssim3d (the default): the [H,W,C] volume in float32 under the 11 x 11 x 11 kernel with a
    replicated border on all three axes, evaluated in float64 (the value the reference's float32 conv3d scatters
    around).  ssim3d=False: per channel in float64, the [5:-5, 5:-5] region; NaN when H or W <= 10.
    test_y_channel: the Y plane in float64, replicated border, C1 and C2 for 255.  Arguments as calculate_psnr."""
    a, b = _pair(img1, img2, crop_border, input_order, "calculate_ssim")
    mode = MODE_Y if test_y_channel else (MODE_3D if ssim3d else MODE_VALID)
    return _stereo(_ssim_view, a, b, mode)


def calculate_ssim_left(img1, img2, crop_border, input_order: str = 'HWC', test_y_channel: bool = False,
                        ssim3d: bool = True) -> Tensor:
    """The reference's calculate_ssim_left: the left view of a stereo pair right of its first 64 columns."""
    assert input_order == 'HWC'
    assert crop_border == 0
    return calculate_ssim(img1=img1[:, 64:, :3], img2=img2[:, 64:, :3], crop_border=0, input_order=input_order,
                          test_y_channel=test_y_channel, ssim3d=ssim3d)


def calculate_skimage_ssim(img1, img2):
    raise NotImplementedError("calculate_skimage_ssim wraps skimage.metrics.structural_similarity, which is not part "
                              "of this project; use calculate_ssim")


def calculate_skimage_ssim_left(img1, img2):
    raise NotImplementedError("calculate_skimage_ssim_left wraps skimage.metrics.structural_similarity, which is not "
                              "part of this project; use calculate_ssim_left")


# ---------------------------------------------------------------------------------------------- the tensor route
def _bytes_pair(pred: Tensor, gt: Tensor, rgb2bgr: bool, min_max: Sequence[float], crop_border: int, who: str):
    """tensor2img's bytes of both tensors (imgout's device quantiser) as cropped [H,W,3] views"""
    from ..imgout import _as_chw, _min_max, _quantize
    lo, hi = _min_max(min_max)
    views = []
    for t in (pred, gt):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise TypeError(f"{who} expects tensors on the GPU")
        chw, n_dim = _as_chw(t)
        if n_dim != 3 or chw.shape[0] != 3:
            raise ValueError(f"{who} expects [1,3,H,W] or [3,H,W], got {tuple(t.shape)}")
        views.append(_quantize(chw, lo, hi, bool(rgb2bgr)))
    a, b = views
    assert a.shape == b.shape, (f'Image shapes are differnet: {tuple(a.shape)}, {tuple(b.shape)}.')
    cb = int(crop_border)
    H, W, _ = a.shape
    if cb < 0 or H - 2 * cb < 1 or W - 2 * cb < 1:
        raise ValueError(f"{who}: crop_border {crop_border} leaves nothing of a {H} x {W} image")
    if cb:
        a, b = a[cb:H - cb, cb:W - cb], b[cb:H - cb, cb:W - cb]
    return a, b


@torch.no_grad()
def psnr_tensor(pred: Tensor, gt: Tensor, crop_border: int = 0, test_y_channel: bool = False, rgb2bgr: bool = True,
                min_max: Sequence[float] = (0, 1)) -> Tensor:
    """calculate_psnr of two restored [1,3,H,W] or [3,H,W] device tensors by the reference's `use_image` route:
    tensor2img of both (clamp to min_max, * 255, round half to even, BGR bytes), then the metric."""
    a, b = _bytes_pair(pred, gt, rgb2bgr, min_max, crop_border, "psnr_tensor")
    return _psnr_view(a, b, bool(test_y_channel))


@torch.no_grad()
def ssim_tensor(pred: Tensor, gt: Tensor, crop_border: int = 0, test_y_channel: bool = False, rgb2bgr: bool = True,
                min_max: Sequence[float] = (0, 1), ssim3d: bool = True) -> Tensor:
    """calculate_ssim of two restored device tensors by the `use_image` route, as psnr_tensor."""
    a, b = _bytes_pair(pred, gt, rgb2bgr, min_max, crop_border, "ssim_tensor")
    return _ssim_view(a, b, MODE_Y if test_y_channel else (MODE_3D if ssim3d else MODE_VALID))


def register_image_metrics(psnr: Optional[str] = "calculate_psnr", ssim: Optional[str] = "calculate_ssim",
                           **defaults) -> None:
    """Opt in: make `type: <psnr>` and `type: <ssim>` available to validation.Validator as psnr_tensor / ssim_tensor of
    (pred, gt), with the reference's YAML keyword arguments crop_border, input_order (only 'HWC': the restored tensor
    has one layout), test_y_channel and, for SSIM, ssim3d.  `defaults` pre-set them.  A name of None registers
    nothing for that metric; nothing at all is registered unless this is called."""
    from ..validation import register_metric
    extra = set(defaults) - {"crop_border", "input_order", "test_y_channel", "ssim3d"}
    if extra:
        raise TypeError(f"register_image_metrics takes the defaults crop_border, input_order, test_y_channel and "
                        f"ssim3d, got {sorted(extra)}")
    d_cb, d_order = defaults.get("crop_border", 0), defaults.get("input_order", "HWC")
    d_y, d_3d = defaults.get("test_y_channel", False), defaults.get("ssim3d", True)

    def _order(input_order):
        if input_order != "HWC":
            raise ValueError(f"the registered image metrics take input_order 'HWC' only, got {input_order!r}")

    _order(d_order)

    def psnr_fn(pred, gt, crop_border=d_cb, input_order=d_order, test_y_channel=d_y):
        _order(input_order)
        return psnr_tensor(pred, gt, crop_border=crop_border, test_y_channel=test_y_channel)

    def ssim_fn(pred, gt, crop_border=d_cb, input_order=d_order, test_y_channel=d_y, ssim3d=d_3d):
        _order(input_order)
        return ssim_tensor(pred, gt, crop_border=crop_border, test_y_channel=test_y_channel, ssim3d=ssim3d)

    if psnr is not None:
        register_metric(psnr, psnr_fn)
    if ssim is not None:
        register_metric(ssim, ssim_fn)
