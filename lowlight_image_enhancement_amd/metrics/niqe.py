"""NIQE on the device (reference: NAFNet_base/basicsr/metrics/niqe.py `calculate_niqe`, the one metric of the
reference's basicsr.metrics that scores a restored frame without a ground truth) -- niqe.hip.

    q = calculate_niqe(img, crop_border=0)          # img: BGR HWC uint8 / float32 in [0, 255], device tensor or numpy
    q = niqe_tensor(out)                            # a restored [1,3,H,W] tensor: tensor2img's bytes, then the metric
    register_niqe_metric("niqe")                    # opt-in: `type: niqe` for validation.Validator

Three launches per frame and no host synchronisation: nbp_niqe_luma (the Y plane, read through strides: no layout
needs a copy), nbp_niqe_features (the MSCN map and the AGGD fits, one work-group per block and scale) and
nbp_niqe_score (nanmean, clean-row covariance, Cholesky solve).  The result is a 0-d float64 device tensor.

The pristine model (mu_pris_param, cov_pris_param, gaussian_window) is data of the reference and is not shipped:
`params` is a path to its niqe_pris_params.npz or a mapping with those three keys; None tries the environment variable
NBP_NIQE_PARAMS and then the reference's own relative path basicsr/metrics/niqe_pris_params.npz.
"""
from __future__ import annotations

import hashlib
import math
import os
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .._lib import NBPError, call, query

__all__ = ["calculate_niqe", "niqe_features", "niqe_tensor", "register_niqe_metric", "aggd_tables", "load_params",
           "PARAMS_ENV", "PARAMS_RELATIVE"]

PARAMS_ENV = "NBP_NIQE_PARAMS"
PARAMS_RELATIVE = os.path.join("basicsr", "metrics", "niqe_pris_params.npz")
BLOCK = 96
_PARAM_KEYS = ("mu_pris_param", "cov_pris_param", "gaussian_window")

_HOST_PARAMS: Dict[str, Dict[str, np.ndarray]] = {}          # path -> arrays
_DEVICE_PARAMS: Dict[Tuple[str, str], Dict[str, Tensor]] = {}  # (path or mapping digest, device) -> mu, cov, window
_DEVICE_TABLES: Dict[str, Tensor] = {}                        # device -> [4][9801]
_HOST_TABLES: Optional[np.ndarray] = None


# ---------------------------------------------------------------------------------------------- tables and parameters
def aggd_tables() -> np.ndarray:
    """float64 [4][9801] over the reference's grid gam = np.arange(0.2, 10.001, 0.001): r_gam = Gamma(2/a)^2 /
    (Gamma(1/a) Gamma(3/a)), sqrt(Gamma(1/a) / Gamma(3/a)), Gamma(2/a) / Gamma(1/a) and gam itself, built with
    math.gamma in float64 (the kernel needs no Gamma function)."""
    global _HOST_TABLES
    if _HOST_TABLES is None:
        gam = np.arange(0.2, 10.001, 0.001)
        t = np.empty((4, gam.size), dtype=np.float64)
        for i, a in enumerate(gam.tolist()):
            rec = 1.0 / a
            g1, g2, g3 = math.gamma(rec), math.gamma(rec * 2), math.gamma(rec * 3)
            t[0, i] = g2 * g2 / (g1 * g3)
            t[1, i] = math.sqrt(g1 / math.gamma(3 / a))
            t[2, i] = math.gamma(2 / a) / g1
        t[3] = gam
        _HOST_TABLES = t
    return _HOST_TABLES


def _check_params(p: Mapping, where: str) -> Dict[str, np.ndarray]:
    missing = [k for k in _PARAM_KEYS if k not in p]
    if missing:
        raise KeyError(f"NIQE parameters from {where} lack {missing}")
    mu = np.asarray(p["mu_pris_param"], dtype=np.float64).reshape(-1)
    cov = np.asarray(p["cov_pris_param"], dtype=np.float64)
    win = np.asarray(p["gaussian_window"], dtype=np.float64)
    if mu.shape != (36,) or cov.shape != (36, 36) or win.shape != (7, 7):
        raise ValueError(f"NIQE parameters from {where}: expected mu [36] (or [1,36]), cov [36,36] and a 7 x 7 window, "
                         f"got {mu.shape}, {cov.shape}, {win.shape}")
    return {"mu_pris_param": mu, "cov_pris_param": cov, "gaussian_window": win}


def load_params(params=None) -> Tuple[str, Dict[str, np.ndarray]]:
    """(cache key, {mu_pris_param [36], cov_pris_param [36,36], gaussian_window [7,7]} as float64 numpy) from a path, a
    mapping, or (None) $NBP_NIQE_PARAMS and then basicsr/metrics/niqe_pris_params.npz relative to the working
    directory, as the reference loads it."""
    if params is not None and not isinstance(params, (str, os.PathLike)):
        if not isinstance(params, Mapping) and not hasattr(params, "files"):
            raise TypeError(f"params must be a path or a mapping with {_PARAM_KEYS}, got {type(params)}")
        host = _check_params(params, "the mapping")
        digest = hashlib.sha1(b"".join(host[k].tobytes() for k in _PARAM_KEYS)).hexdigest()
        return f"<mapping {digest}>", host
    if params is None:
        env = os.environ.get(PARAMS_ENV)
        path = None
        for cand in ([env] if env else []) + [PARAMS_RELATIVE]:
            if os.path.isfile(cand):
                path = cand
                break
        if path is None:
            raise FileNotFoundError(
                f"NIQE needs the reference's pristine model niqe_pris_params.npz, which is not shipped: "
                f"${PARAMS_ENV} is {'unset' if not env else repr(env) + ' (no such file)'} and "
                f"{PARAMS_RELATIVE!r} does not exist under {os.getcwd()!r}; pass params=<path or mapping>")
    else:
        path = os.fspath(params)
    path = os.path.abspath(path)
    if path not in _HOST_PARAMS:
        with np.load(path, allow_pickle=False) as f:
            _HOST_PARAMS[path] = _check_params(f, path)
    return path, _HOST_PARAMS[path]


def _device_params(params, device: torch.device) -> Dict[str, Tensor]:
    """mu [36], cov [36,36] and the correlation weights [49] on the device, uploaded once per (path, device)"""
    key, host = load_params(params)
    cached = _DEVICE_PARAMS.get((key, str(device)))
    if cached is not None:
        return cached
    out = {
        "mu": torch.from_numpy(host["mu_pris_param"].copy()).to(device),
        "cov": torch.from_numpy(np.ascontiguousarray(host["cov_pris_param"])).to(device),
        # scipy.ndimage.convolve correlates with the flipped window
        "window": torch.from_numpy(np.ascontiguousarray(host["gaussian_window"][::-1, ::-1]).reshape(-1)).to(device),
    }
    _DEVICE_PARAMS[(key, str(device))] = out
    return out


def _device_tables(device: torch.device) -> Tensor:
    key = str(device)
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.from_numpy(aggd_tables()).to(device)
    return _DEVICE_TABLES[key]


# ---------------------------------------------------------------------------------------------- the frame
def _frame_view(img, crop_border: int, input_order: str, convert_to: str) -> Tuple[Tensor, int, int, int]:
    """(view [H, W, C] of the cropped frame on the device, uint8 or float32, any strides; H; W; C) -- the reference's
    argument handling (metric_util.reorder_image) without touching the pixels."""
    if convert_to == "gray":
        raise NotImplementedError("calculate_niqe: convert_to='gray' goes through cv2.cvtColor and is not implemented; "
                                  "use convert_to='y'")
    if convert_to != "y":
        raise ValueError(f"Wrong convert_to {convert_to}. Supported values are 'y' and 'gray'")
    if input_order not in ("HWC", "CHW", "HW"):
        raise ValueError(f"Wrong input_order {input_order}. Supported input_orders are 'HWC' and 'CHW'")
    if not isinstance(img, np.ndarray) and not torch.is_tensor(img):
        raise TypeError(f"img must be a torch.Tensor or a numpy array, got {type(img)}")
    # the shape first, on the host: (rows, columns, channels) by the layout
    shape = tuple(img.shape)
    if input_order == "HW" or len(shape) == 2:
        if len(shape) != 2:
            raise ValueError(f"input_order 'HW' needs a 2-D image, got shape {shape}")
        H, W, C = shape[0], shape[1], 1
    elif len(shape) != 3:
        raise ValueError(f"expected a 3-D image for input_order {input_order!r}, got shape {shape}")
    else:
        H, W, C = (shape[1], shape[2], shape[0]) if input_order == "CHW" else shape
    if C not in (1, 3):
        raise ValueError(f"the image has 1 or 3 channels (BGR), got {C}")
    cb = int(crop_border)
    if cb < 0:
        raise ValueError(f"crop_border must not be negative, got {crop_border}")
    H, W = H - 2 * cb, W - 2 * cb
    if H < BLOCK or W < BLOCK:
        raise ValueError(f"NIQE needs at least one {BLOCK} x {BLOCK} block; the frame is {H} x {W} after crop_border")
    if isinstance(img, np.ndarray):
        if img.dtype not in (np.uint8, np.float32):
            img = img.astype(np.float32)
        if not torch.cuda.is_available():
            raise NBPError("calculate_niqe runs on the GPU and none is available; there is no CPU fallback")
        t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    else:
        t = img.detach()
        if not t.is_cuda:
            raise NBPError(f"expected a tensor on the GPU (or a numpy array), got {t.device}")
        if t.dtype not in (torch.uint8, torch.float32):
            t = t.to(torch.float32)
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    elif input_order == "CHW":
        t = t.permute(1, 2, 0)
    t = t[cb:cb + H, cb:cb + W]
    return t, H, W, C


def _features(t: Tensor, H: int, W: int, C: int, par: Dict[str, Tensor]) -> Tensor:
    dev = t.device
    nbh, nbw = H // BLOCK, W // BLOCK
    with torch.cuda.device(dev):
        y = torch.empty((nbh * BLOCK, nbw * BLOCK), dtype=torch.float32, device=dev)
        call("niqe_luma", t, int(t.dtype == torch.uint8), H, W, C, t.stride(0), t.stride(1), t.stride(2) if C == 3 else 0,
             y)
        ws = torch.empty(query("niqe_workspace_bytes", H, W), dtype=torch.uint8, device=dev)
        feat = torch.empty((nbh * nbw, 36), dtype=torch.float64, device=dev)
        call("niqe_features", y, H, W, par["window"], _device_tables(dev), ws, feat)
    return feat


def _score(feat: Tensor, par: Dict[str, Tensor]) -> Tensor:
    out = torch.empty(1, dtype=torch.float64, device=feat.device)
    with torch.cuda.device(feat.device):
        call("niqe_score", feat, feat.shape[0], par["mu"], par["cov"], out)
    return out[0]


@torch.no_grad()
def niqe_features(img, crop_border: int, input_order: str = "HWC", convert_to: str = "y", *, params=None) -> Tensor:
    """The [blocks, 36] float64 feature matrix the reference's `niqe` forms before its Gaussian fit (rows in its
    order: idx_w outer, idx_h inner; columns: 18 of scale 1, 18 of scale 2), on the device."""
    t, H, W, C = _frame_view(img, crop_border, input_order, convert_to)
    return _features(t, H, W, C, _device_params(params, t.device))


@torch.no_grad()
def calculate_niqe(img, crop_border: int, input_order: str = "HWC", convert_to: str = "y", *, params=None) -> Tensor:
    """The reference's calculate_niqe(img, crop_border, input_order, convert_to='y') as a 0-d float64 device tensor.

    img: values in [0, 255], uint8 or float32 (other types are cast to float32, as the reference casts), BGR channel
    order, layout 'HWC', 'CHW' or 'HW'; a device tensor of any strides (read in place) or a numpy array (uploaded).
    Nothing waits for the device.  Fewer than two blocks without a NaN feature give NaN (the reference raises there)."""
    t, H, W, C = _frame_view(img, crop_border, input_order, convert_to)
    par = _device_params(params, t.device)
    return _score(_features(t, H, W, C, par), par)


@torch.no_grad()
def niqe_tensor(t: Tensor, rgb2bgr: bool = True, min_max: Sequence[float] = (0, 1), crop_border: int = 0, *,
                params=None) -> Tensor:
    """NIQE of a restored [1,3,H,W] or [3,H,W] device tensor by the reference's `use_image` route: tensor2img (the
    device quantiser of imgout: clamp to min_max, * 255, round half to even, BGR bytes) and then calculate_niqe."""
    from ..imgout import _as_chw, _min_max, _quantize
    if not torch.is_tensor(t) or not t.is_cuda:
        raise TypeError("niqe_tensor expects a tensor on the GPU")
    lo, hi = _min_max(min_max)
    chw, n_dim = _as_chw(t)
    if n_dim != 3 or chw.shape[0] != 3:
        raise ValueError(f"niqe_tensor expects [1,3,H,W] or [3,H,W], got {tuple(t.shape)}")
    return calculate_niqe(_quantize(chw, lo, hi, bool(rgb2bgr)), crop_border, "HWC", "y", params=params)


def register_niqe_metric(type_name: str = "niqe", **defaults) -> None:
    """Opt in: make `type: <type_name>` available to validation.Validator as fn(pred, gt, crop_border=0, params=None) =
    niqe_tensor(pred, crop_border=crop_border, params=params); gt is ignored.  `defaults` pre-set crop_border /
    params.  Nothing is registered unless this is called."""
    from ..validation import register_metric
    extra = set(defaults) - {"crop_border", "params"}
    if extra:
        raise TypeError(f"register_niqe_metric takes the defaults crop_border and params, got {sorted(extra)}")

    def fn(pred, gt, crop_border=defaults.get("crop_border", 0), params=defaults.get("params")):
        return niqe_tensor(pred, crop_border=crop_border, params=params)

    register_metric(type_name, fn)
