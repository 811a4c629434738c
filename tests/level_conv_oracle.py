"""Float64 oracle of the two level-change convolutions of NAFNet, with a derived per-element rounding bound.

Test infrastructure only; pure torch, imports on the CPU.

The operations, on reference-layout tensors (NCHW activations, [2C, C, 2, 2] and [2C', C', 1, 1] weights), are the
reference's own modules (NAFNet_arch.py:106-122, 148-149):

* down: F.conv2d(x, W, b, stride=2)
* up:   F.pixel_shuffle(F.conv2d(x, W), 2) + skip
* dx, dW, db and (up) dskip: torch autograd on those.

Two forms of the same oracle:

* the conv form (down_conv / up_conv): torch's conv2d / pixel_shuffle / autograd in float64.  This is the definition.
* the matmul form (down_mm / up_mm and the per-quantity functions they are made of): reshape + matmul in float64 on
  the reference layout, for shapes where a float64 conv2d is too slow; it also returns `mag`, the same contraction on
  absolute values (plus |bias| / |skip|), which the bound needs.  tests/test_level_conv_oracle_host.py pins this form to
  the conv form at 1e-12 relative.

Layout conversion goes through the package: weights through NAFNet._to_internal / _to_reference (kinds "down" and
"up"), activations through the package's NCHW <-> NHWC convention (NHWC = NCHW.permute(0, 2, 3, 1), contiguous).

The bound.  All operands are rounded to the storage type before the oracle sees them, so the oracle is the exact result
on the operands the kernel reads.  With u the storage type's unit roundoff (2^-8 bf16, 2^-11 fp16, 2^-24 fp32), mag the
contraction on absolute values plus |bias| and |R|, and Kc the contraction length,

    s     = 2 (Kc + 2) 2^-24 mag       worst-case fp32 accumulation error in any order of the Kc products plus the
                                       bias and residual adds; doubled because the MFMA's internal rounding mode is not
                                       specified
    bound = u |ref| + (1 + u) s        (+ 2^-25 absolute for fp16: half its subnormal spacing)

The kernel's fp32 value v obeys |v - ref| <= s; one rounding to the storage type adds at most u |v| <= u (|ref| + s).
A correct kernel cannot exceed this bound at any element.
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(_HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(_HERE))

STORAGE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTYPE_CODE = {"fp32": 0, "bf16": 1, "fp16": 2}  # the C-ABI's dtype codes
UNIT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}

# (B, gh, gw, cs): gh x gw the low-resolution grid, cs the channels of the high-resolution map.  The down layer takes
# [B, cs, 2gh, 2gw] to [B, 2cs, gh, gw]; the up layer takes [B, 2cs, gh, gw] (+ skip) to [B, cs, 2gh, 2gw].
# All have gh != gw and B >= 2; cs 24: K tail, N % 64 != 0, ragged M.
SMALL_SHAPES = {"s8": (3, 5, 7, 8), "s16": (3, 5, 7, 16), "s24": (2, 9, 6, 24), "s64": (2, 7, 11, 64),
                "s128": (3, 5, 7, 128)}


# ------------------------------------------------------------------------------------------------ layouts
def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2).contiguous()


def entry(kind: str, ref_shape) -> SimpleNamespace:
    """A stand-in for the PEntry of a down / up weight: what _to_internal / _to_reference read of it."""
    return SimpleNamespace(kind=kind, ref_shape=tuple(ref_shape))


def to_internal(kind: str, w_ref: torch.Tensor) -> torch.Tensor:
    """Reference-layout weight -> the flat internal layout the kernels read (NAFNet._to_internal)."""
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    return NAFNet._to_internal(None, entry(kind, w_ref.shape), w_ref).contiguous()


def to_reference(kind: str, ref_shape, flat: torch.Tensor) -> torch.Tensor:
    """Flat internal-layout weight (gradient) -> the reference layout (NAFNet._to_reference)."""
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    return NAFNet._to_reference(None, entry(kind, ref_shape), flat)


# ------------------------------------------------------------------------------------------------ inputs
_NAMES = ("down_x", "down_w", "down_b", "down_dy", "down_res", "up_x", "up_w", "up_skip", "up_dy")


class Inputs:
    """The operands of one case, reference layout, already rounded to the storage type (held in it; .double() is
    exact).  Each tensor has its own seed, so a test may ask for any subset.  The down bias is fp32 on the device
    whatever the storage type, and is rounded to fp32."""

    def __init__(self, B: int, gh: int, gw: int, cs: int, prec: str, seed: int, device="cpu"):
        self.B, self.gh, self.gw, self.cs, self.prec, self.seed, self.device = B, gh, gw, cs, prec, seed, device
        c, B2 = cs, B
        self.shapes = {"down_x": (B2, c, 2 * gh, 2 * gw), "down_w": (2 * c, c, 2, 2), "down_b": (2 * c,),
                       "down_dy": (B2, 2 * c, gh, gw), "down_res": (B2, c, 2 * gh, 2 * gw),
                       "up_x": (B2, 2 * c, gh, gw), "up_w": (4 * c, 2 * c, 1, 1), "up_skip": (B2, c, 2 * gh, 2 * gw),
                       "up_dy": (B2, c, 2 * gh, 2 * gw)}
        self._cache: Dict[str, torch.Tensor] = {}

    def __getitem__(self, name: str) -> torch.Tensor:
        if name not in self._cache:
            shp = self.shapes[name]
            gen = torch.Generator(device=self.device).manual_seed(self.seed * 16 + _NAMES.index(name))
            t = torch.randn(shp, device=self.device, generator=gen)
            if name.endswith("_w"):
                t = t / float(shp[1] * shp[2] * shp[3]) ** 0.5  # fan_in
            self._cache[name] = t if name == "down_b" else t.to(STORAGE[self.prec])
        return self._cache[name]

    def f64(self, name: str) -> torch.Tensor:
        return self[name].double()


# ------------------------------------------------------------------------------------------------ conv form
def down_conv(x, W, b, dy) -> Dict[str, torch.Tensor]:
    x, W, b = (t.detach().clone().requires_grad_(True) for t in (x, W, b))
    out = F.conv2d(x, W, b, stride=2)
    dx, dW, db = torch.autograd.grad(out, (x, W, b), dy)
    return {"out": out.detach(), "dx": dx, "dW": dW, "db": db}


def up_conv(x, W, skip, dy) -> Dict[str, torch.Tensor]:
    x, W, skip = (t.detach().clone().requires_grad_(True) for t in (x, W, skip))
    out = F.pixel_shuffle(F.conv2d(x, W), 2) + skip
    dx, dW, dskip = torch.autograd.grad(out, (x, W, skip), dy)
    return {"out": out.detach(), "dx": dx, "dW": dW, "dskip": dskip}


# ------------------------------------------------------------------------------------------------ matmul form
def _patches(x):
    """[B, C, 2h, 2w] -> [B h w, C*4]: the 2x2 / stride-2 patches, columns in the order of W.reshape(O, -1)."""
    B, C, H, Wd = x.shape
    return x.reshape(B, C, H // 2, 2, Wd // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(-1, C * 4)


def _unpatch(p, B, C, h, w):
    """The adjoint (and inverse) of _patches: [B h w, C*4] -> [B, C, 2h, 2w]."""
    return p.reshape(B, h, w, C, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, C, 2 * h, 2 * w)


def _rows(x):
    """[B, C, h, w] -> [B h w, C]"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _unrows(r, B, h, w):
    return r.reshape(B, h, w, -1).permute(0, 3, 1, 2)


def down_out_mm(x, W, b) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, mag) of the down conv"""
    B, C, H, Wd = x.shape
    Wm, P = W.reshape(W.shape[0], -1), _patches(x)
    out = P @ Wm.t() + b
    mag = P.abs() @ Wm.abs().t() + b.abs()
    return _unrows(out, B, H // 2, Wd // 2), _unrows(mag, B, H // 2, Wd // 2)


def down_dx_mm(dy, W) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx, mag) of the down conv's input gradient"""
    B, O, h, w = dy.shape
    Wm, G = W.reshape(O, -1), _rows(dy)
    C = W.shape[1]
    return _unpatch(G @ Wm, B, C, h, w), _unpatch(G.abs() @ Wm.abs(), B, C, h, w)


def down_dw_mm(x, dy, w_shape) -> Tuple[torch.Tensor, torch.Tensor]:
    G = _rows(dy)
    return (G.t() @ _patches(x)).reshape(w_shape), G.sum(0)


def up_out_mm(x, W, skip) -> Tuple[torch.Tensor, torch.Tensor]:
    """(out, mag) of the up conv + PixelShuffle(2) + skip; conv channel n = c*4 + r1*2 + r2 lands at (c, 2i+r1, 2j+r2)
    (torch.nn.PixelShuffle's definition) -- the adjoint of _patches on the conv output."""
    B, C, h, w = x.shape
    Wm, X = W.reshape(W.shape[0], -1), _rows(x)
    out = _unpatch(X @ Wm.t(), B, W.shape[0] // 4, h, w) + skip
    mag = _unpatch(X.abs() @ Wm.abs().t(), B, W.shape[0] // 4, h, w) + skip.abs()
    return out, mag


def up_dx_mm(dy, W) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx, mag) of the up conv's input gradient"""
    B, _, H, Wd = dy.shape
    Wm, G = W.reshape(W.shape[0], -1), _patches(dy)
    return _unrows(G @ Wm, B, H // 2, Wd // 2), _unrows(G.abs() @ Wm.abs(), B, H // 2, Wd // 2)


def up_dw_mm(x, dy, w_shape) -> torch.Tensor:
    return (_patches(dy).t() @ _rows(x)).reshape(w_shape)


def down_mm(x, W, b, dy) -> Dict[str, torch.Tensor]:
    out, mag_out = down_out_mm(x, W, b)
    dx, mag_dx = down_dx_mm(dy, W)
    dW, db = down_dw_mm(x, dy, W.shape)
    return {"out": out, "dx": dx, "dW": dW, "db": db, "mag_out": mag_out, "mag_dx": mag_dx}


def up_mm(x, W, skip, dy) -> Dict[str, torch.Tensor]:
    out, mag_out = up_out_mm(x, W, skip)
    dx, mag_dx = up_dx_mm(dy, W)
    return {"out": out, "dx": dx, "dW": up_dw_mm(x, dy, W.shape), "dskip": dy.clone(), "mag_out": mag_out,
            "mag_dx": mag_dx}


# ------------------------------------------------------------------------------------------------ the bound
def bound(ref: torch.Tensor, mag: torch.Tensor, kc: int, prec: str) -> torch.Tensor:
    u = UNIT[prec]
    s = 2.0 * (kc + 2) * 2.0 ** -24 * mag
    b = u * ref.abs() + (1.0 + u) * s
    if prec == "fp16":
        b = b + 2.0 ** -25
    return b


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor) -> float:
    """max |got - ref| / bound over all elements; inf if anything is not finite."""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bnd).max())


def share_outside(got: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor) -> float:
    return float(((got - ref).abs() > bnd).double().mean())
