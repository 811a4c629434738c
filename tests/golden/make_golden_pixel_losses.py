"""Generate the pixel-loss fixture (pixel_losses.npz) by running the REFERENCE's basicsr/models/losses/losses.py and
loss_util.py on the cases of tests/pixel_loss_fixtures.py.

Test infrastructure only, as make_golden_niqe.py: the two reference files are loaded by path at run time, with
`basicsr.utils.registry` replaced by a stub whose LOSS_REGISTRY.register() returns the class unchanged; nothing of them
is stored but the numbers they produce.

Per elementwise case (L1Loss / MSELoss / CharbonnierLoss x reduction x weight form, loss_weight != 1) the file holds
  <name>_v64   the reference's value evaluated in float64 (every input cast to double): a scalar, or for reduction
               'none' the map at grad_index() positions
  <name>_v32   the reference's own float32 value (scalar cases)
  <name>_vbound  the relative value bound of the case: 1e-6, or twice the reference's own float32 distance from its
               float64 value where that is larger
  <name>_gp64  d/d pred in float64 at grad_index() positions, for the upstream gradient of the fixtures module
               (d/d target is asserted here to be its exact negative and is not stored)
  <name>_crc   checksum of the inputs
Per PSNRLoss case (the fp32 `coef` tensor cast to double, so that its fp32-rounded coefficients are kept): _v64, _v32,
_vbound (the absolute bound: 2e-6 |loss_weight| + 2e-7 |ref| without toY, 2e-5 |loss_weight| + 2e-7 |ref| with, or
twice the reference's own distance where larger), _gp64 at grad_index(), _crc; every image's MSE is asserted >= 1e-3.

Usage:  python tests/golden/make_golden_pixel_losses.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pixel_loss_fixtures as F  # noqa: E402


def load_reference_losses(ref: str):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def load(full, path):
        spec = importlib.util.spec_from_file_location(full, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[full] = m
        spec.loader.exec_module(m)
        return m

    class _Registry:
        def register(self):
            return lambda cls: cls

    base = os.path.join(ref, "NAFNet_base", "basicsr", "models", "losses")
    for name in ("basicsr", "basicsr.utils", "basicsr.models", "basicsr.models.losses"):
        stub(name)
    stub("basicsr.utils.registry", LOSS_REGISTRY=_Registry())
    load("basicsr.models.losses.loss_util", os.path.join(base, "loss_util.py"))
    return load("basicsr.models.losses.losses", os.path.join(base, "losses.py"))


def t(a, dtype, grad=False):
    if a is None:
        return None
    x = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return x.requires_grad_(grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    L = load_reference_losses(args.ref)
    classes = {"l1": L.L1Loss, "mse": L.MSELoss, "charbonnier": L.CharbonnierLoss}
    out = {}

    for name, sk, kind, red, wm in F.elementwise_cases():
        shape = F.SHAPES[sk]
        pred, target = F.inputs(sk, shape)
        w = F.weight(sk, shape, wm)
        kw = {"eps": F.CHARBONNIER_EPS} if kind == "charbonnier" else {}
        mod = classes[kind](loss_weight=F.LOSS_WEIGHT[kind], reduction=red, **kw)
        p, g = t(pred, torch.float64, True), t(target, torch.float64, True)
        v64 = mod(p, g, weight=t(w, torch.float64))
        up = t(F.upstream_map(name, shape), torch.float64) if red == "none" else torch.tensor(F.UPSTREAM_SCALAR,
                                                                                              dtype=torch.float64)
        v64.backward(gradient=up)
        assert torch.equal(p.grad, -g.grad), name
        with torch.no_grad():
            v32 = mod(t(pred, torch.float32), t(target, torch.float32), weight=t(w, torch.float32))
        idx = F.grad_index(pred.size)
        v64n, v32n = v64.detach().numpy(), v32.numpy().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            own = np.abs(v32n - v64n) / np.abs(v64n)
        own = float(np.nanmax(np.where(v64n == v32n, 0.0, own)))
        out[f"{name}_v64"] = v64n.reshape(-1)[idx] if red == "none" else v64n
        if red != "none":
            out[f"{name}_v32"] = v32.numpy()
        out[f"{name}_vbound"] = np.asarray(max(1e-6, 2.0 * own), dtype=np.float64)
        out[f"{name}_gp64"] = p.grad.numpy().reshape(-1)[idx]
        out[f"{name}_crc"] = np.asarray(F.checksum(pred, target, w), dtype=np.int64)
        if own > 0.5e-6:
            print(f"{name}: the reference's own fp32 value is {own:.3e} (relative) from its float64 value")

    for name, sk, toY in F.psnr_cases():
        shape = F.PSNR_SHAPES[sk]
        pred, target = F.psnr_inputs(sk, shape)
        lw = F.PSNR_LOSS_WEIGHT
        m64 = L.PSNRLoss(loss_weight=lw, toY=toY)
        m64.coef = m64.coef.double()  # the fp32-rounded coefficients, as doubles
        m64.first = False
        p, g = t(pred, torch.float64, True), t(target, torch.float64, True)
        v64 = m64(p, g)
        v64.backward(gradient=torch.tensor(F.UPSTREAM_SCALAR, dtype=torch.float64))
        assert torch.equal(p.grad, -g.grad), name
        with torch.no_grad():
            pp, gg = p.detach(), g.detach()
            if toY:
                pp = ((pp * m64.coef).sum(dim=1, keepdim=True) + 16.0) / 255.0
                gg = ((gg * m64.coef).sum(dim=1, keepdim=True) + 16.0) / 255.0
            mse = ((pp - gg) ** 2).mean(dim=(1, 2, 3))
            assert float(mse.min()) >= 1e-3, (name, mse)
            v32 = L.PSNRLoss(loss_weight=lw, toY=toY)(t(pred, torch.float32), t(target, torch.float32))
        ref = float(v64.detach())
        own = abs(float(v32) - ref)
        bound = (2e-5 if toY else 2e-6) * abs(lw) + 2e-7 * abs(ref)
        idx = F.grad_index(pred.size)
        out[f"{name}_v64"] = np.asarray(ref, dtype=np.float64)
        out[f"{name}_v32"] = v32.numpy()
        out[f"{name}_vbound"] = np.asarray(max(bound, 2.0 * own), dtype=np.float64)
        out[f"{name}_gp64"] = p.grad.numpy().reshape(-1)[idx]
        out[f"{name}_crc"] = np.asarray(F.checksum(pred, target), dtype=np.int64)
        print(f"{name}: value {ref:.9f}, min image MSE {float(mse.min()):.3e}, own fp32 distance {own:.2e} "
              f"(bound {bound:.2e})")

    path = os.path.join(HERE, "pixel_losses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
