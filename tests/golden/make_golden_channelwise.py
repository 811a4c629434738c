"""Generate the channel-wise metric fixture (channelwise.npz) by running the REFERENCE's metrics/channelwise.py on the CPU.

Test infrastructure only, as make_golden_niqe.py: the reference's metrics/linear.py and metrics/channelwise.py are
loaded by path at run time behind a stub package; nothing of them is stored but the numbers they produce.

The file holds the inputs (float32) and, per call, the reference's outputs under the key `<case>__<call>` (dict results
as `<...>__R`, `__G`, `__B`, `__mean`):

  A  [2,3,24,20] in [0,1], noise of a different strength per channel   every reduction, a custom eps, rgb_ssim at
                                                                       kernel 11 / reflect, 7 / replicate, uniform 5,
                                                                       both channel_aggregate values
  B  [1,3,13,11] (a plane of 143 elements: misaligned planes, a tail)  4-D and 3-D
  C  a 0-255 pair, data_range=255                                      no clamp, clamp=True (-> [0, 1]), clamp=200.0
  D  [1,3,13,11] in [-0.3, 1.3]                                        clamp=True and no clamp
  A against itself                                                     10 log10(range^2 / eps), no inf

Usage:  python tests/golden/make_golden_channelwise.py --ref <checkout of the reference>
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

SSIM_CALLS = {
    "k11_reflect": dict(kernel_size=11, padding="reflect"),
    "k7_replicate": dict(kernel_size=7, padding="replicate"),
    "k5_uniform": dict(kernel_size=5, gaussian=False),
}


def load_reference(ref: str):
    pkg = types.ModuleType("refmetrics")
    pkg.__path__ = []
    sys.modules["refmetrics"] = pkg

    def load(name):
        spec = importlib.util.spec_from_file_location(f"refmetrics.{name}", os.path.join(ref, "metrics", f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"refmetrics.{name}"] = m
        spec.loader.exec_module(m)
        return m

    load("linear")
    return load("channelwise")


def inputs():
    g = torch.Generator().manual_seed(20)
    a_t = torch.rand(2, 3, 24, 20, generator=g)
    noise = torch.randn(2, 3, 24, 20, generator=g) * torch.tensor([0.02, 0.05, 0.1]).view(1, 3, 1, 1)
    a_p = (a_t + noise).clamp(0.0, 1.0)
    b_t = torch.rand(1, 3, 13, 11, generator=g)
    b_p = (b_t + 0.03 * torch.randn(1, 3, 13, 11, generator=g)).clamp(0.0, 1.0)
    c_t = torch.round(torch.rand(2, 3, 24, 20, generator=g) * 255.0)
    c_p = (c_t + 6.0 * torch.randn(2, 3, 24, 20, generator=g)).clamp(0.0, 255.0)
    d_t = torch.rand(1, 3, 13, 11, generator=g) * 1.6 - 0.3
    d_p = d_t + 0.08 * torch.randn(1, 3, 13, 11, generator=g)
    return {"A": (a_p, a_t), "B": (b_p, b_t), "C": (c_p, c_t), "D": (d_p, d_t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (its metrics/ is loaded by path)")
    args = ap.parse_args()
    cw = load_reference(args.ref)
    data = inputs()
    out = {}
    for name, (p, t) in data.items():
        out[f"{name}_pred"], out[f"{name}_tgt"] = p.numpy(), t.numpy()

    def put(key, res):
        if isinstance(res, dict):
            for k, v in res.items():
                if k != "meta":
                    out[f"{key}__{k}"] = v.numpy()
        else:
            out[key] = res.numpy()

    ap_, at_ = data["A"]
    for red in ("none", "mean", "sum"):
        put(f"A__psnr_{red}", cw.rgb_psnr(ap_, at_, reduction=red))
        put(f"A__cpsnr_{red}", cw.cpsnr_rgb(ap_, at_, reduction=red))
    put("A__psnr_eps1e-3", cw.rgb_psnr(ap_, at_, reduction="none", eps=1e-3))
    put("A__cpsnr_eps1e-2", cw.cpsnr_rgb(ap_, at_, reduction="none", eps=1e-2))
    put("A__psnr_same", cw.rgb_psnr(ap_, ap_.clone(), reduction="none"))
    put("A__cpsnr_same", cw.cpsnr_rgb(ap_, ap_.clone(), reduction="none"))
    bp, bt = data["B"]
    put("B__psnr_none", cw.rgb_psnr(bp, bt, reduction="none"))
    put("B__cpsnr_none", cw.cpsnr_rgb(bp, bt, reduction="none"))
    put("B__psnr_3d", cw.rgb_psnr(bp[0], bt[0]))
    put("B__cpsnr_3d", cw.cpsnr_rgb(bp[0], bt[0]))
    cp, ct = data["C"]
    for tag, clamp in (("noclamp", False), ("clampTrue", True), ("clamp200", 200.0)):
        put(f"C__psnr_{tag}", cw.rgb_psnr(cp, ct, data_range=255.0, reduction="none", clamp=clamp))
        put(f"C__cpsnr_{tag}", cw.cpsnr_rgb(cp, ct, data_range=255.0, reduction="none", clamp=clamp))
    dp, dt = data["D"]
    for tag, clamp in (("noclamp", False), ("clampTrue", True)):
        put(f"D__psnr_{tag}", cw.rgb_psnr(dp, dt, reduction="none", clamp=clamp))
        put(f"D__cpsnr_{tag}", cw.cpsnr_rgb(dp, dt, reduction="none", clamp=clamp))
    for tag, kw in SSIM_CALLS.items():
        for agg in ("none", "mean"):
            for red in ("none", "mean", "sum"):
                put(f"A__ssim_{tag}_{agg}_{red}", cw.rgb_ssim(ap_, at_, reduction=red, channel_aggregate=agg, **kw))
    put("B__ssim_3d", cw.rgb_ssim(bp[0], bt[0], kernel_size=7))
    path = os.path.join(HERE, "channelwise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    print("A psnr none:", {k: out[f"A__psnr_none__{k}"] for k in "RGB"}, "same:", out["A__psnr_same__R"])


if __name__ == "__main__":
    main()
