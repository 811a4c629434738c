"""Device NIQE time (metrics/niqe.py, niqe.hip): one uint8 HWC frame of 2848 x 4256 (the uncropped SID frame, 1276
blocks) and of 480 x 672 (35 blocks, the size of the fixture's largest case).  One process, HIP events, medians after
warm-up.  Run it under `timeout`.

Per frame size it prints each launch group on its own (nbp_niqe_luma; nbp_niqe_features = the half-size plane and
the two block-feature launches; nbp_niqe_score) and the whole of calculate_niqe as called from Python.  Beside them
it sets the reference's CPU seconds stored in tests/golden/niqe.npz: that is the reference's algorithm on the CPU of
the machine that generated the fixture, at the fixture's size (480 x 672) -- not a like-for-like full-frame time, and
not measured in this run.  Nothing here is a threshold.

The frames are the smooth fields of scripts/val_time.py, quantised to bytes.

    timeout 600 python scripts/niqe_time.py --params <niqe_pris_params.npz> [--sizes 2848x4256,480x672] [--iters 7]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lowlight_image_enhancement_amd._lib import call, query  # noqa: E402
from lowlight_image_enhancement_amd.metrics import niqe  # noqa: E402


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def time_one(fn, reps, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, reps) for _ in range(iters))


def frame_u8(H, W, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.rand(1, 3, max(H // 16, 2), max(W // 16, 2), device=dev, generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    x = (x + 0.02 * torch.randn(1, 3, H, W, device=dev, generator=g)).clamp(0.0, 1.0)
    return (x[0] * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default=os.environ.get(niqe.PARAMS_ENV) or
                    os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))
    ap.add_argument("--sizes", default="2848x4256,480x672")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    par = niqe._device_params(args.params, dev)
    tables = niqe._device_tables(dev)
    gold = os.path.join(ROOT, "tests", "golden", "niqe.npz")
    if os.path.exists(gold):
        g = np.load(gold)
        print(f"reference on the CPU (stored with the fixture, not measured here): {float(g['ref_cpu_seconds']):.3f} s for "
              f"{g['ref_cpu_case']} on {g['ref_cpu_label']}", flush=True)
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = frame_u8(H, W, dev, 1)
        nb = (H // 96) * (W // 96)
        Hc, Wc = H // 96 * 96, W // 96 * 96
        y = torch.empty(Hc, Wc, dtype=torch.float32, device=dev)
        ws = torch.empty(query("niqe_workspace_bytes", H, W), dtype=torch.uint8, device=dev)
        feat = torch.empty(nb, 36, dtype=torch.float64, device=dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)

        def luma():
            call("niqe_luma", img, 1, H, W, 3, img.stride(0), img.stride(1), img.stride(2), y)

        def features():
            call("niqe_features", y, H, W, par["window"], tables, ws, feat)

        def score():
            call("niqe_score", feat, nb, par["mu"], par["cov"], out)

        t_l = time_one(luma, args.reps, args.iters)
        t_f = time_one(features, args.reps, args.iters)
        t_s = time_one(score, args.reps, args.iters)
        t_all = time_one(lambda: niqe.calculate_niqe(img, 0, params=args.params), args.reps, args.iters)
        q = float(niqe.calculate_niqe(img, 0, params=args.params).cpu())
        print(f"{H} x {W} uint8 HWC, {nb} blocks ({2 * nb} work-groups), NIQE {q:.4f}", flush=True)
        print(f"  nbp_niqe_luma     {t_l * 1e3:9.1f} us  ({(3 * H * W + 4 * Hc * Wc) / t_l / 1e6:.0f} GB/s over 3 B read + "
              f"4 B written per pixel)", flush=True)
        print(f"  nbp_niqe_features {t_f * 1e3:9.1f} us  (3 launches: half-size plane, scale 1, scale 2; "
              f"{t_f * 1e3 / (2 * nb):.2f} us per work-group amortised)", flush=True)
        print(f"  nbp_niqe_score    {t_s * 1e3:9.1f} us  (one work-group)", flush=True)
        print(f"  calculate_niqe    {t_all * 1e3:9.1f} us  (from Python, with its allocations; the sum of the launches is "
              f"{(t_l + t_f + t_s) * 1e3:.1f} us)", flush=True)
        del img, y, ws, feat
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
