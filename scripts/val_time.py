"""Validation-pass statistics time (metrics/valstats.py, validation.Validator): one frame of 1424 x 2128 and of
2848 x 4256 (the uncropped SID frame), fp32.  One process, HIP events, medians after warm-up.  Run it under `timeout`.

The frames are smooth fields with a little noise (a low-resolution random image upsampled bilinearly, + 2 % noise), so
that the Sobel magnitudes crowd into few exponents as they do on photographs (the radix select's worst case for
LDS-atomic contention), not the flat spread of white noise.

Per frame size it prints
  * quantile_rows (nbp_quantile_select + lerp) against torch.quantile on the frame's Sobel-magnitude row, q = 0.85;
  * color_stats (nbp_val_color_maps + the select + nbp_masked_mean) against today's pair deltae2000_mean +
    edge_deltae2000_mean of metrics.lowlight_metrics;
  * Validator.update with the four weight-free metrics (linear_psnr, linear_ssim, deltae2000_mean,
    edge_deltae2000_mean) against the four float-returning wrappers;
  * nbp_quantile_select and nbp_val_color_maps on their own: time per call, algorithmic bytes (the select reads the row
    three times; the colour pass reads both images once and writes two maps) and the rate they give;
  * the one condition fixed in advance: each new path is not slower than the existing composition in this run.

A step is timed as `reps` back-to-back calls between two events, the windows of the two formulations alternating, median
of `--iters` such windows.

    timeout 900 python scripts/val_time.py [--sizes 1424x2128,2848x4256] [--iters 7] [--reps 5]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lowlight_image_enhancement_amd.metrics import lowlight_metrics as lm  # noqa: E402
from lowlight_image_enhancement_amd.metrics.valstats import (color_maps, color_stats, quantile_rank,  # noqa: E402
                                                             quantile_rows, quantile_select)
from lowlight_image_enhancement_amd.validation import Validator  # noqa: E402


def window_ms(fn, reps):
    """milliseconds per call of `reps` back-to-back calls between two events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def time_pair(a, b, reps, iters, warmup=2):
    """medians of a and b, their windows alternating"""
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(window_ms(a, reps))
        tb.append(window_ms(b, reps))
    return statistics.median(ta), statistics.median(tb)


def time_one(fn, reps, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, reps) for _ in range(iters))


def frame(H, W, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.rand(1, 3, max(H // 16, 2), max(W // 16, 2), device=dev, generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    return (x + 0.02 * torch.randn(1, 3, H, W, device=dev, generator=g)).clamp(0.0, 1.0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1424x2128,2848x4256")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ok = True
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        n = H * W
        pred, gt = frame(H, W, dev, 1), frame(H, W, dev, 2)
        print(f"1 x 3 x {H} x {W} ({n} pixels)", flush=True)

        def verdict(name, new, old):
            nonlocal ok
            good = new <= old
            ok = ok and good
            print(f"  {name}: new {new:.3f} ms, existing {old:.3f} ms ({old / new:.2f}x): "
                  f"{'pass (not slower)' if good else 'FAIL (slower)'}", flush=True)

        # ---- the quantile of a Sobel-magnitude row
        _, grad, _ = color_maps(pred, gt)
        row = grad.view(1, -1)
        k_lo, k_hi, _ = quantile_rank(n, 0.85)
        if n <= 2 ** 24:
            got, ref = quantile_rows(row, 0.85), torch.quantile(row, 0.85, dim=1)
            assert abs(got.item() - ref.item()) <= 2e-7 * abs(ref.item()), (got.item(), ref.item())
            t_new, t_old = time_pair(lambda: quantile_rows(row, 0.85), lambda: torch.quantile(row, 0.85, dim=1),
                                     args.reps, args.iters)
            verdict("quantile_rows against torch.quantile (q 0.85)", t_new, t_old)
        else:
            print("  torch.quantile refuses this size (more than 2^24 elements): no comparison", flush=True)
        t_sel = time_one(lambda: quantile_select(row, k_lo, k_hi), args.reps, args.iters)
        b_sel = 3 * n * 4
        print(f"  nbp_quantile_select: {t_sel * 1e3:.1f} us per call (6 launches + the clear), {b_sel / 1e6:.1f} MB -> "
              f"{b_sel / t_sel / 1e6:.0f} GB/s", flush=True)
        t_map = time_one(lambda: color_maps(pred, gt), args.reps, args.iters)
        b_map = (2 * 3 + 2) * n * 4
        print(f"  nbp_val_color_maps: {t_map * 1e3:.1f} us per call, {b_map / 1e6:.1f} MB -> "
              f"{b_map / t_map / 1e6:.0f} GB/s", flush=True)

        # ---- the two colour metrics of one frame
        def colour_old():
            return lm.deltae2000_mean(pred, gt), lm.edge_deltae2000_mean(pred, gt)

        st, old = color_stats(pred, gt), colour_old()
        assert abs(st["mean"].item() - old[0]) < 1e-4 and abs(st["edge_mean"].item() - old[1]) < 2e-3 * old[1], (st, old)
        verdict("color_stats against deltae2000_mean + edge_deltae2000_mean",
                *time_pair(lambda: color_stats(pred, gt), colour_old, args.reps, args.iters))

        # ---- one update of the pass, the four weight-free metrics
        val = Validator({"metrics": {"psnr": {"type": "linear_psnr"}, "ssim": {"type": "linear_ssim"},
                                     "de": {"type": "deltae2000_mean"}, "edge": {"type": "edge_deltae2000_mean"}}},
                        device=dev)

        def update_old():
            return (lm.linear_psnr(pred, gt), lm.linear_ssim(pred, gt), lm.deltae2000_mean(pred, gt),
                    lm.edge_deltae2000_mean(pred, gt))

        verdict("Validator.update (4 metrics) against the four wrappers",
                *time_pair(lambda: val.update(pred, gt), update_old, max(1, args.reps // 2), args.iters))
        del pred, gt, grad, row
        torch.cuda.empty_cache()
    print("each new path against the existing composition:", "not slower at every size" if ok else "SLOWER somewhere")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
