"""Device time of the image-domain PSNR / SSIM (metrics/psnr_ssim.py, psnr_ssim.hip) beside the reference's algorithm
composed from torch ops on the same GPU.  One process, HIP events, medians after warm-up.  Run it under `timeout`.

Shapes: 16 uint8 HWC frames of 256 x 256 x 3, one call per frame (the time printed is per frame), and one frame of
2848 x 4256 x 3 (the uncropped SID frame).  Per shape: calculate_psnr and the three maps of calculate_ssim (3-D, valid,
Y) as called from Python, allocations included.

The composition is what the reference computes, on the device: PSNR from float64 tensor ops; the valid and Y maps from
five float64 F.conv2d with the 11 x 11 window (after a replicate pad for Y, whose plane comes from tensor ops); the
3-D map from five float32 F.conv3d with the 11 x 11 x 11 window after a replicate pad of 5 on all three axes.  It runs
at 256 x 256 first, then at 512 x 512, then at the full frame; a shape the library declines (or that does not fit) is
recorded as such and not tried again, and the 512 x 512 figures stand in for it.  Nothing here is a threshold.

    timeout 600 python scripts/psnr_ssim_time.py [--iters 7] [--reps 3] [--no-full-composition]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lowlight_image_enhancement_amd.metrics import psnr_ssim as ps  # noqa: E402

MODES = ("psnr", "ssim3d", "ssim_valid", "ssim_y")


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


def frame_pair(H, W, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.rand(1, 3, max(H // 16, 2), max(W // 16, 2), device=dev, generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    a = (x + 0.02 * torch.randn(1, 3, H, W, device=dev, generator=g)).clamp(0.0, 1.0)
    b = (a + 0.03 * torch.randn(1, 3, H, W, device=dev, generator=g)).clamp(0.0, 1.0)
    q = lambda t: (t[0] * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous()  # noqa: E731
    return q(a), q(b)


def ours(mode, a, b):
    """a, b: uint8 HWC device views; the public functions take tensors as CHW, so the view is permuted (no copy)"""
    a, b = a.permute(2, 0, 1), b.permute(2, 0, 1)
    if mode == "psnr":
        return ps.calculate_psnr(a, b, 0)
    return ps.calculate_ssim(a, b, 0, test_y_channel=mode == "ssim_y", ssim3d=mode == "ssim3d")


# ---------------------------------------------------------------------------------------------- the composition
def _ssim_map(mu1, mu2, e11, e22, e12, max_value):
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    return (((2 * mu1_mu2 + c1) * (2 * (e12 - mu1_mu2) + c2)) /
            ((mu1_sq + mu2_sq + c1) * ((e11 - mu1_sq) + (e22 - mu2_sq) + c2))).mean()


def _y_plane(x64):
    v = (x64.float() / 255.0).double()
    d = v[..., 0] * 24.966 + v[..., 1] * 128.553 + v[..., 2] * 65.481 + 16.0
    return ((d / 255.0).float() * 255.0).double()


def composed(mode, a, b, win):
    """the reference's algorithm from torch ops; a, b: uint8 HWC on the device"""
    a64, b64 = a.double(), b.double()
    if mode == "psnr":
        mse = ((a64 - b64) ** 2).mean()
        max_value = torch.where(a64.max() <= 1, 1.0, 255.0)
        return 20.0 * torch.log10(max_value / torch.sqrt(mse))
    if mode == "ssim3d":
        w3 = (win[:, None, None] * win[None, :, None] * win[None, None, :]).float()[None, None]
        x, y = a.float()[None, None], b.float()[None, None]  # [1,1,H,W,C]
        f = lambda t: F.conv3d(F.pad(t, (5, 5, 5, 5, 5, 5), mode="replicate"), w3)  # noqa: E731
        return _ssim_map(f(x), f(y), f(x * x), f(y * y), f(x * y), 255.0).double()
    w2 = (win[:, None] * win[None, :])[None, None]
    if mode == "ssim_y":
        x, y = _y_plane(a64)[None, None], _y_plane(b64)[None, None]
        f = lambda t: F.conv2d(F.pad(t, (5, 5, 5, 5), mode="replicate"), w2)  # noqa: E731
    else:
        x, y = a64.permute(2, 0, 1)[:, None], b64.permute(2, 0, 1)[:, None]  # [C,1,H,W]
        f = lambda t: F.conv2d(t, w2)  # noqa: E731  (the valid region is what [5:-5, 5:-5] keeps)
    return _ssim_map(f(x), f(y), f(x * x), f(y * y), f(x * y), 255.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-full-composition", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    win = torch.from_numpy(ps.gaussian_window()).to(dev)
    t_ours = {}

    small = [frame_pair(256, 256, dev, s) for s in range(16)]
    full = frame_pair(2848, 4256, dev, 99)
    mid = frame_pair(512, 512, dev, 98)
    for label, frames in (("16 x 256 x 256 x 3", small), ("1 x 512 x 512 x 3", [mid]), ("1 x 2848 x 4256 x 3", [full])):
        print(f"{label} uint8 HWC, this project (per frame, from Python with its allocations):", flush=True)
        for mode in MODES:
            t = time_one(lambda: [ours(mode, a, b) for a, b in frames], args.reps, args.iters) / len(frames)
            t_ours[(label, mode)] = t
            print(f"  {mode:10s} {t * 1e3:10.1f} us   value {float(ours(mode, *frames[0]).cpu()):.6f}", flush=True)

    plans = [("16 x 256 x 256 x 3", small), ("1 x 512 x 512 x 3", [mid])]
    if not args.no_full_composition:
        plans.append(("1 x 2848 x 4256 x 3", [full]))
    for label, frames in plans:
        print(f"{label}, the reference's algorithm composed from torch ops (per frame):", flush=True)
        for mode in MODES:
            try:
                t = time_one(lambda: [composed(mode, a, b, win) for a, b in frames], args.reps,
                             max(3, args.iters // 2), warmup=1) / len(frames)
                v = float(composed(mode, *frames[0], win).cpu())
            except RuntimeError as e:  # out of memory, or the convolution library declines the shape: not retried
                print(f"  {mode:10s} could not run: {str(e).splitlines()[0][:160]}", flush=True)
                torch.cuda.empty_cache()
                continue
            print(f"  {mode:10s} {t * 1e3:10.1f} us   value {v:.6f}   this project is "
                  f"{t / t_ours[(label, mode)]:.1f} x faster", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
