"""Device time of the pixel_opt losses' fused value + gradient launch (nbp_pixel_loss / nbp_psnr_loss with want_grad)
beside the torch composition of the reference's formula (forward and autograd backward, what optimize_parameters runs),
on the same device in the same process.  HIP events, medians after warm-up.  Run it under `timeout`.

  * L1Loss / MSELoss / CharbonnierLoss ('mean', no weight) and PSNRLoss (toY false and true): value and d/d pred;
  * the cfg2 loss head (16 x 3 x 256 x 256): the pixel term as NBPTrainer(pixel_loss=L1Loss()) launches it (one
    nbp_pixel_loss call: the fused kernel and its one-work-group finish) against the w_l1 head of the trainer without a
    pixel loss (nbp_pix_loss_fwd + nbp_pix_loss_bwd: two passes over out and gt and a finish), windows alternated.

Sizes: 16x3x256x256 and 1x3x2848x4256 (the uncropped SID frame).  Nothing here is a threshold.

    timeout 900 python scripts/pixel_loss_time.py [--sizes 16x256x256,1x2848x4256] [--iters 7]
"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lowlight_image_enhancement_amd._lib import call, query  # noqa: E402
from lowlight_image_enhancement_amd.pixel_losses import (CharbonnierLoss, L1Loss, MSELoss, PSNRLoss,  # noqa: E402
                                                         fused_value_and_grad)


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def time_one(fn, reps, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, reps) for _ in range(iters))


def time_pair(fa, fb, reps, iters, warmup=3):
    """medians of two functions whose windows alternate (a, b, a, b, ...), and the spread (min, max) of each"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(iters):
        ta.append(window_ms(fa, reps))
        tb.append(window_ms(fb, reps))
    return statistics.median(ta), statistics.median(tb), (min(ta), max(ta)), (min(tb), max(tb))


def torch_loss(mod, p, t):
    """the reference's formula in torch ops"""
    if isinstance(mod, PSNRLoss):
        if mod.toY:
            coef = mod.coef.to(p.device)
            p = ((p * coef).sum(dim=1).unsqueeze(dim=1) + 16.0) / 255.0
            t = ((t * coef).sum(dim=1).unsqueeze(dim=1) + 16.0) / 255.0
        return mod.loss_weight * mod.scale * torch.log(((p - t) ** 2).mean(dim=(1, 2, 3)) + 1e-8).mean()
    d = p - t
    e = d.abs() if mod.kind == "l1" else (d * d if mod.kind == "mse" else torch.sqrt(d * d + mod.eps))
    return mod.loss_weight * e.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16x256x256,1x2848x4256")
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for size in args.sizes.split(","):
        N, H, W = (int(v) for v in size.split("x"))
        n = N * 3 * H * W
        reps = 3 if n > 12 << 20 else 20
        g = torch.Generator(device=dev).manual_seed(N + H)
        p = torch.rand(N, 3, H, W, device=dev, generator=g)
        t = (p + 0.05 * torch.randn(N, 3, H, W, device=dev, generator=g)).clamp(0.0, 1.0)
        up = torch.ones(1, device=dev)
        value = torch.zeros(1, device=dev)
        grad = torch.empty_like(p)
        for label, mod in (("L1Loss", L1Loss()), ("MSELoss", MSELoss()), ("CharbonnierLoss", CharbonnierLoss()),
                           ("PSNRLoss", PSNRLoss()), ("PSNRLoss(toY)", PSNRLoss(toY=True))):
            pr = p.clone().requires_grad_(True)

            def torch_step():
                pr.grad = None
                torch_loss(mod, pr, t).backward()

            t_k = time_one(lambda: fused_value_and_grad(mod, p, t, up, value, grad), reps, args.iters)
            t_t = time_one(torch_step, reps, args.iters)
            fused_value_and_grad(mod, p, t, up, value, grad)
            torch_step()
            dv = abs(value.item() - torch_loss(mod, p, t).item())
            dg = ((grad - pr.grad).norm() / pr.grad.norm()).item()
            # bytes the algorithm needs: read pred and target, write the gradient (PSNRLoss reads both twice)
            need = (5 if isinstance(mod, PSNRLoss) else 3) * 4 * n
            print(f"{N}x3x{H}x{W} {label:16s} value+grad: HIP {t_k * 1e3:9.1f} us ({need / t_k / 1e6:.0f} GB/s over "
                  f"{need // n} B per element), torch composition {t_t * 1e3:9.1f} us, ratio {t_t / t_k:.2f}x; "
                  f"|value difference| {dv:.2e}, gradient norm-wise difference {dg:.2e}", flush=True)
            del pr
        if (N, H, W) == (16, 256, 256):
            mod = L1Loss()
            old_v = torch.zeros(1, device=dev)
            old_g = torch.empty_like(p)

            def old_head():
                ws = torch.empty(query("pix_workspace_doubles", n), dtype=torch.float64, device=dev)  # as the trainer
                call("pix_loss_fwd", p, t, n, 0, 0.0, 0, 0, ws, old_v)
                call("pix_loss_bwd", p, t, n, 0, 0.0, 0, 0, up, old_g)

            t_new, t_old, s_new, s_old = time_pair(lambda: fused_value_and_grad(mod, p, t, up, value, grad), old_head,
                                                   reps, args.iters)
            same = torch.equal(grad, old_g)
            print(f"cfg2 loss head, pixel term (16x3x256x256): nbp_pixel_loss (fused) {t_new * 1e3:.1f} us "
                  f"[{s_new[0] * 1e3:.1f}, {s_new[1] * 1e3:.1f}], nbp_pix_loss_fwd + nbp_pix_loss_bwd {t_old * 1e3:.1f} us "
                  f"[{s_old[0] * 1e3:.1f}, {s_old[1] * 1e3:.1f}], old / new {t_old / t_new:.2f}x; values "
                  f"{value.item():.9g} / {old_v.item():.9g}, gradients bitwise equal: {same}", flush=True)
        del p, t, grad
        torch.cuda.empty_cache()
    assert math.isfinite(value.item())
    return 0


if __name__ == "__main__":
    sys.exit(main())
