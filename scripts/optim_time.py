"""Device time of one optimizer apply launch per kind (nbp_adam_apply, nbp_sgd_apply) beside the existing
nbp_adamw_apply in the same process, and beside torch's own optimizer step (foreach and, where this torch has it, fused)
over one flat tensor on the same GPU.  HIP events around windows of launches, medians after warm-up.  Run it under
`timeout`.

Sizes: the parameter counts of the width-32 and width-64 networks of bench.py.  The achieved bytes/s counts the words
the update has to move per element: 7 for Adam / AdamW (read p, g, m, v; write p, m, v), 9 with amsgrad, 5 for SGD with
momentum (read p, g, buf; write p, buf), 3 without.  Nothing here is a threshold.

    timeout 900 python scripts/optim_time.py [--reps 100] [--iters 7]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lowlight_image_enhancement_amd._lib import call, query  # noqa: E402

BLK = dict(enc_blk_nums=[2, 2, 4, 8], middle_blk_num=12, dec_blk_nums=[2, 2, 2, 2])
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.01


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def time_one(fn, reps, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, reps) for _ in range(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    assert args.reps >= 50
    from lowlight_image_enhancement_amd.NewBP_model.newbp_net_arch import create_newbp_net
    dev = torch.device("cuda:0")
    for width in (32, 64):
        n = create_newbp_net(in_channels=3, width=width, **BLK).numel
        gen = torch.Generator(device=dev).manual_seed(width)
        p = torch.randn(n, device=dev, generator=gen)
        g = 1e-3 * torch.randn(n, device=dev, generator=gen)
        m, v, vmax, buf = (torch.zeros(n, device=dev) for _ in range(4))
        state = torch.zeros(8, device=dev)
        ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        lr = torch.full((1,), 1e-4, device=dev)
        ws = torch.empty(query("clip_workspace_doubles", n), dtype=torch.float64, device=dev)
        call("optim_prepare", g, n, 1.0, 0.01, ws, lr, B1, B2, state, ctl, None, None, None, 0)
        kinds = [
            ("nbp_adamw_apply (existing)", 7, lambda: call("adamw_apply", p, g, m, v, n, state, B1, B2, EPS, WD)),
            ("nbp_adam_apply AdamW", 7, lambda: call("adam_apply", p, g, m, v, None, n, state, B1, B2, EPS, WD, 1)),
            ("nbp_adam_apply Adam (L2)", 7, lambda: call("adam_apply", p, g, m, v, None, n, state, B1, B2, EPS, WD, 0)),
            ("nbp_adam_apply Adam amsgrad", 9,
             lambda: call("adam_apply", p, g, m, v, vmax, n, state, B1, B2, EPS, WD, 0)),
            ("nbp_sgd_apply momentum 0", 3, lambda: call("sgd_apply", p, g, None, n, state, ctl, 0.0, 0.0, WD, 0)),
            ("nbp_sgd_apply momentum 0.9", 5, lambda: call("sgd_apply", p, g, buf, n, state, ctl, 0.9, 0.0, WD, 0)),
            ("nbp_sgd_apply nesterov", 5, lambda: call("sgd_apply", p, g, buf, n, state, ctl, 0.9, 0.0, WD, 1)),
        ]
        print(f"width {width}: numel {n}", flush=True)
        for label, words, fn in kinds:
            t = time_one(fn, args.reps, args.iters)
            print(f"  {label:30s} {t * 1e3:8.1f} us  {words * 4 * n / t / 1e9:7.2f} TB/s over {words} words per "
                  f"element", flush=True)
        # torch's own optimizers over the same flat tensor (host-side step() included: what a torch trainer pays)
        q = torch.nn.Parameter(p.clone())
        q.grad = g.clone()
        for label, cls, kw in (("torch.optim.AdamW", torch.optim.AdamW, dict(weight_decay=WD)),
                               ("torch.optim.Adam amsgrad", torch.optim.Adam, dict(weight_decay=WD, amsgrad=True)),
                               ("torch.optim.SGD momentum 0.9", torch.optim.SGD, dict(momentum=0.9, weight_decay=WD))):
            for impl in ("foreach", "fused"):
                try:
                    opt = cls([q], lr=1e-4, **kw, **{impl: True})
                    t = time_one(opt.step, args.reps, args.iters)
                except (RuntimeError, TypeError, ValueError) as e:  # this torch has no such implementation
                    print(f"  {label + ' ' + impl:30s} not available ({type(e).__name__})", flush=True)
                    continue
                print(f"  {label + ' ' + impl:30s} {t * 1e3:8.1f} us", flush=True)
                del opt
        assert torch.isfinite(p).all()
        del p, g, m, v, vmax, buf, q
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
