"""The module-API AMP body, timed: cfg2 (w32 [2,2,4,8]/12/[2,2,2,2]), 16 images of 256 x 256, the way the reference's
optimize_parameters drives its network (image_restoration_model.py:255-257, 308-310):

    with torch.autocast("cuda", dtype=torch.float16):
        preds = net(lq)
        loss = l1_loss(preds, gt)
    scaler.scale(loss).backward()

No attribute of the network is set: what the region selects is what is measured (the fp32 kernels before NAFNet read the
autocast state, the fp16 kernels since).  One process, HIP events around each iteration, the median after warm-up; run it
with no other GPU process, under `timeout`.  Prints one JSON line.

    timeout 600 python scripts/autocast_time.py [--iters 20] [--warmup 5] [--batch 16] [--size 256]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lowlight_image_enhancement_amd.nafnet import NAFNet  # noqa: E402

CFG2 = dict(img_channel=3, width=32, enc_blk_nums=[2, 2, 4, 8], middle_blk_num=12, dec_blk_nums=[2, 2, 2, 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = NAFNet(**CFG2).to(dev)
    with torch.no_grad():
        net.flat.add_(torch.randn_like(net.flat) * 0.02)  # beta / gamma away from zero: every branch is live
    gen = torch.Generator().manual_seed(1)
    lq = (torch.rand(args.batch, 3, args.size, args.size, generator=gen) * 0.3).to(dev)
    gt = torch.rand(args.batch, 3, args.size, args.size, generator=gen).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        scaler = torch.cuda.amp.GradScaler(init_scale=2.0 ** 16)

    def body():
        net.flat.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            preds = net(lq)
            loss = torch.nn.functional.l1_loss(preds, gt)
        scaler.scale(loss).backward()
        return preds

    for _ in range(args.warmup):
        preds = body()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(net.flat.grad).all().item())
    ms = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        body()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(json.dumps({"workload": "cfg2", "batch": args.batch, "size": args.size, "iters": args.iters,
                      "precision_setting": getattr(net, "precision", None), "preds_dtype": str(preds.dtype),
                      "grad_finite": finite, "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
                      "ms_max": round(max(ms), 3), "img_per_s": round(args.batch * 1000.0 / med, 1)}))


if __name__ == "__main__":
    main()
