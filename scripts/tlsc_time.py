"""Full-resolution inference time of NAFNetLocal (TLSC local-window SCA) against the plain NAFNet on the same weights:
cfg2 (w32 [2,2,4,8]/12/[2,2,2,2]), fp16, train_size (1,3,256,256), one image of 1424 x 2128 and of 2848 x 4256 (the
uncropped SID frame).  HIP events around each forward, median over the iterations after warm-up, one process.  Run it
under `timeout`.  A size at which a forward is refused (an argument check of the library, or out of memory) is reported
as such and skipped; any other error ends the run.

    timeout 600 python scripts/tlsc_time.py [--sizes 1424x2128,2848x4256] [--iters 10] [--warmup 2] [--only local|plain]

With --only local under `rocprofv3 --kernel-trace --stats` the per-kernel times of tlsc_colsum / tlsc_rowsum / tlsc_sca_a
/ tlsc_gate divide the algorithmic bytes this script prints per level ("NAFNetLocal")."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lowlight_image_enhancement_amd._lib import NBPError  # noqa: E402
from lowlight_image_enhancement_amd.nafnet import NAFNet, NAFNetLocal  # noqa: E402

CFG2 = dict(img_channel=3, width=32, enc_blk_nums=[2, 2, 4, 8], middle_blk_num=12, dec_blk_nums=[2, 2, 2, 2])


def time_forward(net, x, iters, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            net(x)
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            net(x)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def algorithmic_bytes(net, H, W, esz=2):
    """per local block of each level: (pool bytes, gate bytes) -- g read + column sums written and read + V written;
    V read + a written and read + g read + ga written (each tensor once)"""
    hp, wp = net.check_image_size_hw(H, W)
    L = len(net.enc_blk_nums)
    rows = []
    for lv in range(L + 1):
        pre = f"encoders.{lv}.0." if lv < L else "middle_blks.0."
        h, w, c = hp >> lv, wp >> lv, net.width << lv
        lk = net._local_window(pre, h, w)
        if lk is None:
            rows.append((lv, h, w, c, None, 0, 0, 0))
            continue
        hv, wv = h - lk[0] + 1, w - lk[1] + 1
        nblk = sum(1 for p in net.local_kernels if net.local_blocks(H, W)[p] and
                   (p.startswith(f"encoders.{lv}.") or p.startswith(f"decoders.{L - 1 - lv}.") or
                    (lv == L and p.startswith("middle_blks."))))
        pool = h * w * c * esz + 2 * hv * w * c * 4 + hv * wv * c * 4
        gate = 3 * hv * wv * c * 4 + 2 * h * w * c * esz
        rows.append((lv, h, w, c, lk, nblk, pool, gate))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1424x2128,2848x4256")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["local", "plain"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = NAFNet(**CFG2)
    with torch.no_grad():  # non-zero layer scales (the reference initialises them to 0)
        for k, e in net.entries.items():
            if k.endswith(("beta", "gamma")):
                net.flat.data[e.offset:e.offset + e.numel] = 0.1 * torch.randn(e.numel)
    net = net.to(dev)
    net.precision = "fp16"
    local = NAFNetLocal.from_net(net, train_size=(1, 3, 256, 256))
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        x = torch.rand(1, 3, H, W, device=dev)
        res = {}
        for name, m in (("plain", net), ("local", local)):
            if args.only and name != args.only:
                continue
            try:
                res[name] = time_forward(m, x, args.iters, args.warmup)
                print(f"{H}x{W} {name}: {res[name]:.2f} ms per image (median of {args.iters})", flush=True)
            except (NBPError, torch.cuda.OutOfMemoryError) as e:  # refused, not faulted: say so and go on
                print(f"{H}x{W} {name}: does not run: {type(e).__name__}: {str(e)[:300]}", flush=True)
            torch.cuda.empty_cache()
        if "plain" in res and "local" in res:
            print(f"{H}x{W} ratio local / plain: {res['local'] / res['plain']:.3f}", flush=True)
        for lv, h, w, c, lk, nblk, pool, gate in algorithmic_bytes(local, H, W):
            print(f"  level {lv}: map {h}x{w} C {c} window {lk} local blocks {nblk} "
                  f"pool {pool / 1e6:.1f} MB gate {gate / 1e6:.1f} MB per block", flush=True)
        print(f"  peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)


if __name__ == "__main__":
    main()
