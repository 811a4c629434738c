"""Image output time (imgout.py: nbp_img_quantize, nbp_png_filter, nbp_png_encode, ImageWriter, Validator.run with
save_dir): one frame of 1424 x 2128 and of 2848 x 4256 (the uncropped SID frame), fp32, the smooth fields of
scripts/val_time.py.  One process, HIP events for device work and the host clock for host work, medians after warm-up,
the windows of two compared paths alternating.  Run it under `timeout`.

Per frame size it prints
  * nbp_img_quantize against the torch composition it replaces on the device (clamp, sub, div, mul, round, cast,
    permute, flip), after checking that both give the same bytes -- the one condition fixed in advance: the kernel is
    not slower, or the script exits non-zero;
  * nbp_png_filter: time per call and the rate over its algorithmic bytes (3HW read, H(1 + 3W) written);
  * the device-to-host copy of the scanlines (uint8) against that of the float32 frame, both into pinned memory;
  * nbp_png_encode at level 1 with 1 and 8 threads, against PIL's save(compress_level=1) when PIL is present, and the
    sizes of the files;
  * what two ImageWriter.write calls (restored frame and ground truth) add on the stream, the writer's frames/s, and
    a Validator.run over four items with and without save_dir.

    timeout 900 python scripts/imgout_time.py [--sizes 1424x2128,2848x4256] [--iters 7] [--reps 5]
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from val_time import frame, time_one, time_pair  # noqa: E402

from lowlight_image_enhancement_amd import imgout  # noqa: E402
from lowlight_image_enhancement_amd.validation import Validator  # noqa: E402


def torch_quantize(x, lo, hi, reverse):
    """the host route's device part: [C,H,W] float32 -> [H,W,C] uint8 with torch operators"""
    t = x.clamp(lo, hi)
    t = t - lo
    t = t / (hi - lo)
    t = t * 255.0
    t = t.round()
    t = t.to(torch.uint8)
    t = t.permute(1, 2, 0)
    if reverse:
        t = t.flip(-1)
    return t.contiguous()


def host_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


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
        pred, gt = frame(H, W, dev, 1)[0], frame(H, W, dev, 2)[0]
        print(f"3 x {H} x {W} ({n} pixels)", flush=True)

        # ---- the quantiser against the torch composition
        new, old = imgout._quantize(pred, 0.0, 1.0, True), torch_quantize(pred, 0.0, 1.0, True)
        assert torch.equal(new, old), int((new != old).sum())
        t_new, t_old = time_pair(lambda: imgout._quantize(pred, 0.0, 1.0, True),
                                 lambda: torch_quantize(pred, 0.0, 1.0, True), args.reps, args.iters)
        good = t_new <= t_old
        ok = ok and good
        print(f"  nbp_img_quantize against clamp/sub/div/mul/round/cast/permute/flip: new {t_new:.3f} ms, existing "
              f"{t_old:.3f} ms ({t_old / t_new:.2f}x), {15 * n / t_new / 1e6:.0f} GB/s over 15 B/px: "
              f"{'pass (not slower)' if good else 'FAIL (slower)'}", flush=True)

        # ---- the filter
        hwc = imgout._quantize(pred, 0.0, 1.0, False)
        t_f = time_one(lambda: imgout._filter(hwc), args.reps, args.iters)
        b_f = 3 * n + H * (1 + 3 * W)
        print(f"  nbp_png_filter: {t_f * 1e3:.1f} us per call, {b_f / 1e6:.1f} MB -> {b_f / t_f / 1e6:.0f} GB/s",
              flush=True)
        scan = imgout._filter(hwc)
        types = np.bincount(scan[:, 0].cpu().numpy(), minlength=5)
        print(f"  filter types chosen (0-4): {types.tolist()}", flush=True)

        # ---- device-to-host: one byte per sample against four
        pin8 = torch.empty(scan.numel(), dtype=torch.uint8, pin_memory=True)
        pin32 = torch.empty(pred.numel(), dtype=torch.float32, pin_memory=True)
        t_c8, t_c32 = time_pair(lambda: pin8.copy_(scan.view(-1), non_blocking=True),
                                lambda: pin32.copy_(pred.view(-1), non_blocking=True), args.reps, args.iters)
        print(f"  device-to-host into pinned memory: scanlines {scan.numel() / 1e6:.1f} MB {t_c8:.3f} ms, float32 frame "
              f"{pred.numel() * 4 / 1e6:.1f} MB {t_c32:.3f} ms", flush=True)

        # ---- the host encoder
        torch.cuda.synchronize()
        host = pin8.numpy()
        out = np.empty(imgout.lib().dll.nbp_png_encode_bound(H, W, 3), dtype=np.uint8)
        enc = {}
        for nt in (1, 8):
            enc[nt] = host_ms(lambda: imgout.png_encode(host, H, W, 3, 1, nt, out), max(3, args.iters // 2))
        size_new = imgout.png_encode(host, H, W, 3, 1, 8, out).size
        line = (f"  nbp_png_encode level 1: 1 thread {enc[1]:.1f} ms, 8 threads {enc[8]:.1f} ms "
                f"({enc[1] / enc[8]:.2f}x), file {size_new / 1e6:.2f} MB")
        try:
            from PIL import Image
            rgb = hwc.cpu().numpy()

            def pil_save():
                bio = io.BytesIO()
                Image.fromarray(rgb).save(bio, format="PNG", compress_level=1)
                return bio.tell()

            line += f"; PIL save(compress_level=1) {host_ms(pil_save, 3):.1f} ms, file {pil_save() / 1e6:.2f} MB"
        except ImportError:
            line += "; PIL not present: not measured"
        print(line, flush=True)

        # ---- the writer and the validation pass
        with tempfile.TemporaryDirectory() as tmp:
            with imgout.ImageWriter(nthreads=8, level=1, depth=2) as w:
                for i in range(2):  # warm-up: the pinned ring and the worker's buffer
                    w.write(pred, os.path.join(tmp, f"w{i}.png"))
                w.flush()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                w.write(pred, os.path.join(tmp, "p.png"))
                w.write(gt, os.path.join(tmp, "g.png"))
                e1.record()
                e1.synchronize()
                print(f"  two ImageWriter.write calls (restored frame + ground truth) on the stream: "
                      f"{e0.elapsed_time(e1):.3f} ms", flush=True)
                w.flush()
                k = 8
                t0 = time.perf_counter()
                for i in range(k):
                    w.write(pred if i % 2 else gt, os.path.join(tmp, f"s{i}.png"))
                w.flush()
                dt = time.perf_counter() - t0
                print(f"  ImageWriter (8 threads, level 1, depth 2): {k / dt:.1f} frames/s ({dt / k * 1e3:.1f} ms per "
                      f"frame, files on a temporary directory)", flush=True)
            items = [{"lq": pred[None], "gt": gt[None], "lq_path": f"item{i}.png"} for i in range(4)]
            val = Validator({"metrics": {"psnr": {"type": "linear_psnr"}, "ssim": {"type": "linear_ssim"}}}, device=dev)

            def net(x):
                return 0.9 * x + 0.02

            val.run(net, items[:1])
            t_plain = host_ms(lambda: val.run(net, items), 3)
            t_save = host_ms(lambda: val.run(net, items, save_dir=os.path.join(tmp, "vis")), 3)
            print(f"  Validator.run over 4 items (psnr + ssim): {t_plain:.1f} ms, with save_dir (8 files written when "
                  f"it returns) {t_save:.1f} ms", flush=True)
        del pred, gt, hwc, scan, new, old
        torch.cuda.empty_cache()
    print("nbp_img_quantize against the torch composition:", "not slower at every size" if ok else "SLOWER somewhere")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
