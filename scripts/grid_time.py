"""Tiled full-frame inference time (tiling.tiled_forward, the reference's val.grids mode): cfg2 (w32
[2,2,4,8]/12/[2,2,2,2]), fp16, 256 x 256 crops, one image of 1424 x 2128 and of 2848 x 4256 (the uncropped SID frame),
max_minibatch 16 and 32.  One process, HIP events, medians after warm-up.  Run it under `timeout`.

Per frame size it prints
  * the whole tiled forward per max_minibatch, and beside it the whole-frame forwards of NAFNetLocal and the plain NAFNet
    on the same weights (skipped with --no-nets);
  * nbp_grid_gather (one chunk of `max_minibatch` tiles) and nbp_grid_blend (all tiles) on their own: time per launch,
    algorithmic bytes (every tensor once: the tiles read or written plus the frame pixels read or written) and the
    rate they give;
  * the same two steps as the torch ops a user would write without them: slices + cat per chunk; zeros, one `+=` per
    tile, the count map and the divide;
  * the one condition fixed in advance: gather (all chunks) + blend is not slower than that formulation in this run.

A step is timed as `reps` back-to-back calls between two events, alternating the two formulations, median of `--iters`
such windows.

    timeout 900 python scripts/grid_time.py [--sizes 1424x2128,2848x4256] [--minibatch 16,32] [--iters 7] [--no-nets]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lowlight_image_enhancement_amd import _lib  # noqa: E402
from lowlight_image_enhancement_amd.nafnet import NAFNet, NAFNetLocal  # noqa: E402
from lowlight_image_enhancement_amd.tiling import _device_plan, grid_plan, tiled_forward  # noqa: E402

CFG2 = dict(img_channel=3, width=32, enc_blk_nums=[2, 2, 4, 8], middle_blk_num=12, dec_blk_nums=[2, 2, 2, 2])
CROP = 256


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


def time_forward(fn, iters, warmup=2):
    with torch.no_grad():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        return statistics.median(window_ms(fn, 1) for _ in range(iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1424x2128,2848x4256")
    ap.add_argument("--minibatch", default="16,32")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-nets", action="store_true", help="time the gather / blend steps only")
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
    local = NAFNetLocal.from_net(net, train_size=(1, 3, CROP, CROP))
    mbs = [int(v) for v in args.minibatch.split(",")]
    ok = True
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        C = 3
        lq = torch.rand(1, C, H, W, device=dev)
        opt = {"crop_size_h": CROP, "crop_size_w": CROP}
        _, _, idxes = grid_plan(H, W, opt)
        plan = _device_plan(H, W, CROP, CROP)
        T = len(idxes)
        print(f"{H}x{W}: {plan[0]} x {plan[2]} = {T} tiles of {CROP}x{CROP}, steps {plan[1]} / {plan[3]}", flush=True)

        # ---- gather and blend on their own, against the torch-op formulation
        img = lq[0]
        outs = torch.rand(T, C, CROP, CROP, device=dev)
        out = torch.empty(C, H, W, device=dev)
        tile_bytes = C * CROP * CROP * 4

        def blend_hip():
            _lib.call("grid_blend", outs, out, C, H, W, CROP, CROP, *plan)

        def blend_torch():
            preds = torch.zeros(1, C, H, W, device=dev)
            count = torch.zeros(1, 1, H, W, device=dev)
            for t, d in enumerate(idxes):
                i, j = d["i"], d["j"]
                preds[0, :, i:i + CROP, j:j + CROP] += outs[t]
                count[0, 0, i:i + CROP, j:j + CROP] += 1.0
            return preds / count

        blend_hip()
        assert torch.equal(blend_torch()[0].view(torch.int32), out.view(torch.int32))
        b_hip, b_torch = time_pair(blend_hip, blend_torch, max(1, args.reps // 4), args.iters)
        b_bytes = T * tile_bytes + C * H * W * 4
        print(f"  blend: nbp_grid_blend {b_hip * 1e3:.1f} us per launch, {b_bytes / 1e6:.1f} MB -> "
              f"{b_bytes / b_hip / 1e6:.0f} GB/s; torch ops ({2 * T + 3} launches) {b_torch * 1e3:.1f} us", flush=True)
        for mb in mbs:
            n = min(mb, T)
            tiles = torch.empty(n, C, CROP, CROP, device=dev)
            t0 = (T - n) // 2  # a chunk from the middle of the plan

            def gather_hip():
                _lib.call("grid_gather", img, tiles, C, H, W, CROP, CROP, *plan, t0, n)

            def gather_torch():
                return torch.cat([lq[:, :, d["i"]:d["i"] + CROP, d["j"]:d["j"] + CROP] for d in idxes[t0:t0 + n]], dim=0)

            gather_hip()
            assert torch.equal(gather_torch(), tiles)
            g_hip, g_torch = time_pair(gather_hip, gather_torch, args.reps, args.iters)
            g_bytes = 2 * n * tile_bytes
            chunks = (T + mb - 1) // mb
            tot_hip = g_hip * T / n + b_hip  # every chunk at this chunk's rate, plus the blend
            tot_torch = g_torch * T / n + b_torch
            verdict = "not slower" if tot_hip <= tot_torch else "SLOWER"
            ok = ok and tot_hip <= tot_torch
            print(f"  max_minibatch {mb}: nbp_grid_gather of {n} tiles {g_hip * 1e3:.1f} us per launch, "
                  f"{g_bytes / 1e6:.1f} MB -> {g_bytes / g_hip / 1e6:.0f} GB/s; slices + cat {g_torch * 1e3:.1f} us; "
                  f"gather ({chunks} launches) + blend {tot_hip * 1e3:.0f} us against {tot_torch * 1e3:.0f} us in torch "
                  f"ops: {verdict}", flush=True)
        del outs, out
        if args.no_nets:
            continue

        # ---- the whole forwards
        for mb in mbs:
            torch.cuda.reset_peak_memory_stats()
            ms = time_forward(lambda: tiled_forward(net, lq, dict(opt, max_minibatch=mb)), args.iters)
            print(f"  tiled forward, max_minibatch {mb}: {ms:.2f} ms per frame (median of {args.iters}), peak memory "
                  f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)
        for name, m in (("NAFNetLocal", local), ("plain NAFNet", net)):
            try:
                torch.cuda.reset_peak_memory_stats()
                ms = time_forward(lambda: m(lq), args.iters)
                print(f"  {name}, whole frame: {ms:.2f} ms (median of {args.iters}), peak memory "
                      f"{torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB", flush=True)
            except (_lib.NBPError, torch.cuda.OutOfMemoryError) as e:  # refused, not faulted: say so and go on
                print(f"  {name}, whole frame: does not run: {type(e).__name__}: {str(e)[:300]}", flush=True)
            torch.cuda.empty_cache()
    print("gather + blend against the torch-op formulation:", "not slower at every size" if ok else "SLOWER somewhere")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
