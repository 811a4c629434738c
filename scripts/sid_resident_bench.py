"""HBM-resident SID dataset: what a batch costs once the frames live on the device.

  (a) nbp_sid_crop_to_float (gather from resident frames) against nbp_sid_to_float (dense uint16 crops) at the same
      B, h, w, in one process, alternating, HIP events, median after warm-up: 16 x 256^2, 16 x 512^2, 1 x 2848 x 4256.
      The resident frames are random uint16 made on the device at 2848 x 4256 (no PNGs); a few dozen of them, drawn
      at random, so the windows do not come from a cache.
  (b) wall time per batch of a bare CUDAPrefetcher.next() loop over the resident dataset at 16 x 256^2, no training
      step: the host cost of a batch (RNG draws, collate, validation, descriptor upload, launch).
  (c) the one-off build: frames per second of decode + upload on synthetic PNG16 files (as sid_input_bench.py makes
      them), disk backend.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
import torch

from sid_input_bench import png16


def _manifest(root, pairs, ext=".png"):
    os.makedirs(os.path.join(root, "short"), exist_ok=True)
    os.makedirs(os.path.join(root, "long"), exist_ok=True)
    recs = [{"pair_id": f"p{i}", "subset": "train", "short_key": f"s{i}{ext}", "long_key": f"l{i}{ext}",
             "short_exposure": 0.1, "long_exposure": 10.0, "exposure_ratio": 100.0} for i in range(pairs)]
    with open(os.path.join(root, "manifest.json"), "w") as f:
        json.dump(recs, f)
    return {"manifest_path": os.path.join(root, "manifest.json"), "phase": "train", "subset": "train", "seed": 0,
            "io_backend": {"type": "disk", "paths": {"short": os.path.join(root, "short"),
                                                     "long": os.path.join(root, "long")}}}


def kernel_times(frames, ptrs, hw, H, W, shapes, iters, warmup):
    """(a): per shape, the median event time of the gather and of the dense conversion, alternated."""
    from lowlight_image_enhancement_amd._lib import call
    dev = ptrs.device
    rng = np.random.default_rng(1)
    F = len(frames)
    out = {}
    for B, h, w in shapes:
        outs = tuple(torch.empty(B, 3, h, w, device=dev) for _ in range(3))
        ratio = torch.full((B,), 100.0, device=dev)
        nsets = 8 if h * w < 1 << 20 else 2  # dense inputs rotated, as the gather's windows are
        dense = [torch.randint(-32768, 32767, (2, B, h, w, 3), dtype=torch.int16, device=dev) for _ in range(nsets)]
        descs = []
        for _ in range(warmup + iters):
            d = np.stack([rng.integers(0, F, B), rng.integers(0, F, B), rng.integers(0, H - h + 1, B),
                          rng.integers(0, W - w + 1, B)], 1).astype(np.int32)
            descs.append(torch.from_numpy(d).to(dev))
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(warmup + iters)]
        torch.cuda.synchronize()
        for i in range(warmup + iters):
            ev[i][0].record()
            call("sid_crop_to_float", ptrs, hw, descs[i], ratio, B, F, h, w, *outs)
            ev[i][1].record()
            call("sid_to_float", dense[i % nsets][0], dense[i % nsets][1], ratio, B, h, w, *outs)
            ev[i][2].record()
        torch.cuda.synchronize()
        crop = statistics.median(e[0].elapsed_time(e[1]) for e in ev[warmup:])
        conv = statistics.median(e[1].elapsed_time(e[2]) for e in ev[warmup:])
        nbytes = B * h * w * 3 * (2 * 2 + 3 * 4)
        out[f"{B}x{h}x{w}"] = {"crop_us": round(crop * 1e3, 1), "to_float_us": round(conv * 1e3, 1),
                               "ratio": round(crop / conv, 3), "crop_GBps": round(nbytes / crop / 1e6, 1),
                               "to_float_GBps": round(nbytes / conv / 1e6, 1)}
        del dense, outs
    return out


def prefetcher_time(frames, H, W, batch, ps, epochs):
    """(b): wall ms per batch of CUDAPrefetcher.next() over a resident dataset whose frames are `frames`."""
    from lowlight_image_enhancement_amd.data import CUDAPrefetcher, SonySIDResidentDataset, create_dataloader
    from lowlight_image_enhancement_amd.data.sony_sid_resident_dataset import _Resident

    class DeviceMade(SonySIDResidentDataset):  # the frames are already on the device: no PNG behind a key
        def _header_shape(self, client, key):
            return H, W, 3

        def build(self):
            if self._resident is None:
                self._resident = _Resident(frames, frames[0].device)
            return self._resident

    pairs = len(frames) // 2
    with tempfile.TemporaryDirectory() as root:
        opt = _manifest(root, pairs)
        opt.update(patch_size=ps, samples_per_pair=max(1, 96 * batch // pairs))
        ds = DeviceMade(opt)
    loader = create_dataloader(ds, {"phase": "train", "batch_size_per_gpu": batch, "num_worker_per_gpu": 8,
                                    "pin_memory": True}, seed=0)
    pf = CUDAPrefetcher(loader, {"num_gpu": 1})
    per_batch = []
    for _ in range(epochs + 1):  # the first epoch is warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while pf.next() is not None:
            n += 1
        torch.cuda.synchronize()
        per_batch.append((time.perf_counter() - t0) / n * 1e3)
        pf.reset()
    return {"batches_per_epoch": n, "num_workers": loader.num_workers,
            "ms_per_batch_median": round(statistics.median(per_batch[1:]), 3),
            "ms_per_batch_epochs": [round(v, 3) for v in per_batch[1:]]}


def build_time(H, W, pairs, threads):
    """(c): decode + upload of 2 * pairs synthetic PNG16 frames through SonySIDResidentDataset.build()."""
    from lowlight_image_enhancement_amd.data import SonySIDResidentDataset
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    pngs = []
    for i in range(4):
        img = np.stack([(yy * 7 + xx * 3 + 997 * c + 1000 * i) % 60000 for c in range(3)], -1)
        pngs.append(png16((img + rng.integers(0, 256, img.shape)).astype(np.uint16)))
    with tempfile.TemporaryDirectory() as root:
        opt = _manifest(root, pairs)
        for i in range(pairs):
            for kind, j in (("short", 2 * i), ("long", 2 * i + 1)):
                with open(os.path.join(root, kind, f"{kind[0]}{i}.png"), "wb") as f:
                    f.write(pngs[j % 4])
        opt["resident"] = {"decode_threads": threads}
        t0 = time.perf_counter()
        ds = SonySIDResidentDataset(opt)
        t_plan = time.perf_counter() - t0
        t0 = time.perf_counter()
        res = ds.build()
        t_build = time.perf_counter() - t0
    n = len(res.frames)
    return {"frames": n, "decode_threads": threads, "png_bytes_mean": int(np.mean([len(p) for p in pngs])),
            "plan_s": round(t_plan, 3), "build_s": round(t_build, 3), "frames_per_s": round(n / t_build, 2),
            "resident_MB": round(ds.plan.total_bytes / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48, help="resident random frames for (a) and (b)")
    ap.add_argument("--H", type=int, default=2848)
    ap.add_argument("--W", type=int, default=4256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--build-pairs", type=int, default=8)
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sid_resident_bench: needs the GPU (nothing here can be timed without it)")
    dev = torch.device("cuda")
    H, W = args.H, args.W
    frames = [torch.randint(-32768, 32767, (H, W, 3), dtype=torch.int16, device=dev) for _ in range(args.frames)]
    ptrs = torch.tensor([t.data_ptr() for t in frames], dtype=torch.int64).to(dev)
    hw = torch.tensor([[H, W]] * len(frames), dtype=torch.int32).to(dev)
    shapes = [(16, min(256, H), min(256, W)), (16, min(512, H), min(512, W)), (1, H, W)]
    res = {"resident_frames": len(frames), "frame": [H, W],
           "kernel": kernel_times(frames, ptrs, hw, H, W, shapes, args.iters, args.warmup)}
    print(res, flush=True)
    pre = {"prefetcher_16x256": prefetcher_time(frames, H, W, 16, min(256, H, W), args.epochs)}
    print(pre, flush=True)
    del frames
    torch.cuda.empty_cache()
    print({"build": build_time(H, W, args.build_pairs, args.threads)}, flush=True)


if __name__ == "__main__":
    main()
