"""Generate the TLSC / NAFNetLocal fixtures (tlsc_kernels.npz, tlsc_pool.npz, tlsc_nets.npz) by running the REFERENCE.

Test infrastructure only, as make_golden.py (whose reference loader and writers it uses): the reference's
NAFNetLocal (NAFNet_arch.py:164-174) and its test-time local converter (local_arch.py:10-104) are imported at run time;
nothing of them is stored but the numbers they produce.  Network parameters are not stored either: they come from
param_recipe.recipe_state by seed.

Usage:  python tests/golden/make_golden_tlsc.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference, save, t2n  # noqa: E402
from param_recipe import recipe_state  # noqa: E402

W8 = dict(img_channel=3, width=8, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
W32 = dict(img_channel=3, width=32, enc_blk_nums=[1, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])
# case: (cfg, train_size, input shape, seed)
CASES = {
    "A": (W8, (1, 3, 24, 40), (2, 3, 70, 90), 411),   # local at every level, odd middle kernel, padding, batch 2
    "B": (W8, (1, 3, 24, 40), (1, 3, 30, 90), 412),   # k1 >= h at every level: local in width only
    "C": (W8, (1, 3, 32, 32), (1, 3, 32, 48), 413),   # every block global
    "D": (W32, (1, 3, 64, 64), (1, 3, 192, 128), 414),  # 5 levels, C 32 .. 512
}
KERNEL_TRAIN_SIZES = [(1, 3, 24, 40), (1, 3, 30, 44), (1, 3, 256, 256)]
# AvgPool2d stage: (input NCHW shape, kernel)
POOL_CASES = [((2, 8, 18, 23), (9, 15)), ((1, 8, 8, 23), (9, 15)), ((1, 16, 36, 46), (18, 30)),
              ((1, 8, 20, 9), (7, 12))]


def _pools(R, net):
    """[(block prefix, the converter's AvgPool2d of that block)] in module order"""
    local = sys.modules["basicsr.models.archs.local_arch"]
    return [(n[:-len("sca.0")], m) for n, m in net.named_modules() if isinstance(m, local.AvgPool2d)]


def gen_kernels(R):
    out = {}
    for i, ts in enumerate(KERNEL_TRAIN_SIZES):
        net = R.arch.NAFNetLocal(train_size=ts, **W8)
        pools = _pools(R, net)
        out[f"train_{i}"] = np.asarray(ts, dtype=np.int64)
        out[f"names_{i}"] = np.asarray([n for n, _ in pools])
        out[f"ks_{i}"] = np.asarray([list(m.kernel_size) for _, m in pools], dtype=np.int64)
    save("tlsc_kernels.npz", **out)


def gen_pool(R):
    local = sys.modules["basicsr.models.archs.local_arch"]
    gen = torch.Generator().manual_seed(421)
    out = {}
    for i, (shape, k) in enumerate(POOL_CASES):
        x = torch.randn(shape, generator=gen)
        pool = local.AvgPool2d(kernel_size=list(k))
        out[f"x_{i}"] = t2n(x)
        out[f"k_{i}"] = np.asarray(k, dtype=np.int64)
        out[f"out_{i}"] = t2n(pool(x))
    save("tlsc_pool.npz", **out)


def gen_nets(R):
    out = {}
    for name, (cfg, ts, shape, seed) in CASES.items():
        torch.manual_seed(seed)
        net = R.arch.NAFNetLocal(train_size=ts, **cfg)
        st = recipe_state([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed=seed)
        net.load_state_dict(st)
        gen = torch.Generator().manual_seed(seed + 1000)
        lq = torch.randint(0, 256, shape, generator=gen).float() / 255.0  # an 8-bit image
        pools = _pools(R, net)
        decided = {}
        hooks = [m.register_forward_hook(
            lambda m, inp, o, n=n: decided.__setitem__(n, not (m.kernel_size[0] >= inp[0].size(-2)
                                                               and m.kernel_size[1] >= inp[0].size(-1))))
                 for n, m in pools]
        with torch.no_grad():
            y = net(lq)
        for h in hooks:
            h.remove()
        if name == "C":  # every block global: the plain NAFNet on the same weights gives the same image
            plain = R.arch.NAFNet(**cfg)
            plain.load_state_dict(st)
            with torch.no_grad():
                assert (plain(lq) - y).abs().max().item() == 0.0
        out[f"{name}_lq"] = t2n(lq)
        out[f"{name}_out"] = t2n(y)
        out[f"{name}_seed"] = np.asarray(seed, dtype=np.int64)
        out[f"{name}_train"] = np.asarray(ts, dtype=np.int64)
        out[f"{name}_width"] = np.asarray(cfg["width"], dtype=np.int64)
        out[f"{name}_levels"] = np.asarray(len(cfg["enc_blk_nums"]), dtype=np.int64)
        out[f"{name}_names"] = np.asarray([n for n, _ in pools])
        out[f"{name}_local"] = np.asarray([decided[n] for n, _ in pools], dtype=np.bool_)
    save("tlsc_nets.npz", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    R = load_reference(args.ref)
    gen_kernels(R)
    gen_pool(R)
    gen_nets(R)


if __name__ == "__main__":
    main()
