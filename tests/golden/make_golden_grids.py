"""Generate the tiled-inference fixtures (grid_plans.npz, grid_blend.npz, grid_nets.npz) by running the REFERENCE.

Test infrastructure only, as make_golden.py (whose reference loader and writers it uses): the reference's
ImageRestorationModel (NAFNet_base/basicsr/models/image_restoration_model.py) is loaded at run time behind stub modules
for what it imports but grids() / test() / grids_inverse() never touch, and the three unbound methods are called on a
bare namespace object carrying opt, scale, device, lq, gt and net_g.  Nothing of the reference is stored but the numbers
it produces.  Network parameters are not stored either: they come from param_recipe.recipe_state by seed.

The reference's grids_inverse() reads `self.outs`, which nothing in it assigns (test() writes `self.output`), so
`val.grids: true` raises there as written.  The fixtures pin the evident intent: run() below sets outs = output, the
tile outputs of test() in tile order, between the two calls.

Usage:  python tests/golden/make_golden_grids.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference, save, t2n  # noqa: E402
from param_recipe import recipe_state  # noqa: E402

W8 = dict(img_channel=3, width=8, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])
# hand-picked plans: (h, w, opt['val'])
PLAN_CASES = [
    (70, 90, {"crop_size_h": 32, "crop_size_w": 32}),
    (33, 32, {"crop_size_h": 32, "crop_size_w": 32}),    # step 1: two tiles that almost coincide
    (64, 96, {"crop_size_h": 32, "crop_size_w": 32}),    # exact tiling, no overlap
    (50, 77, {"crop_size_h_ratio": 0.5, "crop_size_w_ratio": 0.34}),
    (40, 40, {"crop_size_h": 40, "crop_size_w": 40}),    # one tile
    (97, 61, {"crop_size_h": 24, "crop_size_w": 40}),    # the clamped last row at 73
    (65, 100, {"crop_size_h": 32, "crop_size_w": 33}),
]
SWEEP_MAX = 64          # every (h, c) with 1 <= c <= h <= SWEEP_MAX on one axis ...
SWEEP_OTHER = (7, 5)    # ... paired with this (extent, crop) on the other: origins 0, 2
BLEND_CASES = [5, 1, 2, 6]  # indices into PLAN_CASES: 97x61 / 24x40, 33x32 / 32x32, 64x96 / 32x32, 65x100 / 32x33
# network cases: (lq shape, opt['val'], seed)
NET_CASES = [
    ((1, 3, 70, 90), {"crop_size_h": 32, "crop_size_w": 32, "max_minibatch": 4}, 431),  # nine tiles in chunks 4, 4, 1
    ((1, 3, 61, 75), {"crop_size_h": 30, "crop_size_w": 34}, 432),  # crops no multiple of the padder: every tile is padded
]


def load_model_class(ref: str):
    """ImageRestorationModel, its module loaded by path behind stubs (load_reference has made `basicsr` a stub package)"""
    def stub(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__dict__.setdefault("__path__", [])
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m

    def unused(*a, **k):
        raise RuntimeError("stub: not part of grids() / test() / grids_inverse()")

    stub("tqdm", tqdm=unused)
    stub("basicsr.models.archs", define_network=unused)
    stub("basicsr.models.base_model", BaseModel=object)
    stub("basicsr.utils", imwrite=unused, tensor2img=unused)
    stub("basicsr.utils.dist_util", get_dist_info=lambda: (0, 1))
    stub("basicsr.models.losses")
    stub("basicsr.metrics")
    path = os.path.join(ref, "NAFNet_base", "basicsr", "models", "image_restoration_model.py")
    spec = importlib.util.spec_from_file_location("basicsr.models.image_restoration_model", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.ImageRestorationModel


def bare(val_opt, lq, net=None):
    """the attributes the three methods read, on an object that is not a model"""
    return types.SimpleNamespace(opt={"val": dict(val_opt)}, scale=1, device=torch.device("cpu"), lq=lq, gt=lq, net_g=net)


def plan_of(M, h, w, val_opt):
    """(crop_h, crop_w, i origins, j origins) of every tile, from the reference's grids()"""
    ns = bare(val_opt, torch.zeros(1, 1, h, w))
    M.grids(ns)
    T = len(ns.idxes)
    crop = ns.lq.shape[2:]
    assert ns.lq.shape[0] == T
    return int(crop[0]), int(crop[1]), [d["i"] for d in ns.idxes], [d["j"] for d in ns.idxes]


def gen_plans(M):
    out = {"n_cases": np.asarray(len(PLAN_CASES), dtype=np.int64)}
    for k, (h, w, opt) in enumerate(PLAN_CASES):
        ch, cw, ii, jj = plan_of(M, h, w, opt)
        out[f"hw_{k}"] = np.asarray([h, w], dtype=np.int64)
        out[f"size_{k}"] = np.asarray([opt.get("crop_size_h", -1), opt.get("crop_size_w", -1)], dtype=np.int64)
        out[f"ratio_{k}"] = np.asarray([opt.get("crop_size_h_ratio", np.nan), opt.get("crop_size_w_ratio", np.nan)],
                                       dtype=np.float64)
        out[f"crop_{k}"] = np.asarray([ch, cw], dtype=np.int64)
        out[f"i_{k}"] = np.asarray(ii, dtype=np.int64)
        out[f"j_{k}"] = np.asarray(jj, dtype=np.int64)
    # the sweep: the swept axis once as rows, once as columns; per (h, c) the origins along the swept axis
    oh, oc = SWEEP_OTHER
    hc, off, rows, cols = [], [0], [], []
    for h in range(1, SWEEP_MAX + 1):
        for c in range(1, h + 1):
            _, _, ii, jj = plan_of(M, h, oh, {"crop_size_h": c, "crop_size_w": oc})
            assert sorted(set(jj)) == [0, 2]
            r = [i for i, j in zip(ii, jj) if j == 0]
            _, _, ii, jj = plan_of(M, oh, h, {"crop_size_h": oc, "crop_size_w": c})
            assert sorted(set(ii)) == [0, 2]
            q = [j for i, j in zip(ii, jj) if i == 0]
            assert len(r) == len(q)
            hc.append([h, c])
            rows += r
            cols += q
            off.append(len(rows))
    out["sweep_other"] = np.asarray(SWEEP_OTHER, dtype=np.int64)
    out["sweep_hc"] = np.asarray(hc, dtype=np.int64)
    out["sweep_off"] = np.asarray(off, dtype=np.int64)
    out["sweep_rows"] = np.asarray(rows, dtype=np.int64)
    out["sweep_cols"] = np.asarray(cols, dtype=np.int64)
    save("grid_plans.npz", **out)


def gen_blend(M):
    gen = torch.Generator().manual_seed(441)
    out = {"cases": np.asarray(BLEND_CASES, dtype=np.int64)}
    for k in BLEND_CASES:
        h, w, opt = PLAN_CASES[k]
        ns = bare(opt, torch.zeros(1, 3, h, w))
        M.grids(ns)
        outs = torch.randn(ns.lq.shape, generator=gen)
        # signed zeros: scattered ones, and two rows of every tile so that overlapping tiles meet -0.0 with -0.0
        outs.view(-1)[::97] = -0.0
        outs[:, 1, :2, :] = -0.0
        ns.outs = outs  # the reference never assigns `outs`: see the module docstring
        M.grids_inverse(ns)
        assert ns.output.shape == (1, 3, h, w) and ns.lq.shape == (1, 3, h, w)
        out[f"outs_{k}"] = t2n(outs)
        out[f"out_{k}"] = t2n(ns.output)
    save("grid_blend.npz", **out)


def gen_nets(R, M):
    out = {"n_cases": np.asarray(len(NET_CASES), dtype=np.int64)}
    for k, (shape, opt, seed) in enumerate(NET_CASES):
        torch.manual_seed(seed)
        net = R.arch.NAFNet(**W8)
        net.load_state_dict(recipe_state([(n, tuple(v.shape)) for n, v in net.state_dict().items()], seed=seed))
        gen = torch.Generator().manual_seed(seed + 1000)
        lq = torch.randint(0, 256, shape, generator=gen).float() / 255.0  # an 8-bit image
        ns = bare(opt, lq, net)
        M.grids(ns)
        tiles = ns.lq.shape[0]
        M.test(ns)
        ns.outs = ns.output  # the reference never assigns `outs`: see the module docstring
        M.grids_inverse(ns)
        with torch.no_grad():
            whole = net(lq)
        print(f"net case {k}: {tiles} tiles, max |tiled - whole-frame| = {(ns.output - whole).abs().max().item():.3e}")
        out[f"lq_{k}"] = t2n(lq)
        out[f"out_{k}"] = t2n(ns.output)
        out[f"seed_{k}"] = np.asarray(seed, dtype=np.int64)
        out[f"crop_{k}"] = np.asarray([opt["crop_size_h"], opt["crop_size_w"]], dtype=np.int64)
        out[f"minibatch_{k}"] = np.asarray(opt.get("max_minibatch", -1), dtype=np.int64)
        out[f"tiles_{k}"] = np.asarray(tiles, dtype=np.int64)
    save("grid_nets.npz", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    R = load_reference(args.ref)
    M = load_model_class(args.ref)
    gen_plans(M)
    gen_blend(M)
    gen_nets(R, M)


if __name__ == "__main__":
    main()
