"""Generate the lr-schedule fixture (lr_schedules.npz) by running the REFERENCE's basicsr/models/lr_scheduler.py on the
cases of tests/lr_schedule_fixtures.py.

Test infrastructure only, as make_golden_pixel_losses.py: the reference file is loaded by path at run time; nothing of
it is stored but the numbers it produces.  Each case builds a one-parameter torch optimizer, the scheduler
base_model.setup_schedulers would build for the case's `train:` dict, and then does per iteration what
base_model.update_learning_rate does (step the scheduler from iteration 2 on; while current_iter < warmup_iter set the
group's lr to initial_lr / warmup_iter * current_iter), recording the group's lr.

Per case the file holds
  <name>         float64 [n]: the lr iteration i + 1 runs with
  <name>__keys   the keys of the reference scheduler's state_dict() (sorted)
  <name>__final  float64 [3]: last_epoch, _step_count and _last_lr[0] after the n iterations

Usage:  python tests/golden/make_golden_lr_schedules.py --ref <checkout of the reference>
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lr_schedule_fixtures as F  # noqa: E402


def load_reference(ref: str):
    path = os.path.join(ref, "NAFNet_base", "basicsr", "models", "lr_scheduler.py")
    spec = importlib.util.spec_from_file_location("ref_lr_scheduler", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build(ref, opt, optimizer):
    kind = opt["scheduler"].pop("type")
    if kind in ("MultiStepLR", "MultiStepRestartLR"):
        return ref.MultiStepRestartLR(optimizer, **opt["scheduler"])
    if kind == "CosineAnnealingRestartLR":
        return ref.CosineAnnealingRestartLR(optimizer, **opt["scheduler"])
    if kind == "TrueCosineAnnealingLR":
        return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, **opt["scheduler"])
    if kind == "LinearLR":
        return ref.LinearLR(optimizer, opt["total_iter"])
    if kind == "VibrateLR":
        return ref.VibrateLR(optimizer, opt["total_iter"])
    raise KeyError(kind)


def run_case(ref, name):
    opt, lr, n = F.train_opt(name)
    optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = build(ref, opt, optimizer)
    warmup_iter = opt.get("warmup_iter", -1)
    out = []
    for current_iter in range(1, n + 1):
        optimizer.step()
        if current_iter > 1:
            sched.step()
        if current_iter < warmup_iter:
            for group in optimizer.param_groups:
                group["lr"] = group["initial_lr"] / warmup_iter * current_iter
        out.append(optimizer.param_groups[0]["lr"])
    assert all(isinstance(v, float) for v in out)
    sd = sched.state_dict()
    return (np.asarray(out, dtype=np.float64), np.asarray(sorted(sd)),
            np.asarray([sd["last_epoch"], sd["_step_count"], sd["_last_lr"][0]], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    args = ap.parse_args()
    ref = load_reference(args.ref)
    arrays = {}
    for name in F.CASES:
        arrays[name], arrays[name + "__keys"], arrays[name + "__final"] = run_case(ref, name)
    path = os.path.join(HERE, "lr_schedules.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(F.CASES), "cases")


if __name__ == "__main__":
    main()
