"""The learning-rate schedule cases shared by tests/golden/make_golden_lr_schedules.py (which runs the reference's
schedulers on them) and tests/test_lr_schedules_host.py (which requires the same Python floats from lr_scheduler.py).

A case is a reference `train:` dict reduced to what drives the lr: `scheduler` (with its `type`), `total_iter` where
the type reads it, `warmup_iter`, the base lr (`optim_g.lr`) and the number of iterations to run (<= 200).  Iteration
i (1-based) runs with the lr at index i - 1 of the stored array.
"""
from copy import deepcopy

_MS = dict(type="MultiStepRestartLR", milestones=[10, 30, 30, 55], gamma=0.5, restarts=[0, 40],
           restart_weights=[1, 0.5])
_CR = dict(type="CosineAnnealingRestartLR", periods=[10, 10, 10], restart_weights=[1, 0.5, 0.25], eta_min=1e-7)

CASES = {
    # a milestone listed twice applies gamma twice; 'MultiStepLR' is the same class in setup_schedulers
    "ms_repeat": dict(scheduler=dict(type="MultiStepLR", milestones=[20, 20, 50], gamma=0.3), lr=3.7e-4, n=80),
    "ms_restart": dict(scheduler=_MS, lr=5e-4, n=100),
    # warm-up ending before the first milestone (10): the restart at 0 has set initial_lr, the warm-up overrides it
    "ms_restart_warm5": dict(scheduler=_MS, lr=5e-4, n=100, warmup_iter=5),
    # warm-up ending after it: the milestone multiplies the lr the warm-up wrote, and the schedule goes on from there
    "ms_restart_warm15": dict(scheduler=_MS, lr=5e-4, n=100, warmup_iter=15),
    "ms_repeat_warm25": dict(scheduler=dict(type="MultiStepLR", milestones=[20, 20, 50], gamma=0.3), lr=3.7e-4, n=80,
                             warmup_iter=25),
    # last_epoch 0..30: one more step indexes past the last period
    "cos_restart": dict(scheduler=_CR, lr=5e-4, n=31),
    "cos_restart_warm4": dict(scheduler=_CR, lr=3.7e-4, n=31, warmup_iter=4),
    # torch's chained CosineAnnealingLR past T_max, through both of its (last_epoch - 1 - T_max) % (2 T_max) == 0 steps
    "cosine": dict(scheduler=dict(type="TrueCosineAnnealingLR", T_max=50, eta_min=1e-6), lr=5e-4, n=160),
    "cosine_warm10": dict(scheduler=dict(type="TrueCosineAnnealingLR", T_max=50, eta_min=1e-6), lr=5e-4, n=120,
                          warmup_iter=10),
    "linear_160": dict(scheduler=dict(type="LinearLR"), total_iter=160, lr=5e-4, n=160),
    "linear_400": dict(scheduler=dict(type="LinearLR"), total_iter=400, lr=3.7e-4, n=200, warmup_iter=7),
    "vibrate_160": dict(scheduler=dict(type="VibrateLR"), total_iter=160, lr=5e-4, n=160),
    "vibrate_400": dict(scheduler=dict(type="VibrateLR"), total_iter=400, lr=3.7e-4, n=200),
    "vibrate_400_warm8": dict(scheduler=dict(type="VibrateLR"), total_iter=400, lr=3.7e-4, n=200, warmup_iter=8),
}


def train_opt(name):
    """A fresh `train:` dict of the case (the builders pop 'type' from it)."""
    c = deepcopy(CASES[name])
    opt = dict(scheduler=c["scheduler"], optim_g=dict(type="Adam", lr=c["lr"]))
    if "total_iter" in c:
        opt["total_iter"] = c["total_iter"]
    if "warmup_iter" in c:
        opt["warmup_iter"] = c["warmup_iter"]
    return opt, c["lr"], c["n"]
