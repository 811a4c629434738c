"""basicsr.models.lr_scheduler without an optimizer object: the schedules base_model.setup_schedulers builds
(NAFNet_base/basicsr/models/base_model.py:83-114) and the warm-up of update_learning_rate (:164-186), evaluated on
the host in float64 exactly as the reference's Python does; NBPTrainer uploads the resulting lr (4 bytes) per step.

Each object is the reference's stateful protocol over ONE parameter group: it holds `last_epoch`, the group's
current `lr` and `initial_lr` (`param_groups[0]`), is stepped once at construction (last_epoch 0) like every torch
_LRScheduler, and `step()` sets the group's lr from `get_lr()`.  Nothing is tidied into a closed form:
MultiStepRestartLR multiplies whatever lr the group holds (so it continues from what the warm-up last wrote, and a
milestone listed k times applies gamma k times), CosineAnnealingLR is torch's chained recurrence.  Where the
reference's arithmetic raises (VibrateLR with total_iter < 160, CosineAnnealingRestartLR past its last period) the
same exception type comes out of the same operation here.

`state_dict()` is torch's _LRScheduler.state_dict(): every attribute but the optimizer (here: but the parameter
group).  As in torch, the group's current lr is optimizer state; `lr` reads and sets it.
"""
from __future__ import annotations

import math
from collections import Counter
from typing import Any, Dict, List


class _Scheduler:
    def __init__(self, base_lr: float, last_epoch: int = -1):
        self.param_groups: List[Dict[str, float]] = [{"lr": base_lr, "initial_lr": base_lr}]
        self.base_lrs = [base_lr]
        self.last_epoch = last_epoch
        # the construction step of torch's LRScheduler: one step() in "initial" mode
        self._step_count = 0
        self._is_initial = True
        self.step()
        self._is_initial = False

    # ---- the group
    @property
    def lr(self) -> float:
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v: float):
        self.param_groups[0]["lr"] = v

    @property
    def initial_lr(self) -> float:
        return self.param_groups[0]["initial_lr"]

    def get_lr(self) -> List[float]:
        raise NotImplementedError

    def get_last_lr(self) -> List[float]:
        return self._last_lr

    def step(self) -> None:
        self._step_count += 1
        self.last_epoch += 1
        self._get_lr_called_within_step = True
        try:
            values = self.get_lr()
        finally:
            self._get_lr_called_within_step = False
        for group, v in zip(self.param_groups, values):
            group["lr"] = v
        self._last_lr = [group["lr"] for group in self.param_groups]

    def update(self, current_iter: int, warmup_iter: int = -1) -> float:
        """base_model.update_learning_rate: step from iteration 2 on, then the linear warm-up override of the
        group's lr while current_iter < warmup_iter.  Returns the lr iteration `current_iter` runs with."""
        if current_iter > 1:
            self.step()
        if current_iter < warmup_iter:
            for group in self.param_groups:
                group["lr"] = group["initial_lr"] / warmup_iter * current_iter
        return self.param_groups[0]["lr"]

    def state_dict(self) -> Dict[str, Any]:
        return {k: v for k, v in self.__dict__.items() if k != "param_groups"}

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        self.__dict__.update({k: v for k, v in state_dict.items() if k != "param_groups"})


class MultiStepRestartLR(_Scheduler):
    """At a restart iteration lr = initial_lr * weight; at a milestone lr = (current lr) * gamma ** (times listed)."""

    def __init__(self, milestones, gamma=0.1, restarts=(0,), restart_weights=(1,), last_epoch=-1, *, base_lr: float):
        self.milestones = Counter(milestones)
        self.gamma = gamma
        self.restarts = restarts
        self.restart_weights = restart_weights
        assert len(self.restarts) == len(self.restart_weights), "restarts and their weights do not match."
        super().__init__(base_lr, last_epoch)

    def get_lr(self):
        e = self.last_epoch
        if e in self.restarts:
            w = self.restart_weights[self.restarts.index(e)]
            return [g["initial_lr"] * w for g in self.param_groups]
        if e not in self.milestones:
            return [g["lr"] for g in self.param_groups]
        return [g["lr"] * self.gamma ** self.milestones[e] for g in self.param_groups]


class LinearLR(_Scheduler):
    """lr = (1 - last_epoch / total_iter) * initial_lr."""

    def __init__(self, total_iter, last_epoch=-1, *, base_lr: float):
        self.total_iter = total_iter
        super().__init__(base_lr, last_epoch)

    def get_lr(self):
        process = self.last_epoch / self.total_iter
        weight = 1 - process
        return [weight * g["initial_lr"] for g in self.param_groups]


class VibrateLR(_Scheduler):
    """A triangle wave of period total_iter // 80 under a piecewise envelope (1 -> 0 over the first 3/8 of the run,
    0.2 up to 5/8, then 0.1), floored at 0.1 during the first half period."""

    def __init__(self, total_iter, last_epoch=-1, *, base_lr: float):
        self.total_iter = total_iter
        super().__init__(base_lr, last_epoch)

    def get_lr(self):
        e = self.last_epoch
        process = e / self.total_iter
        if process < 3 / 8:
            envelope = 1 - process * 8 / 3
        elif process < 5 / 8:
            envelope = 0.2
        else:
            envelope = 0.1
        period = self.total_iter // 80
        half = period // 2
        t = e % period  # total_iter < 80: ZeroDivisionError, as in the reference
        wave = t / half  # total_iter < 160: ZeroDivisionError, as in the reference
        if t >= half:
            wave = 2 - wave
        weight = envelope * wave
        if e < half:
            weight = max(0.1, weight)
        return [weight * g["initial_lr"] for g in self.param_groups]


def get_position_from_periods(iteration, cumulative_period):
    """Index of the first cumulative period that is >= iteration; None past the last one."""
    for i, end in enumerate(cumulative_period):
        if iteration <= end:
            return i
    return None


class CosineAnnealingRestartLR(_Scheduler):
    """One cosine from weight * base_lr to eta_min per period; past the last period get_lr indexes with None."""

    def __init__(self, periods, restart_weights=(1,), eta_min=0, last_epoch=-1, *, base_lr: float):
        self.periods = periods
        self.restart_weights = restart_weights
        self.eta_min = eta_min
        assert len(self.periods) == len(self.restart_weights), \
            "periods and restart_weights should have the same length."
        self.cumulative_period = [sum(self.periods[0:i + 1]) for i in range(0, len(self.periods))]
        super().__init__(base_lr, last_epoch)

    def get_lr(self):
        idx = get_position_from_periods(self.last_epoch, self.cumulative_period)
        weight = self.restart_weights[idx]
        start = 0 if idx == 0 else self.cumulative_period[idx - 1]
        period = self.periods[idx]
        return [self.eta_min + weight * 0.5 * (base_lr - self.eta_min) *
                (1 + math.cos(math.pi * ((self.last_epoch - start) / period))) for base_lr in self.base_lrs]


class CosineAnnealingLR(_Scheduler):
    """torch.optim.lr_scheduler.CosineAnnealingLR, what setup_schedulers builds for `TrueCosineAnnealingLR`: the
    chained form, each lr computed from the group's current one."""

    def __init__(self, T_max, eta_min=0.0, last_epoch=-1, *, base_lr: float):
        self.T_max = T_max
        self.eta_min = eta_min
        super().__init__(base_lr, last_epoch)

    def get_lr(self):
        e, T = self.last_epoch, self.T_max
        if self._is_initial:
            return [g["lr"] for g in self.param_groups]
        if self._step_count == 1 and e > 0:
            return [self.eta_min + (base_lr - self.eta_min) * (1 + math.cos(e * math.pi / T)) / 2
                    for base_lr in self.base_lrs]
        if (e - 1 - T) % (2 * T) == 0:
            return [g["lr"] + (base_lr - self.eta_min) * (1 - math.cos(math.pi / T)) / 2
                    for base_lr, g in zip(self.base_lrs, self.param_groups)]
        return [(1 + math.cos(math.pi * e / T)) / (1 + math.cos(math.pi * (e - 1) / T)) * (g["lr"] - self.eta_min)
                + self.eta_min for g in self.param_groups]


def build_scheduler(train_opt: dict, base_lr: float) -> _Scheduler:
    """setup_schedulers' dispatch: pops 'type' from train_opt['scheduler'], as the reference does; LinearLR and
    VibrateLR take train_opt['total_iter'] and nothing from the scheduler dict."""
    scheduler_type = train_opt["scheduler"].pop("type")
    if scheduler_type in ["MultiStepLR", "MultiStepRestartLR"]:
        return MultiStepRestartLR(**train_opt["scheduler"], base_lr=base_lr)
    if scheduler_type == "CosineAnnealingRestartLR":
        return CosineAnnealingRestartLR(**train_opt["scheduler"], base_lr=base_lr)
    if scheduler_type == "TrueCosineAnnealingLR":
        return CosineAnnealingLR(**train_opt["scheduler"], base_lr=base_lr)
    if scheduler_type == "LinearLR":
        return LinearLR(train_opt["total_iter"], base_lr=base_lr)
    if scheduler_type == "VibrateLR":
        return VibrateLR(train_opt["total_iter"], base_lr=base_lr)
    raise NotImplementedError(f"Scheduler {scheduler_type} is not implemented yet.")


__all__ = ["MultiStepRestartLR", "CosineAnnealingRestartLR", "CosineAnnealingLR", "LinearLR", "VibrateLR",
           "get_position_from_periods", "build_scheduler"]
