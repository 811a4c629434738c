"""CPU tests of lr_scheduler.py and optim.py: the schedules of base_model.setup_schedulers with the warm-up of
update_learning_rate, against golden/lr_schedules.npz (the reference's own classes driven by a torch optimizer,
tests/golden/make_golden_lr_schedules.py), and the options-level builders.

Equality is exact: the classes perform the reference's float64 operations in the reference's order, so they return the
same Python floats.  No case needed a 1-ulp allowance."""
import collections
from copy import deepcopy

import numpy as np
import pytest
import torch

from conftest import golden

import lr_schedule_fixtures as F
from lowlight_image_enhancement_amd import lr_scheduler as LS
from lowlight_image_enhancement_amd import optim as O


@pytest.fixture(scope="module")
def gold():
    return golden("lr_schedules.npz")


def _run(name, upto=None):
    opt, lr, n = F.train_opt(name)
    s = LS.build_scheduler(opt, lr)
    w = opt.get("warmup_iter", -1)
    return s, w, [s.update(i, w) for i in range(1, (upto or n) + 1)]


@pytest.mark.parametrize("name", list(F.CASES))
def test_schedule_is_the_reference_sequence(gold, name):
    s, _, out = _run(name)
    ref = gold[name]
    assert len(out) == len(ref) <= 200
    assert all(type(v) is float for v in out)
    got = np.asarray(out, dtype=np.float64)
    bad = np.nonzero(got.view(np.uint64) != ref.view(np.uint64))[0]
    assert bad.size == 0, (name, bad[:5], got[bad[:5]], ref[bad[:5]])
    # the scheduler's own state after the run, and the keys of its state_dict()
    last_epoch, step_count, last_lr = gold[name + "__final"]
    assert (s.last_epoch, s._step_count) == (int(last_epoch), int(step_count))
    assert np.float64(s.get_last_lr()[0]).view(np.uint64) == np.float64(last_lr).view(np.uint64)
    assert sorted(s.state_dict()) == gold[name + "__keys"].tolist()


def test_schedules_move_as_described(gold):
    """The two semantics a closed form would lose, read off the reference's numbers."""
    r = gold["ms_repeat"]
    assert r[19] == 3.7e-4 and r[20] == 3.7e-4 * 0.3 ** 2  # the milestone 20 is listed twice
    w = gold["ms_restart_warm15"]
    assert w[13] == 5e-4 / 15 * 14
    assert w[14] == w[13] and w[29] == w[13]  # the schedule continues from what the warm-up last wrote
    assert w[30] == w[13] * 0.5 ** 2 and w[40] == 5e-4 * 0.5  # milestone 30 twice, then the restart at 40


# (case, iteration the state is taken at): inside a warm-up, and after a milestone
@pytest.mark.parametrize("name,at", [("ms_restart_warm15", 7), ("ms_restart_warm15", 33), ("ms_repeat", 25),
                                     ("cosine_warm10", 4), ("cosine", 60), ("cos_restart_warm4", 13),
                                     ("vibrate_400_warm8", 5)])
def test_resume_from_state_dict_continues_the_sequence(gold, name, at):
    s, w, _ = _run(name, upto=at)
    sd, lr = deepcopy(s.state_dict()), s.lr  # the group's lr is optimizer state, as in torch
    assert "param_groups" not in sd and sd["last_epoch"] == at - 1
    opt, base, n = F.train_opt(name)
    fresh = LS.build_scheduler(opt, base)
    fresh.load_state_dict(sd)
    fresh.lr = lr
    out = [fresh.update(i, w) for i in range(at + 1, n + 1)]
    assert np.array_equal(np.asarray(out).view(np.uint64), gold[name][at:].view(np.uint64))


def test_state_dict_holds_the_reference_attributes():
    s = LS.MultiStepRestartLR([3, 3, 5], gamma=0.5, base_lr=1e-3)
    sd = s.state_dict()
    assert isinstance(sd["milestones"], collections.Counter) and sd["milestones"] == {3: 2, 5: 1}
    assert sd["base_lrs"] == [1e-3] and sd["last_epoch"] == 0 and sd["_step_count"] == 1 and sd["_last_lr"] == [1e-3]
    assert s.param_groups[0] == {"lr": 1e-3, "initial_lr": 1e-3}


def test_reference_errors():
    for total in (159, 100, 79):  # period // 2 == 0 (or period == 0): the reference divides by zero, at construction
        with pytest.raises(ZeroDivisionError):
            LS.VibrateLR(total, base_lr=1e-3)
        with pytest.raises(ZeroDivisionError):
            LS.build_scheduler(dict(scheduler=dict(type="VibrateLR"), total_iter=total), 1e-3)
    LS.VibrateLR(160, base_lr=1e-3)
    s, w, _ = _run("cos_restart")  # 31 iterations: last_epoch 30, the end of the last period
    with pytest.raises(TypeError):  # restart_weights[None]
        s.update(32, w)
    assert LS.get_position_from_periods(31, [10, 20, 30]) is None
    assert [LS.get_position_from_periods(i, [100, 200, 300, 400]) for i in (50, 210, 300)] == [0, 2, 2]
    with pytest.raises(AssertionError, match="restarts and their weights do not match"):
        LS.MultiStepRestartLR([1], restarts=[0, 5], restart_weights=[1], base_lr=1e-3)
    with pytest.raises(AssertionError, match="periods and restart_weights should have the same length"):
        LS.CosineAnnealingRestartLR([10, 10], restart_weights=[1], base_lr=1e-3)


def test_build_scheduler_dispatch():
    kinds = {"MultiStepLR": LS.MultiStepRestartLR, "MultiStepRestartLR": LS.MultiStepRestartLR,
             "CosineAnnealingRestartLR": LS.CosineAnnealingRestartLR, "TrueCosineAnnealingLR": LS.CosineAnnealingLR,
             "LinearLR": LS.LinearLR, "VibrateLR": LS.VibrateLR}
    args = {"MultiStepLR": dict(milestones=[5]), "MultiStepRestartLR": dict(milestones=[5]),
            "CosineAnnealingRestartLR": dict(periods=[10]), "TrueCosineAnnealingLR": dict(T_max=10)}
    for kind, cls in kinds.items():
        opt = dict(scheduler=dict(type=kind, **args.get(kind, {})), total_iter=400)
        s = LS.build_scheduler(opt, 2e-4)
        assert type(s) is cls and s.base_lrs == [2e-4] and s.last_epoch == 0 and s.initial_lr == 2e-4
        assert s.lr == (2e-4 if cls is not LS.VibrateLR else 0.1 * 2e-4)  # VibrateLR starts at its 0.1 floor
        assert "type" not in opt["scheduler"]  # popped, as setup_schedulers does
    assert LS.build_scheduler(dict(scheduler=dict(type="LinearLR"), total_iter=123), 1.0).total_iter == 123
    d = LS.build_scheduler(dict(scheduler=dict(type="MultiStepLR", milestones=[5])), 1.0)
    assert (d.gamma, d.restarts, d.restart_weights) == (0.1, (0,), (1,))
    c = LS.build_scheduler(dict(scheduler=dict(type="CosineAnnealingRestartLR", periods=[4])), 1.0)
    assert (c.restart_weights, c.eta_min, c.cumulative_period) == ((1,), 0, [4])
    assert LS.build_scheduler(dict(scheduler=dict(type="TrueCosineAnnealingLR", T_max=7)), 1.0).eta_min == 0.0
    with pytest.raises(NotImplementedError, match="Scheduler StepLR is not implemented yet."):
        LS.build_scheduler(dict(scheduler=dict(type="StepLR")), 1.0)
    with pytest.raises(KeyError):  # Linear / Vibrate read train_opt['total_iter']
        LS.build_scheduler(dict(scheduler=dict(type="LinearLR")), 1.0)


def test_build_optimizer_dispatch_defaults_and_messages():
    a = O.build_optimizer(dict(type="Adam", lr=2e-4))
    w = O.build_optimizer(dict(type="AdamW", lr=5e-4, betas=[0.9, 0.99], weight_decay=0.02))
    s = O.build_optimizer(dict(type="SGD", lr=0.1, momentum=0.9, nesterov=True))
    assert (type(a), type(w), type(s)) == (O.Adam, O.AdamW, O.SGD)
    # defaults are the installed torch's
    p = [torch.nn.Parameter(torch.zeros(1))]
    for spec, cls in ((O.Adam(), torch.optim.Adam), (O.AdamW(), torch.optim.AdamW), (O.SGD(), torch.optim.SGD)):
        ref = cls(p).state_dict()["param_groups"][0]
        ref.pop("params")
        assert spec.param_group() == ref
        for k, v in spec.kwargs.items():  # every keyword of the class, at torch's default
            assert getattr(spec, k) == v == ref[k], k
    assert (a.lr, a.weight_decay, a.amsgrad, a.decoupled, a.plain_adamw) == (2e-4, 0, False, False, False)
    assert (w.weight_decay, w.decoupled, w.plain_adamw) == (0.02, True, True)
    assert not O.AdamW(amsgrad=True).plain_adamw and O.Adam(decoupled_weight_decay=True).plain_adamw
    assert (s.momentum, s.dampening, s.nesterov, s.kind, a.kind) == (0.9, 0, True, "sgd", "adam")
    opt = dict(type="SGD", lr=0.1)
    O.build_optimizer(opt)
    assert "type" not in opt  # popped, as setup_optimizers does
    with pytest.raises(NotImplementedError, match="optimizer RMSprop is not supperted yet."):
        O.build_optimizer(dict(type="RMSprop", lr=1e-3))
    # torch's own argument errors, at construction
    for cls, kw, msg in ((O.Adam, dict(lr=-1.0), "Invalid learning rate: -1.0"),
                         (O.AdamW, dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0: 1.0"),
                         (O.Adam, dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1: -0.1"),
                         (O.Adam, dict(eps=-1e-8), "Invalid epsilon value: -1e-08"),
                         (O.AdamW, dict(weight_decay=-0.1), "Invalid weight_decay value: -0.1"),
                         (O.SGD, dict(lr=-0.1), "Invalid learning rate: -0.1"),
                         (O.SGD, dict(momentum=-0.5), "Invalid momentum value: -0.5"),
                         (O.SGD, dict(weight_decay=-1.0), "Invalid weight_decay value: -1.0"),
                         (O.SGD, dict(nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
                         (O.SGD, dict(nesterov=True, momentum=0.9, dampening=0.1),
                          "Nesterov momentum requires a momentum and zero dampening")):
        with pytest.raises(ValueError, match=msg):
            cls(**kw)
    for cls in (O.Adam, O.AdamW, O.SGD):
        with pytest.raises(NotImplementedError):
            cls(maximize=True)
        with pytest.raises(TypeError):
            cls(rho=0.9)
    # implementation selectors: accepted, no numerical meaning
    O.Adam(foreach=True, capturable=True, differentiable=False)
    O.AdamW(fused=True)
    O.SGD(foreach=False, fused=None)


def test_install_aliases_registers_the_scheduler_module():
    import sys
    import lowlight_image_enhancement_amd as pkg
    pkg.install_aliases()
    assert sys.modules["basicsr.models.lr_scheduler"] is LS


class _FlatState:
    """The surface of NBPTrainer that checkpoint.py touches, with flat AdamW buffers on the CPU."""

    def __init__(self, net, it, scheduler=None, warmup_iter=-1, lr=5e-4):
        self.net, self.t, self.lr, self.betas, self.eps, self.wd = net, it, lr, (0.9, 0.999), 1e-8, 0.01
        self.exp_avg, self.exp_avg_sq = torch.zeros(net.numel), torch.zeros(net.numel)
        self.iter, self.scaler, self.scheduler, self.warmup_iter = it, None, scheduler, warmup_iter


def test_checkpoint_lr_inside_a_warmup_and_initial_lr_on_resume(tmp_path):
    from lowlight_image_enhancement_amd import checkpoint as ck
    from lowlight_image_enhancement_amd.NewBP_model.newbp_net_arch import create_newbp_net
    net = create_newbp_net(in_channels=3, width=8, enc_blk_nums=[1], middle_blk_num=1, dec_blk_nums=[1])
    # a default trainer (no spec) inside its warm-up writes the lr the iteration ran with; outside it, what it always wrote
    assert ck.adamw_state_dict(_FlatState(net, 3, warmup_iter=10))["param_groups"][0]["lr"] == 5e-4 / 10 * 3
    assert ck.adamw_state_dict(_FlatState(net, 3))["param_groups"][0]["lr"] == 5e-4
    assert ck.adamw_state_dict(_FlatState(net, 12, warmup_iter=10))["param_groups"][0]["lr"] == 5e-4
    # a stateful scheduler resumed into a trainer configured with another lr takes the file's initial_lr
    a = _FlatState(net, 0, LS.MultiStepRestartLR([4], gamma=0.5, restarts=[0, 6], restart_weights=[1, 0.5],
                                                base_lr=5e-4), warmup_iter=3)
    seq = []
    for i in range(1, 9):
        a.iter = a.t = i
        seq.append(a.scheduler.update(i, 3))
        if i == 2:
            path = ck.save_training_state(a, 0, 2, str(tmp_path))
    b = _FlatState(net, 0, LS.MultiStepRestartLR([4], gamma=0.5, restarts=[0, 6], restart_weights=[1, 0.5],
                                                base_lr=1e-3), warmup_iter=3, lr=1e-3)
    ck.resume_training(b, path)
    assert b.iter == 2 and b.lr == 5e-4 and b.scheduler.initial_lr == 5e-4 and b.scheduler.base_lrs == [5e-4]
    assert [b.scheduler.update(i, 3) for i in range(3, 9)] == seq[2:]
    assert seq[6] == 5e-4 * 0.5  # the restart at last_epoch 6 multiplies initial_lr
