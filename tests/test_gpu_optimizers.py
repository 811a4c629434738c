"""GPU tests of the optimizer kinds beyond plain AdamW: the nbp_adam_apply / nbp_sgd_apply kernels through the C-ABI
against torch.optim on the CPU, and NBPTrainer(optimizer=..., scheduler=<lr_scheduler object>, warmup_iter=...) with
its checkpoints.

Kernel tolerance.  Each case (kind, n) runs the same five steps three ways: the device, torch.optim in float64 on the
CPU (the reference: float32 gradients, float32-rounded lr, clip_grad_norm_ before every step) and torch.optim in float32
on the CPU.  For the parameters and for every optimizer buffer on its own, at every size, the device's largest element
error against float64 may be at most 4x torch-float32's own largest error on that tensor of that case: both are float32
evaluations of one formula with differently ordered roundings, each a few ulps of p per step.  One floor, from the
number format alone: an element also passes when it is within half a float32 ulp of the float64 value per applied step
(2.5 ulps after five steps, 2 after four).  Every applied step stores the tensor rounded to float32 once, so a perfect
evaluation of the formula can be that far off, while torch-float32's largest error over the one to four elements of the
small sizes is often a tenth of an ulp by chance (seen at n = 4, Adam with amsgrad: 1.4e-8 against the device's
1.05e-7 = 0.9 ulp, one rounding away in one element, a ratio of 7.5 between two correctly rounded results).  The floor
is at most 3e-7 absolute for |p| < 2; a missed or doubled element is off by 1e-4 or more.  Worst ratios measured on an
MI355X: see DESIGN 3k.

The one-pass capacity of the apply kernels is their grid cap x 256 threads x 4 elements = 2048 * 256 * 4 = 2097152
elements; N_BIG = 2097152 + 1027 lies above it with N_BIG % 4 == 3, so the grid-stride loop and the scalar tail both run.
"""
import collections
import functools

import pytest
import torch

from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

ONE_PASS = 2048 * 256 * 4
N_BIG = ONE_PASS + 1027
SIZES = [1, 3, 4, 1027, N_BIG]
STEPS = 5
BETAS = (0.9, 0.999)
EPS = 1e-8

# name -> (torch class, torch keywords); lr is set per step
KINDS = {
    "adam_wd0": ("Adam", dict(weight_decay=0.0)),
    "adam_l2": ("Adam", dict(weight_decay=0.01)),
    "adamw_amsgrad": ("AdamW", dict(weight_decay=0.01, amsgrad=True)),
    "adam_amsgrad": ("Adam", dict(weight_decay=0.01, amsgrad=True)),
    "sgd_plain": ("SGD", dict(weight_decay=0.01)),
    "sgd_momentum": ("SGD", dict(momentum=0.9, weight_decay=0.01)),
    "sgd_dampening": ("SGD", dict(momentum=0.9, dampening=0.1, weight_decay=0.01)),
    "sgd_nesterov": ("SGD", dict(momentum=0.9, nesterov=True, weight_decay=0.01)),
}
BUFFERS = {"Adam": ["exp_avg", "exp_avg_sq"], "AdamW": ["exp_avg", "exp_avg_sq"], "SGD": []}


def _buffer_names(kind):
    cls, kw = KINDS[kind]
    names = list(BUFFERS[cls])
    if kw.get("amsgrad"):
        names.append("max_exp_avg_sq")
    if kw.get("momentum"):
        names.append("momentum_buffer")
    return names


def _inputs(kind, n, bad_step=None):
    """Seeded parameters, five gradients with exact zeros and step-dependent scales, float32-rounded lrs, and a
    max_norm equal to the median gradient norm (so the clip coefficient is below 1 on some steps and 1 on others).
    |p| in [0.5, 2): the errors under test are ulps of p.  `bad_step` (0-based) gets one inf."""
    g = torch.Generator().manual_seed(1000 * len(kind) + n % 9973 + sum(map(ord, kind)))
    p0 = (0.5 + 1.5 * torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    scales = [1.0, 3.0, 0.5, 2.0, 0.7]
    grads = []
    for k in range(STEPS):
        gr = 0.01 * scales[k] * torch.randn(n, generator=g)
        if n > 4:
            gr[k::7] = 0.0
        elif k == 3:
            gr[0] = 0.0  # tiny sizes: one exact zero, at step 4
        grads.append(gr)
    base = 0.05 if KINDS[kind][0] == "SGD" else 1e-3
    lrs = [float(torch.tensor(base * f, dtype=torch.float32)) for f in (1.0, 0.8, 0.8, 0.4, 0.25)]
    norms = sorted(float(gr.double().norm()) for gr in grads)
    max_norm = norms[len(norms) // 2]
    if bad_step is not None:
        grads[bad_step][n // 2] = float("inf")
    return p0, grads, lrs, max_norm


def _torch_run(kind, p0, grads, lrs, max_norm, dtype):
    """clip_grad_norm_ + torch.optim on the CPU in `dtype`; a non-finite gradient's step is never seen (scaler.step's
    skip).  Returns the state {name: tensor} and the clip coefficients."""
    cls, kw = KINDS[kind]
    p = torch.nn.Parameter(p0.to(dtype).clone())
    extra = dict(betas=BETAS, eps=EPS) if cls != "SGD" else {}
    opt = getattr(torch.optim, cls)([p], lr=lrs[0], **extra, **kw)
    coefs = []
    for gr, lr in zip(grads, lrs):
        if not torch.isfinite(gr).all():
            continue
        p.grad = gr.to(dtype).clone()
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        coefs.append(min(1.0, max_norm / (float(total) + 1e-6)))
        opt.param_groups[0]["lr"] = lr
        opt.step()
    out = {"param": p.detach().clone()}
    for name in _buffer_names(kind):
        out[name] = opt.state[p][name].detach().clone()
    return out, coefs


def _max_err(state, ref64):
    return {k: (state[k].cpu().double() - ref64[k]).abs().max().item() for k in ref64}


@functools.lru_cache(maxsize=None)
def _cpu_small(kind, n, bad_step=None):
    """Inputs, the float64 reference and torch-float32's errors of a case with n <= 1027, computed once."""
    p0, grads, lrs, max_norm = _inputs(kind, n, bad_step)
    ref64, coefs = _torch_run(kind, p0, grads, lrs, max_norm, torch.float64)
    ref32, _ = _torch_run(kind, p0, grads, lrs, max_norm, torch.float32)
    return (p0, grads, lrs, max_norm), ref64, coefs, ref32


def _cpu(kind, n, bad_step=None):
    if n <= 1027:
        return _cpu_small(kind, n, bad_step)
    return _cpu_small.__wrapped__(kind, n, bad_step)


class _Device:
    """The flat buffers and the nbp_optim_prepare + apply sequence of one kind."""

    def __init__(self, kind, p0, max_norm, dev):
        from lowlight_image_enhancement_amd._lib import query
        self.kind, self.max_norm = kind, max_norm
        n = self.n = p0.numel()
        self.t = {"param": p0.to(dev).clone()}
        for name in _buffer_names(kind):
            self.t[name] = torch.zeros(n, device=dev)
        self.state = torch.zeros(8, device=dev)
        self.ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        self.lr = torch.zeros(1, device=dev)
        self.ws = torch.empty(query("clip_workspace_doubles", n), dtype=torch.float64, device=dev)

    def step(self, grad, lr):
        from lowlight_image_enhancement_amd._lib import call
        cls, kw = KINDS[self.kind]
        self.lr.fill_(lr)
        call("optim_prepare", grad, self.n, 1.0, float(self.max_norm), self.ws, self.lr, BETAS[0], BETAS[1],
             self.state, self.ctl, None, None, None, 0)
        t = self.t
        if cls == "SGD":
            call("sgd_apply", t["param"], grad, t.get("momentum_buffer"), self.n, self.state, self.ctl,
                 float(kw.get("momentum", 0.0)), float(kw.get("dampening", 0.0)), float(kw["weight_decay"]),
                 int(kw.get("nesterov", False)))
        else:
            call("adam_apply", t["param"], grad, t["exp_avg"], t["exp_avg_sq"], t.get("max_exp_avg_sq"), self.n,
                 self.state, BETAS[0], BETAS[1], EPS, float(kw["weight_decay"]), int(cls == "AdamW"))

    def snapshot(self):
        return {k: v.clone() for k, v in self.t.items()}


def _ulp32(x64):
    """The float32 spacing at each value of a float64 tensor."""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _compare(tag, dev_state, ref64, ref32, applied=STEPS):
    """The bound of the module docstring, per tensor: every element within 4x torch-float32's largest error on that
    tensor, or within applied / 2 float32 ulps of the float64 value.  Prints the ratios before asserting."""
    e_f32 = _max_err(ref32, ref64)
    e_dev, per, bad = {}, {}, {}
    for k in ref64:
        assert torch.isfinite(dev_state[k]).all(), (tag, k)
        err = (dev_state[k].cpu().double() - ref64[k]).abs()
        e_dev[k] = err.max().item()
        per[k] = e_dev[k] / e_f32[k] if e_f32[k] > 0 else (0.0 if e_dev[k] == 0 else float("inf"))
        ok = (err <= 4.0 * e_f32[k]) | (err <= 0.5 * applied * _ulp32(ref64[k]))
        bad[k] = int((~ok).sum())
    worst_dev, worst_f32 = max(e_dev.values()), max(e_f32.values())
    ratio = worst_dev / worst_f32 if worst_f32 > 0 else (0.0 if worst_dev == 0 else float("inf"))
    print(f"{tag}: device max err {worst_dev:.3e}, torch-f32 max err {worst_f32:.3e}, ratio {ratio:.3f}; per tensor "
          + ", ".join(f"{k} {v:.3f}" for k, v in per.items()))
    assert not any(bad.values()), (tag, bad, per, e_dev, e_f32)
    return ratio


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_apply_kernels_match_torch_optim(dev, kind, n):
    (p0, grads, lrs, max_norm), ref64, coefs, ref32 = _cpu(kind, n)
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs  # the clip engages on some steps only
    assert all((gr == 0).any() for gr in grads) if n > 4 else (grads[3] == 0).any()
    d = _Device(kind, p0, max_norm, dev)
    for gr, lr in zip(grads, lrs):
        d.step(gr.to(dev), lr)
    ctl = d.ctl.cpu().tolist()
    assert ctl[0] == STEPS and ctl[2] == 0
    assert ctl[3] == int("momentum_buffer" in d.t)  # set by the first applied step of SGD with momentum only
    assert float(d.state[5]) == lrs[-1]
    _compare(f"{kind} n={n}", d.t, ref64, ref32)


# every kind with the inf at step 2: the tail alone (3), the vector body with the tail (1027); above one pass for some
SKIP_CASES = [(k, n, 1) for k in KINDS for n in (3, 1027)]
SKIP_CASES += [(k, N_BIG, 1) for k in ("adam_l2", "adamw_amsgrad", "sgd_plain", "sgd_momentum", "sgd_nesterov")]
# SGD with momentum: the inf at step 1, so the first-step copy is deferred to step 2
SKIP_CASES += [(k, n, 0) for k in ("sgd_momentum", "sgd_dampening", "sgd_nesterov") for n in (3, 1027)]


@pytest.mark.parametrize("kind,n,bad", SKIP_CASES)
def test_non_finite_gradient_skips_the_step(dev, kind, n, bad):
    """One inf in the gradient of step bad + 1: that step leaves the parameters and every buffer bitwise untouched and
    does not advance ctl[0]; the final state is that of a float64 run that never saw the step."""
    (p0, grads, lrs, max_norm), ref64, _, ref32 = _cpu(kind, n, bad)
    d = _Device(kind, p0, max_norm, dev)
    has_buf = "momentum_buffer" in d.t
    for k, (gr, lr) in enumerate(zip(grads, lrs)):
        before, ctl_before = d.snapshot(), d.ctl.cpu().tolist()
        d.step(gr.to(dev), lr)
        ctl = d.ctl.cpu().tolist()
        if k == bad:
            for name, v in before.items():
                assert torch.equal(v.view(torch.int32), d.t[name].view(torch.int32)), (kind, name)
            assert float(d.state[2]) == 1.0
            assert ctl[0] == ctl_before[0] and ctl[2] == ctl_before[2] + 1 and ctl[3] == ctl_before[3]
        else:
            assert float(d.state[2]) == 0.0 and ctl[0] == ctl_before[0] + 1
            assert ctl[3] == int(has_buf)
            if has_buf and ctl_before[3] == 0:  # the first applied step copies the clipped, decayed gradient
                kw = KINDS[kind][1]
                want = gr.to(dev) * d.state[1] + kw["weight_decay"] * before["param"]
                # (no dampening); values ~0.01, compared to an ulp of that: the two terms may cancel
                assert torch.allclose(d.t["momentum_buffer"], want, rtol=1e-6, atol=2e-9)
    assert d.ctl.cpu().tolist()[0] == STEPS - 1
    _compare(f"{kind} n={n} inf at step {bad + 1}", d.t, ref64, ref32, applied=STEPS - 1)


# ---------------------------------------------------------------------------------------------------- trainer
CFG = dict(width=8, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])


def _net(dev, precision="fp32", seed=71):
    from param_recipe import recipe_state
    from lowlight_image_enhancement_amd.NewBP_model.newbp_net_arch import create_newbp_net
    net = create_newbp_net(in_channels=3, kernel_type="rgb", kernel_spec="B2", **CFG)
    net.load_state_dict(recipe_state([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed))
    net = net.to(dev)
    net.precision = precision
    return net


def _batch(dev, seed=17):
    gen = torch.Generator(device=dev).manual_seed(seed)
    lq, gt = (torch.rand(2, 3, 32, 32, device=dev, generator=gen) for _ in range(2))
    r = torch.ones(2, 1, 1, 1, device=dev)
    return lq, gt, (lq * r).clamp(0, 1), r


def _spec(name):
    from lowlight_image_enhancement_amd.optim import SGD, Adam
    if name == "sgd":
        return SGD(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4)
    if name == "sgd_momentum":
        return SGD(lr=0.05, momentum=0.9, weight_decay=1e-4)
    return Adam(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.01, amsgrad=True)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def test_adamw_spec_is_bitwise_the_default_trainer(dev):
    from lowlight_image_enhancement_amd.optim import AdamW
    from lowlight_image_enhancement_amd.train import NBPTrainer
    a = NBPTrainer(_net(dev))
    b = NBPTrainer(_net(dev), optimizer=AdamW(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01))
    assert b.max_exp_avg_sq is None and b.momentum_buffer is None and a.optimizer is None
    for s in range(3):
        batch = _batch(dev, 17 + s)
        a.step(*batch)
        b.step(*batch)
    assert torch.equal(a.net.flat.data, b.net.flat.data)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.opt_state, b.opt_state) and torch.equal(a.ctl, b.ctl) and a.t == 3


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["sgd", "adam_amsgrad"])
def test_graph_step_is_bitwise_step(dev, name, precision):
    """Four steps with MultiStepRestartLR(milestones=[2], gamma=0.5) and warmup_iter=2 (the lr moves inside the run);
    fp16 with a dynamic loss scale that grows every second step.  opt_state[5] is the float32 of the host schedule."""
    from lowlight_image_enhancement_amd.lr_scheduler import MultiStepRestartLR
    from lowlight_image_enhancement_amd.train import NBPTrainer
    spec = _spec(name)
    host = MultiStepRestartLR(milestones=[2], gamma=0.5, base_lr=spec.lr)
    want = [_f32(host.update(i, 2)) for i in range(1, 5)]
    assert len(set(want)) >= 2, want
    res = {}
    for mode in ("step", "graph_step"):
        kw = dict(init_scale=2.0 ** 12, growth_interval=2) if precision == "fp16" else {}
        tr = NBPTrainer(_net(dev, precision), optimizer=_spec(name), warmup_iter=2,
                        scheduler=MultiStepRestartLR(milestones=[2], gamma=0.5, base_lr=spec.lr), **kw)
        assert (tr.scaler is not None) == (precision == "fp16")
        if name == "sgd":
            assert tr.exp_avg is None and tr.exp_avg_sq is None and tr.max_exp_avg_sq is None
            assert tr.momentum_buffer is not None
        else:
            assert tr.momentum_buffer is None and tr.max_exp_avg_sq is not None
        lrs = []
        for s in range(4):
            getattr(tr, mode)(*_batch(dev, 17 + s))
            lrs.append(float(tr.opt_state[5]))
        assert lrs == want, (mode, lrs, want)
        res[mode] = ([tr.net.flat.data.clone()] + [b.clone() for b in tr._opt_buffers()], tr.ctl.clone(),
                     tr.opt_state.clone(), None if tr.scaler is None else tr.scaler.clone(), tr.logs())
    a, b = res["step"], res["graph_step"]
    assert len(a[0]) == (2 if name == "sgd" else 4)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert int(a[1][0]) + int(a[1][2]) == 4  # applied + skipped steps
    if precision == "fp16":
        assert torch.equal(a[3], b[3]) and float(a[3][0]) != 2.0 ** 12
    assert a[4] == b[4]
    assert not torch.equal(a[0][0], _net(dev, precision).flat.data)  # the parameters moved


def test_momentumless_sgd_step_matches_the_module_path(dev):
    """One step of SGD(momentum=0) in the trainer against the same net under autograd, clip_grad_norm_(0.01) and
    torch.optim.SGD([net.flat]): the update p_after - p_before matches norm-wise within 1e-5 + 1e-6 (1e-5: the
    gradient bound test_gpu_pixel_trainer.py holds for this network; the rest: the float32 clip coefficient).
    lr = 50 with max_norm = 0.01 gives an update of norm 0.5 over 19899 parameters of magnitude ~0.17, i.e. elements
    ~1e5 ulps of p: the rounding of p_after itself, which is no part of the bound, stays far below it."""
    from lowlight_image_enhancement_amd.optim import SGD
    from lowlight_image_enhancement_amd.pixel_losses import L1Loss
    from lowlight_image_enhancement_amd.train import NBPTrainer
    lq, gt, _, _ = _batch(dev)
    tr = NBPTrainer(_net(dev), pixel_loss=L1Loss(1.0, "mean"), w_l1=0.0, w_ssim=0.0, w_phys=0.0, max_norm=0.01,
                    optimizer=SGD(lr=50.0))
    assert not tr._opt_buffers()  # momentum-less SGD keeps no state
    before = tr.net.flat.data.clone()
    tr.step(lq, gt)
    upd = (tr.net.flat.data - before).double()
    assert float(tr.opt_state[1]) < 1.0  # the clip engaged

    net = _net(dev)
    ref_before = net.flat.detach().clone()
    L1Loss(1.0, "mean")(net(lq), gt).backward()
    torch.nn.utils.clip_grad_norm_([net.flat], 0.01)
    torch.optim.SGD([net.flat], lr=50.0).step()
    ref = (net.flat.detach() - ref_before).double()
    rel = ((upd - ref).norm() / ref.norm()).item()
    print(f"momentum-less SGD update: norm {ref.norm().item():.4f}, norm-wise rel err {rel:.3e}")
    assert torch.equal(before, ref_before) and ref.norm().item() > 0.4
    assert rel <= 1e-5 + 1e-6, rel


@pytest.mark.parametrize("name", ["sgd_momentum", "adam_amsgrad"])
def test_checkpoint_is_torch_form_and_resumes_bitwise(dev, tmp_path, name):
    """save_training_state after 2 steps (inside the warm-up, two steps before a milestone): the optimizer entry has
    exactly torch's keys and loads into the matching torch.optim object; a fresh trainer resumed from the files
    continues bit for bit for 2 more steps, lr included."""
    from lowlight_image_enhancement_amd import checkpoint as ck
    from lowlight_image_enhancement_amd.lr_scheduler import MultiStepRestartLR
    from lowlight_image_enhancement_amd.train import NBPTrainer

    def trainer():
        spec = _spec(name)
        return NBPTrainer(_net(dev), optimizer=spec, warmup_iter=3,
                          scheduler=MultiStepRestartLR(milestones=[3], gamma=0.5, base_lr=spec.lr))

    a = trainer()
    fresh = ck.optimizer_state_dict(a)
    if name == "sgd_momentum":
        assert fresh["state"] == {}  # no momentum_buffer before the first applied step
    for s in range(2):
        a.step(*_batch(dev, 17 + s))
    ck.save_network(a.net, str(tmp_path / "net_g_2.pth"))
    path = ck.save_training_state(a, 0, 2, str(tmp_path))
    with torch.serialization.safe_globals([collections.Counter]):
        state = torch.load(path, map_location="cpu", weights_only=True)
    entry = state["optimizers"][0]
    assert isinstance(state["schedulers"][0]["milestones"], collections.Counter)
    assert state["schedulers"][0]["last_epoch"] == 1

    # torch's own object over state_dict()-shaped CPU parameters, with a scheduler attached (initial_lr)
    net = a.net
    params = [torch.nn.Parameter(v.detach().cpu().clone()) for v in net.state_dict().values()]
    spec = _spec(name)
    opt = spec.torch_cls(params, **spec.torch_kwargs())
    torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0)
    for p in params:
        p.grad = torch.zeros_like(p)
    opt.step()
    own = opt.state_dict()
    assert set(entry["param_groups"][0]) == set(own["param_groups"][0])
    assert entry["param_groups"][0]["params"] == own["param_groups"][0]["params"]
    assert set(entry["state"]) == set(own["state"])
    assert set(entry["state"][0]) == set(own["state"][0])
    assert entry["param_groups"][0]["lr"] == spec.lr / 3 * 2 and entry["param_groups"][0]["initial_lr"] == spec.lr
    opt.load_state_dict(entry)
    bufs = {"sgd_momentum": [("momentum_buffer", a.momentum_buffer)],
            "adam_amsgrad": [("exp_avg", a.exp_avg), ("exp_avg_sq", a.exp_avg_sq),
                             ("max_exp_avg_sq", a.max_exp_avg_sq)]}[name]
    for i, k in enumerate(net.state_dict()):
        e = net.entries[k]
        for key, flat in bufs:
            assert torch.equal(opt.state[params[i]][key], net._to_reference(e, flat[e.offset:e.offset + e.numel]).cpu())
        if name == "adam_amsgrad":
            assert float(opt.state[params[i]]["step"]) == 2.0

    c = trainer()
    ck.load_network(c.net, str(tmp_path / "net_g_2.pth"))
    ck.resume_training(c, path)
    assert c.iter == 2 and c.scheduler.last_epoch == 1 and c.scheduler.lr == a.scheduler.lr
    for s in range(2, 4):
        batch = _batch(dev, 17 + s)
        a.step(*batch)
        c.step(*batch)
        assert float(c.opt_state[5]) == float(a.opt_state[5])
    # iteration 4 stands at the milestone (last_epoch 3): it halves the lr the warm-up wrote at iteration 2, which only
    # the restored group lr carries
    assert float(a.opt_state[5]) == _f32(_spec(name).lr / 3 * 2 * 0.5)
    assert torch.equal(c.net.flat.data, a.net.flat.data)
    for x, y in zip(c._opt_buffers(), a._opt_buffers()):
        assert torch.equal(x, y)
    # the growth tracker, the skip count and the buffer flag; the step count too where torch keeps one (SGD's state
    # has no 'step', and its update does not read ctl[0])
    assert torch.equal(c.ctl[1:], a.ctl[1:]) and (name == "sgd_momentum" or int(c.ctl[0]) == int(a.ctl[0]) == 4)


def test_from_train_opt(dev):
    from lowlight_image_enhancement_amd import lr_scheduler as LS
    from lowlight_image_enhancement_amd import optim as O
    from lowlight_image_enhancement_amd.pixel_losses import L1Loss
    from lowlight_image_enhancement_amd.train import NBPTrainer
    train_opt = dict(optim_g=dict(type="Adam", lr=2e-4, weight_decay=0, betas=[0.9, 0.9]),
                     scheduler=dict(type="MultiStepLR", milestones=[5], gamma=0.5), total_iter=100, warmup_iter=3,
                     use_grad_clip=False, pixel_opt=dict(type="L1Loss", loss_weight=1.0, reduction="mean"))
    keep = repr(train_opt)
    tr = NBPTrainer.from_train_opt(_net(dev), train_opt)
    assert repr(train_opt) == keep  # the caller's dict keeps its 'type' entries
    assert isinstance(tr.optimizer, O.Adam) and (tr.lr, tr.betas, tr.wd) == (2e-4, (0.9, 0.9), 0.0)
    assert isinstance(tr.scheduler, LS.MultiStepRestartLR) and tr.scheduler.base_lrs == [2e-4]
    assert tr.warmup_iter == 3 and tr.max_norm == 0.0 and isinstance(tr.pixel_loss, L1Loss)
    assert tr.w == (0.0, 0.0, 0.0)
    lq, gt, _, _ = _batch(dev)
    tr.step(lq, gt)
    assert float(tr.opt_state[5]) == _f32(2e-4 / 3 * 1) and float(tr.opt_state[1]) == 1.0 and tr.t == 1
    sgd = NBPTrainer.from_train_opt(_net(dev), dict(optim_g=dict(type="SGD", lr=0.1, momentum=0.9)), w_phys=0.0)
    assert isinstance(sgd.optimizer, O.SGD) and sgd.max_norm == 0.01 and sgd.scheduler is None
    assert sgd.warmup_iter == -1 and sgd.w[2] == 0.0
    with pytest.raises(NotImplementedError, match="optimizer Lion is not supperted yet."):
        NBPTrainer.from_train_opt(_net(dev), dict(optim_g=dict(type="Lion", lr=0.1)))
    with pytest.raises(TypeError):
        NBPTrainer(_net(dev), optimizer=torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1))
