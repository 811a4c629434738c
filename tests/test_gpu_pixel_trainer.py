"""GPU tests of NBPTrainer(pixel_loss=...): the reference's cri_pix term (image_restoration_model.py:264-269) inside
the fused training step.  A width-8 [1,1,1,1] / 1 / [1,1,1,1] network at 2 x 3 x 32 x 32.  The loss modules' own values
and gradients are pinned to the reference by test_gpu_pixel_losses.py; here the trainer's fused launch is compared
with the module path (net(lq) under autograd -> the same loss module -> backward())."""
import pytest
import torch

from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = dict(width=8, enc_blk_nums=[1, 1, 1, 1], middle_blk_num=1, dec_blk_nums=[1, 1, 1, 1])


def _net(dev, precision="fp32", seed=71):
    from param_recipe import recipe_state
    from lowlight_image_enhancement_amd.NewBP_model.newbp_net_arch import create_newbp_net
    net = create_newbp_net(in_channels=3, kernel_type="rgb", kernel_spec="B2", **CFG)
    net.load_state_dict(recipe_state([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed))
    net = net.to(dev)
    net.precision = precision
    return net


def _batch(dev):
    gen = torch.Generator(device=dev).manual_seed(17)
    return tuple(torch.rand(2, 3, 32, 32, device=dev, generator=gen) for _ in range(2))


def _losses():
    from lowlight_image_enhancement_amd.pixel_losses import CharbonnierLoss, L1Loss, MSELoss, PSNRLoss
    return {"l1_mean": (lambda: L1Loss(0.8, "mean"), 0.0), "mse_sum": (lambda: MSELoss(0.02, "sum"), 0.0),
            "charbonnier_mean": (lambda: CharbonnierLoss(1.0, "mean", eps=1e-6), 0.0),
            "psnr": (lambda: PSNRLoss(0.5), 0.0), "psnr_y": (lambda: PSNRLoss(0.5, toY=True), 0.0),
            "l1_mean_beside_w_l1": (lambda: L1Loss(0.8, "mean"), 0.3)}


@pytest.mark.parametrize("case", ["l1_mean", "mse_sum", "charbonnier_mean", "psnr", "psnr_y", "l1_mean_beside_w_l1"])
def test_gradient_and_logs_match_the_module_path(dev, case):
    """(a) self.grad of loss_and_grad equals the module path's parameter gradient within 1e-5 norm-wise; (b) logs():
    l_pix equals the module's value (1e-6 relative for the elementwise kinds, 2e-6 |loss_weight| + 2e-7 |ref| for
    PSNRLoss, 2e-5 |loss_weight| with toY) and Total contains it.  The last case keeps w_l1 > 0 beside the pixel term
    (its gradient is then added to d_out instead of opening it)."""
    from lowlight_image_enhancement_amd.NewBP_model.losses import l1_loss
    from lowlight_image_enhancement_amd.pixel_losses import PSNRLoss
    from lowlight_image_enhancement_amd.train import NBPTrainer
    make, w_l1 = _losses()[case]
    lq, gt = _batch(dev)
    tr = NBPTrainer(_net(dev), pixel_loss=make(), w_l1=w_l1, w_ssim=0.0, w_phys=0.0)
    tr.loss_and_grad(lq, gt)
    logs = tr.logs()

    net = _net(dev)
    mod = make()
    out = net(lq)
    l_pix = mod(out, gt)
    total = l_pix + w_l1 * l1_loss(out, gt) if w_l1 else l_pix
    total.backward()
    ref = net.flat.grad.double()
    rel = ((tr.grad.double() - ref).norm() / ref.norm()).item()
    print(f"{case}: parameter gradient norm-wise rel err {rel:.3e}; logs {logs}")
    assert ref.norm().item() > 0 and rel <= 1e-5, rel

    v = float(l_pix.detach().double().item())
    if isinstance(mod, PSNRLoss):
        bound = (2e-5 if mod.toY else 2e-6) * abs(mod.loss_weight) + 2e-7 * abs(v)
    else:
        bound = 1e-6 * abs(v)
    assert abs(logs["l_pix"] - v) <= bound, (logs["l_pix"], v)
    assert abs(logs["Total"] - float(total.detach().double().item())) <= 1e-6 * abs(float(total)) + bound
    assert ("L1_raw" in logs) == bool(w_l1)


def test_fp16_dynamic_scale_graph_step_matches_step(dev):
    """(c) fp16 mode with the dynamic loss scale: three graph_steps leave the parameters bitwise equal to three steps
    from the same start, with the same loss scale (growth_interval 2: the scale, and with it the pixel term's upstream
    entry that nbp_optim_prepare rescales, moves inside the three steps)."""
    from lowlight_image_enhancement_amd.pixel_losses import L1Loss
    from lowlight_image_enhancement_amd.train import NBPTrainer
    lq, gt = _batch(dev)
    res = {}
    for mode in ("step", "graph_step"):
        tr = NBPTrainer(_net(dev, "fp16"), pixel_loss=L1Loss(1.0, "mean"), w_l1=0.0, w_ssim=0.0, w_phys=0.0,
                        init_scale=2.0 ** 12, growth_interval=2)
        assert tr.scaler is not None and tr.precision == "fp16"
        for _ in range(3):
            getattr(tr, mode)(lq, gt)
        logs = tr.logs()
        res[mode] = (tr.net.flat.data.clone(), logs)
    (p0, l0), (p1, l1) = res["step"], res["graph_step"]
    assert torch.equal(p0, p1)
    assert l0["loss_scale"] == l1["loss_scale"] and l0["loss_scale"] != 2.0 ** 12
    assert l0["l_pix"] == l1["l_pix"] and "skipped" not in l0 and "skipped" not in l1


def test_construction_errors(dev):
    """(d)"""
    from lowlight_image_enhancement_amd.pixel_losses import L1Loss
    from lowlight_image_enhancement_amd.train import NBPTrainer
    net = _net(dev)
    with pytest.raises(ValueError):
        NBPTrainer(net, pixel_loss=L1Loss(reduction="none"))
    with pytest.raises(TypeError):
        NBPTrainer(net, pixel_loss=torch.nn.L1Loss())
    tr = NBPTrainer(net)  # no pixel loss: the upstream buffers keep the parent's layout
    tr._ensure_up(2)
    assert tr.pixel_loss is None and tr.up_base.numel() == 5 + 2
