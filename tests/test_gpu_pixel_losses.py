"""GPU tests of the pixel_opt losses (pixel_losses.py over nbp_pixel_loss / nbp_psnr_loss) against the reference's
basicsr/models/losses evaluated in float64 (tests/golden/pixel_losses.npz, made by golden/make_golden_pixel_losses.py).

Bounds.  Elementwise value: relative error <= 1e-6 (at most three fp32 roundings per element at 2^-24 each, float64
accumulation, one final rounding); the fixture's per-case `_vbound` is that number, or twice the reference's own fp32
distance from its float64 value where that is larger (never derived from the code under test).  Gradient: every element
within max(1e-6 |ref|, 1e-6 max|ref of the case|).  PSNRLoss value: |d| <= 2e-6 |loss_weight| + 2e-7 |ref| (the error
of log(mse) is the relative error of mse, times 10/ln 10), 2e-5 |loss_weight| with toY (a few fp32 roundings of O(1)
luma values before the difference); gradient: norm-wise relative error <= 1e-5.  Gradients and maps of more than 4096
elements are compared at the fixture's stored positions (grad_index)."""
import numpy as np
import pytest
import torch

from conftest import golden
import pixel_loss_fixtures as F

pytestmark = pytest.mark.gpu

_G = {}


def fixture():
    if "g" not in _G:
        _G["g"] = golden("pixel_losses.npz")
    return _G["g"]


def _place(a, dev, offset):
    """the array on the device; offset > 0: as a contiguous view at that element offset of a larger buffer (a base
    pointer that is only 4-byte aligned)"""
    if a is None:
        return None
    t = torch.from_numpy(a)
    if offset == 0:
        return t.to(dev)
    buf = torch.zeros(t.numel() + offset + 3, device=dev)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * (offset % 4) and view.is_contiguous()
    return view


def _classes():
    from lowlight_image_enhancement_amd.pixel_losses import CharbonnierLoss, L1Loss, MSELoss
    return {"l1": L1Loss, "mse": MSELoss, "charbonnier": CharbonnierLoss}


def _module(kind, red):
    kw = {"eps": F.CHARBONNIER_EPS} if kind == "charbonnier" else {}
    return _classes()[kind](loss_weight=F.LOSS_WEIGHT[kind], reduction=red, **kw)


def _run_elementwise(dev, name, sk, kind, red, wm, offset):
    shape = F.SHAPES[sk]
    pred_np, target_np = F.inputs(sk, shape)
    w_np = F.weight(sk, shape, wm)
    g = fixture()
    assert F.checksum(pred_np, target_np, w_np) == int(g[f"{name}_crc"]), "fixture inputs changed"
    pred = _place(pred_np, dev, offset).detach().requires_grad_(True)
    target = _place(target_np, dev, offset).detach().requires_grad_(True)
    w = _place(w_np, dev, 2 * offset)
    v = _module(kind, red)(pred, target, weight=w)
    up = (_place(F.upstream_map(name, shape), dev, 3 * offset) if red == "none"
          else torch.tensor(F.UPSTREAM_SCALAR, device=dev))
    v.backward(gradient=up)
    return v.detach(), pred.grad, target.grad


def _check_elementwise(name, red, v, gp, gt, n):
    g = fixture()
    idx = F.grad_index(n)
    ref_v, vb = g[f"{name}_v64"], float(g[f"{name}_vbound"])
    mine_v = v.double().cpu().numpy()
    if red == "none":
        mine_v = mine_v.reshape(-1)[idx]
    err = np.abs(mine_v - ref_v)
    print(f"{name}: value rel err {float(np.max(err / np.maximum(np.abs(ref_v), 1e-300))):.3e} (bound {vb:.1e})")
    assert np.all(err <= vb * np.abs(ref_v)), (name, float(err.max()))
    ref_g = g[f"{name}_gp64"]
    tol = np.maximum(1e-6 * np.abs(ref_g), 1e-6 * np.abs(ref_g).max())
    for label, mine, ref in (("pred", gp, ref_g), ("target", gt, -ref_g)):
        m = mine.double().cpu().numpy().reshape(-1)[idx]
        e = np.abs(m - ref)
        print(f"{name}: d/d {label} max err / max|g| {float(e.max() / max(np.abs(ref_g).max(), 1e-300)):.3e}")
        assert np.all(e <= tol), (name, label, float(e.max()), float(np.abs(ref_g).max()))


ELEMENTWISE = F.elementwise_cases()


@pytest.mark.parametrize("name,sk,kind,red,wm", ELEMENTWISE, ids=[c[0] for c in ELEMENTWISE])
def test_elementwise_against_reference_f64(dev, name, sk, kind, red, wm):
    v, gp, gt = _run_elementwise(dev, name, sk, kind, red, wm, 0)
    _check_elementwise(name, red, v, gp, gt, int(np.prod(F.SHAPES[sk])))


OFFSET = [c for c in ELEMENTWISE if c[1] == "A"]


@pytest.mark.parametrize("name,sk,kind,red,wm", OFFSET, ids=[c[0] + "_offset1" for c in OFFSET])
def test_elementwise_on_a_4_byte_aligned_view(dev, name, sk, kind, red, wm):
    """(2,3,9,37) as a contiguous view at element offset 1 (weight at 2, upstream map at 3) of larger buffers: the
    same numbers as the aligned case, so the same fixture entries."""
    v, gp, gt = _run_elementwise(dev, name, sk, kind, red, wm, 1)
    _check_elementwise(name, red, v, gp, gt, int(np.prod(F.SHAPES[sk])))


def _run_psnr(dev, name, sk, toY, offset):
    from lowlight_image_enhancement_amd.pixel_losses import PSNRLoss
    shape = F.PSNR_SHAPES[sk]
    pred_np, target_np = F.psnr_inputs(sk, shape)
    assert F.checksum(pred_np, target_np) == int(fixture()[f"{name}_crc"]), "fixture inputs changed"
    pred = _place(pred_np, dev, offset).detach().requires_grad_(True)
    target = _place(target_np, dev, offset).detach().requires_grad_(True)
    v = PSNRLoss(loss_weight=F.PSNR_LOSS_WEIGHT, toY=toY)(pred, target)
    v.backward(gradient=torch.tensor(F.UPSTREAM_SCALAR, device=dev))
    return v.detach(), pred.grad, target.grad


def _check_psnr(name, v, gp, gt, n):
    g = fixture()
    ref, vb = float(g[f"{name}_v64"]), float(g[f"{name}_vbound"])
    err = abs(float(v.double().item()) - ref)
    print(f"{name}: value {float(v):.9f} ref {ref:.9f} |d| {err:.3e} (bound {vb:.2e})")
    assert err <= vb, (name, err, vb)
    idx = F.grad_index(n)
    ref_g = g[f"{name}_gp64"]
    for label, mine, r in (("pred", gp, ref_g), ("target", gt, -ref_g)):
        m = mine.double().cpu().numpy().reshape(-1)[idx]
        rel = float(np.linalg.norm(m - r) / np.linalg.norm(r))
        print(f"{name}: d/d {label} norm-wise rel err {rel:.3e}")
        assert rel <= 1e-5, (name, label, rel)


PSNR = F.psnr_cases()


@pytest.mark.parametrize("name,sk,toY", PSNR, ids=[c[0] for c in PSNR])
def test_psnr_against_reference_f64(dev, name, sk, toY):
    v, gp, gt = _run_psnr(dev, name, sk, toY, 0)
    _check_psnr(name, v, gp, gt, int(np.prod(F.PSNR_SHAPES[sk])))


@pytest.mark.parametrize("name,sk,toY", [c for c in PSNR if c[1] in ("P2", "P3")],
                         ids=[c[0] + "_offset1" for c in PSNR if c[1] in ("P2", "P3")])
def test_psnr_on_a_4_byte_aligned_view(dev, name, sk, toY):
    v, gp, gt = _run_psnr(dev, name, sk, toY, 1)
    _check_psnr(name, v, gp, gt, int(np.prod(F.PSNR_SHAPES[sk])))


@pytest.mark.parametrize("name", ["A_charbonnier_mean_one", "E_charbonnier_mean_full", "E_mse_none_none", "D_l1_mean_none"])
def test_elementwise_runs_are_bitwise_equal(dev, name):
    case = next(c for c in ELEMENTWISE if c[0] == name)
    a = _run_elementwise(dev, *case, 0)
    b = _run_elementwise(dev, *case, 0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["P3_y", "PE_rgb"])
def test_psnr_runs_are_bitwise_equal(dev, name):
    case = next(c for c in PSNR if c[0] == name)
    a = _run_psnr(dev, *case, 0)
    b = _run_psnr(dev, *case, 0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_agrees_with_the_mean_only_functions(dev):
    from lowlight_image_enhancement_amd.NewBP_model.losses import charbonnier_loss, l1_loss
    from lowlight_image_enhancement_amd.pixel_losses import CharbonnierLoss, L1Loss
    gen = torch.Generator(device=dev).manual_seed(5)
    a, b = (torch.rand(2, 3, 33, 47, device=dev, generator=gen) for _ in range(2))
    for new, old in ((L1Loss(1.0, "mean")(a, b), l1_loss(a, b)), (CharbonnierLoss()(a, b), charbonnier_loss(a, b))):
        new, old = float(new.double().item()), float(old.double().item())
        assert abs(new - old) <= 1e-6 * abs(old), (new, old)


def test_functional_forms_and_broadcast_weight(dev):
    """l1_loss / mse_loss / charbonnier_loss(pred, target, weight, reduction); a weight that broadcasts but is neither
    [N,C,H,W] nor [N,1,H,W] is materialised, and 'mean' divides by the reference's denominator of the weight as given
    (loss_util.py:53-58: weight.sum() * C for a one-channel weight), here against that formula in float64."""
    from lowlight_image_enhancement_amd import pixel_losses as P
    gen = torch.Generator(device=dev).manual_seed(6)
    a, b = (torch.rand(2, 3, 9, 11, device=dev, generator=gen) for _ in range(2))
    w = torch.rand(1, 1, 9, 11, device=dev, generator=gen)
    a.requires_grad_(True)
    ad = a.detach().double().requires_grad_(True)
    for fn, elem in ((P.l1_loss, lambda d: d.abs()), (P.mse_loss, lambda d: d * d),
                     (P.charbonnier_loss, lambda d: torch.sqrt(d * d + 1e-12))):
        for red in ("mean", "sum"):
            a.grad = ad.grad = None
            v = fn(a, b, w, reduction=red)
            v.backward()
            e = elem(ad - b.double()) * w.double()
            ref = e.sum() / (w.double().sum() * 3) if red == "mean" else e.sum()
            ref.backward()
            assert abs(float(v.double().item()) - float(ref)) <= 1e-6 * abs(float(ref))
            assert (a.grad.double() - ad.grad).abs().max().item() <= 1e-6 * ad.grad.abs().max().item()
    with pytest.raises(ValueError):
        P.l1_loss(a, b[:, :, :4])
