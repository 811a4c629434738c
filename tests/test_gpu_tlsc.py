"""NAFNetLocal on the device: the TLSC pool and per-pixel SCA gate kernels stage by stage against float64, and the whole
network against the reference's NAFNetLocal outputs (tests/golden/tlsc_nets.npz, made by make_golden_tlsc.py).

Bounds: pooled means atol = rtol = 1e-4 (the project's bound for the SCA's pooled mean); the fp32 gate atol 1e-4 /
rtol 1e-5; a 16-bit gate output within one ulp of its storage type of the float64 value plus the fp32 accumulation
allowance (test_gpu_ffn_rows_f64._within_ulp); the fp32 restored image within 1e-4 of the reference's; the 16-bit modes
at the PSNR floors of test_nafnet_16bit_modes_any_width (35 dB fp16, 30 dB bf16)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_ffn_rows_f64 import _within_ulp
from test_tlsc_host import CASES, case_cfg, tlsc_pool64

pytestmark = pytest.mark.gpu
DTYPES = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
PREC = {0: "fp32", 1: "bf16", 2: "fp16"}


def _pool(g, k1, k2, dt):
    """nbp_tlsc_pool on an NHWC map: (V [B][_h][_w][C], the workspace)"""
    from lowlight_image_enhancement_amd._lib import call, query
    B, H, W, C = g.shape
    assert query("tlsc_supported", B, H, W, C, k1, k2, dt) == 1
    V = torch.full((B, H - k1 + 1, W - k2 + 1, C), float("nan"), device=g.device)
    ws = torch.empty(query("tlsc_workspace_bytes", B, H, W, C, k1, k2), device=g.device, dtype=torch.uint8)
    call("tlsc_pool", g, V, ws, B, H, W, C, k1, k2, dt)
    return V, ws


def _gate(g, V, w, b, ws, k1, k2, dt):
    from lowlight_image_enhancement_amd._lib import call
    B, H, W, C = g.shape
    ga = torch.full_like(g, float("nan"))
    call("tlsc_sca_gate", g, V, w, b, ga, ws, B, H, W, C, k1, k2, dt)
    return ga


def _gate64(g, V, w, b):
    """float64 ga = g (.) (W_sca V[clamp] + b_sca) from the kernel's own window means"""
    B, H, W, C = g.shape
    hv, wv = V.shape[1:3]
    a = V.double() @ w.double().T + b.double()
    iy = (torch.arange(H, device=g.device) - (H - hv) // 2).clamp(0, hv - 1)
    ix = (torch.arange(W, device=g.device) - (W - wv) // 2).clamp(0, wv - 1)
    return g.double() * a[:, iy][:, :, ix]


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_pool_against_float64_on_the_reference_inputs(dev, dt):
    f = golden("tlsc_pool.npz")
    for i in range(len([k for k in f.files if k.startswith("x_")])):
        k = f[f"k_{i}"]
        g = torch.from_numpy(f[f"x_{i}"]).to(dev).permute(0, 2, 3, 1).contiguous().to(DTYPES[dt])
        H, W = g.shape[1:3]
        V, _ = _pool(g, min(H, int(k[0])), min(W, int(k[1])), dt)
        ref, pooled = tlsc_pool64(g.permute(0, 3, 1, 2), k)
        assert torch.allclose(V.double(), ref.permute(0, 2, 3, 1), atol=1e-4, rtol=1e-4), i
        if dt == 0:  # fp32 storage: the same input the reference pooled
            out = torch.from_numpy(f[f"out_{i}"]).to(dev).double()
            assert torch.allclose(pooled, out, atol=1e-4, rtol=1e-4), i


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("shape,k", [((1, 3000, 8, 8), (384, 4)), ((1, 8, 4300, 8), (4, 384))])
def test_pool_long_walks(dev, dt, shape, k):
    """thousands of sliding steps along one axis at a window sum of ~3 k1 k2: the running sums must not drift"""
    gen = torch.Generator(device=dev).manual_seed(5 + shape[1])
    g = (3 + torch.randn(shape, device=dev, generator=gen)).to(DTYPES[dt])
    V, _ = _pool(g, k[0], k[1], dt)
    ref, _ = tlsc_pool64(g.permute(0, 3, 1, 2), k)
    err = (V.double() - ref.permute(0, 2, 3, 1)).abs().max().item()
    print(f"long walk {shape} k {k} dtype {dt}: max |V - float64| = {err:.3e}")
    assert torch.allclose(V.double(), ref.permute(0, 2, 3, 1), atol=1e-4, rtol=1e-4), err


GATE_SHAPES = [  # B, H, W, C, k1, k2
    (2, 18, 23, 8, 9, 15),
    (1, 13, 17, 24, 5, 7),     # odd sizes and kernels, C not a multiple of 32
    (1, 20, 21, 32, 8, 6),
    (1, 10, 12, 64, 4, 5),
    (1, 9, 10, 96, 3, 4),      # channel tiles partly masked
    (2, 12, 8, 512, 6, 6),
    (1, 8, 23, 8, 8, 15),      # one-dimensional: k1 = H (_h = 1)
    (1, 20, 9, 16, 7, 9),      # one-dimensional: k2 = W (_w = 1)
    (3, 7, 50, 16, 2, 1),      # k2 = 1: no horizontal window; more positions than one workgroup's 128
]


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("B,H,W,C,k1,k2", GATE_SHAPES)
def test_sca_gate_against_float64(dev, dt, B, H, W, C, k1, k2):
    from param_recipe import recipe_tensor
    cg = torch.Generator().manual_seed(100 + C + H)
    w = recipe_tensor("sca.1.weight", (C, C, 1, 1), cg).reshape(C, C).contiguous().to(dev)
    b = recipe_tensor("sca.1.bias", (C,), cg).to(dev)
    gen = torch.Generator(device=dev).manual_seed(7 + C + W)
    g = torch.randn(B, H, W, C, device=dev, generator=gen).to(DTYPES[dt])
    V, ws = _pool(g, k1, k2, dt)
    ref_v, _ = tlsc_pool64(g.permute(0, 3, 1, 2), (k1, k2))
    assert torch.allclose(V.double(), ref_v.permute(0, 2, 3, 1), atol=1e-4, rtol=1e-4)
    ga = _gate(g, V, w, b, ws, k1, k2, dt)
    ref = _gate64(g, V, w, b)
    assert ga.dtype == DTYPES[dt] and torch.isfinite(ga.float()).all()
    if dt == 0:
        assert torch.allclose(ga.double(), ref, atol=1e-4, rtol=1e-5), (ga.double() - ref).abs().max().item()
    else:
        _within_ulp(ga, ref, dt, "ga")


@pytest.mark.parametrize("dt", [0, 1, 2])
def test_windows_stay_inside_their_image(dev, dt):
    """two images filled with different constants: every window mean is its own image's constant"""
    B, H, W, C, k1, k2 = 2, 18, 23, 8, 9, 15
    g = torch.empty(B, H, W, C, device=dev, dtype=DTYPES[dt])
    g[0], g[1] = 1.0, 3.0
    V, ws = _pool(g, k1, k2, dt)
    assert (V[0] - 1.0).abs().max().item() <= 1e-5 and (V[1] - 3.0).abs().max().item() <= 1e-5
    w = (torch.eye(C, device=dev) * 0.5).contiguous()
    b = torch.zeros(C, device=dev)
    ga = _gate(g, V, w, b, ws, k1, k2, dt)
    assert (ga[0].float() - 0.5).abs().max().item() <= 1e-5 and (ga[1].float() - 4.5).abs().max().item() <= 1e-4


# ---------------------------------------------------------------------------------------------- the whole network
def _net(g, c, dev, cls=None, **kw):
    from lowlight_image_enhancement_amd.nafnet import NAFNetLocal
    from param_recipe import recipe_state
    cls = cls or NAFNetLocal
    if cls is NAFNetLocal:
        kw.setdefault("train_size", tuple(int(v) for v in g[c + "_train"]))
    net = cls(**case_cfg(g, c), **kw)
    net.load_state_dict(recipe_state([(k, tuple(v.shape)) for k, v in net.state_dict().items()], int(g[c + "_seed"])))
    return net.to(dev)


@pytest.mark.parametrize("c", list(CASES))
def test_nafnet_local_fp32_against_the_reference(dev, c):
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    g = golden("tlsc_nets.npz")
    net = _net(g, c, dev)
    lq = torch.from_numpy(g[c + "_lq"]).to(dev)
    with torch.no_grad():
        out = net(lq)
    err = (out.cpu() - torch.from_numpy(g[c + "_out"])).abs().max().item()
    print(f"case {c}: fp32 max |out - reference| = {err:.3e}")
    assert err <= 1e-4, err
    plain = _net(g, c, dev, cls=NAFNet)
    with torch.no_grad():
        ref = plain(lq)
    if c == "C":  # every block global: NAFNet's own launches
        assert torch.equal(out, ref)
    else:  # the local window matters at these shapes (a wrong dispatch cannot hide under the bound)
        assert (out - ref).abs().max().item() > 1e-2


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("c", ["A", "D"])
def test_nafnet_local_16bit_modes(dev, c, dt):
    g = golden("tlsc_nets.npz")
    net = _net(g, c, dev)
    net.precision = PREC[dt]
    lq = torch.from_numpy(g[c + "_lq"]).to(dev)
    with torch.no_grad():
        out = net(lq)
    mse = ((out.cpu().double() - torch.from_numpy(g[c + "_out"]).double()) ** 2).mean().item()
    psnr = 10 * np.log10(1.0 / max(mse, 1e-30))
    print(f"case {c}: {PREC[dt]} PSNR against the reference's fp32 output = {psnr:.2f} dB")
    assert psnr >= (35.0 if dt == 2 else 30.0), psnr


def test_inference_only_contract(dev):
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    g = golden("tlsc_nets.npz")
    net = _net(g, "A", dev)
    lq = torch.from_numpy(g["A_lq"]).to(dev)
    with pytest.raises(RuntimeError, match="inference only"):
        net(lq)
    with pytest.raises(RuntimeError, match="inference only"):  # the executor refuses too
        net.exec_forward(lq, save=True)
    net.flat.requires_grad_(False)  # nothing requires grad: plain inference
    assert net(lq).shape == lq.shape
    # every block global: back-propagates exactly as NAFNet
    loc, plain = _net(g, "C", dev), _net(g, "C", dev, cls=NAFNet)
    lq = torch.from_numpy(g["C_lq"]).to(dev)
    o1, o2 = loc(lq), plain(lq)
    assert torch.equal(o1, o2)
    o1.square().mean().backward()
    o2.square().mean().backward()
    assert torch.equal(loc.flat.grad, plain.flat.grad) and loc.flat.grad.abs().max().item() > 0


def test_from_net_follows_the_trainers_weights(dev):
    from lowlight_image_enhancement_amd.nafnet import NAFNet, NAFNetLocal
    g = golden("tlsc_nets.npz")
    net = _net(g, "A", dev, cls=NAFNet)
    view = NAFNetLocal.from_net(net, train_size=tuple(int(v) for v in g["A_train"]))
    assert view.flat.data_ptr() == net.flat.data_ptr()
    lq = torch.from_numpy(g["A_lq"]).to(dev)
    with torch.no_grad():
        o1 = view(lq)
        assert (o1.cpu() - torch.from_numpy(g["A_out"])).abs().max().item() <= 1e-4
        net.flat.mul_(0.5)  # an optimizer step on the trainer's network, in place
        o2 = view(lq)
        fresh = NAFNetLocal(train_size=view.train_size, **case_cfg(g, "A")).to(dev)
        fresh.flat.copy_(net.flat)
        assert torch.equal(o2, fresh(lq)) and not torch.equal(o1, o2)
        assert torch.equal(net(lq), _plain_again(net, lq))  # the trainer's network still pools globally


def _plain_again(net, lq):
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    again = NAFNet(img_channel=net.img_channel, width=net.width, enc_blk_nums=net.enc_blk_nums,
                   middle_blk_num=net.middle_blk_num, dec_blk_nums=net.dec_blk_nums).to(lq.device)
    again.flat.data.copy_(net.flat.data)
    return again(lq)
