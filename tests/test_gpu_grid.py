"""Tiled inference (val.grids) on the device: nbp_grid_gather bit for bit against torch slices, nbp_grid_blend bit for
bit against the reference's grids_inverse() outputs (tests/golden/grid_blend.npz), and tiling.tiled_forward /
val_forward against the reference's grids() -> test() -> grids_inverse() on a W8 network (grid_nets.npz; fixtures by
make_golden_grids.py).

Bounds: gather and blend are exact (int32 views compared); the fp32 restored frame within 1e-4 max-abs of the
reference's, the project's bound for a restored image (test_gpu_parity.py, test_gpu_tlsc.py); fp16 / bf16 at the PSNR
floors test_gpu_tlsc.py uses for the same network (35 dB / 30 dB); and on block_oracle's U-shaped width-32 network, in
fp16 / bf16, bit for bit its own composition (slices, net(...) in chunks, the pinned blend) and per element within
block_oracle's bound of the float64 frame."""
import functools

import numpy as np
import pytest
import torch

import block_oracle as bo
from conftest import golden
from test_gpu_block_oracle import _check_bound
from test_grid_host import W8_CFG, c_plan, plan_cases

pytestmark = pytest.mark.gpu
PREC = {0: "fp32", 1: "bf16", 2: "fp16"}


def _unaligned(shape, dev):
    """a NaN-filled tensor whose data pointer is 4 bytes past a 16-byte boundary"""
    n = int(np.prod(shape))
    t = torch.full((n + 1,), float("nan"), device=dev)[1:].view(shape)
    assert t.data_ptr() % 16 == 4
    return t


def _gather(img, ch, cw, plan, t0, n, tiles=None):
    from lowlight_image_enhancement_amd._lib import call
    C, H, W = img.shape
    if tiles is None:
        tiles = torch.full((n, C, ch, cw), float("nan"), device=img.device)
    call("grid_gather", img, tiles, C, H, W, ch, cw, *plan, t0, n)
    return tiles


def _blend(outs, H, W, plan, out=None):
    from lowlight_image_enhancement_amd._lib import call
    T, C, ch, cw = outs.shape
    if out is None:
        out = torch.full((C, H, W), float("nan"), device=outs.device)
    call("grid_blend", outs, out, C, H, W, ch, cw, *plan)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("k", range(7))
def test_gather_is_the_slices(dev, k, C):
    h, w, _, ch, cw, ii, jj = plan_cases(golden("grid_plans.npz"))[k]
    rc, *plan = c_plan(h, w, ch, cw)
    assert rc == 0
    T, nc = len(ii), plan[2]
    gen = torch.Generator(device=dev).manual_seed(50 + k)
    img = torch.randn(C, h, w, device=dev, generator=gen)
    img.view(-1)[::31] = -0.0
    ref = torch.cat([img[None, :, i:i + ch, j:j + cw] for i, j in zip(ii, jj)])
    # every tile at once, and sub-ranges that start and end in mid-row of the plan (where it has more than one column)
    ranges = {(0, T), (T - 1, 1), (T // 2, T - T // 2), (min(1, T - 1), max(1, T - 2)), (nc // 2, min(T - nc // 2, nc))}
    for t0, n in sorted(ranges):
        got = _gather(img, ch, cw, plan, t0, n)
        assert torch.equal(_bits(got), _bits(ref[t0:t0 + n])), (t0, n)


def test_gather_and_blend_refuse_a_foreign_plan(dev):
    from lowlight_image_enhancement_amd._lib import NBPError
    h, w, ch, cw = 70, 90, 32, 32
    rc, nr, si, nc, sj = c_plan(h, w, ch, cw)
    img = torch.zeros(3, h, w, device=dev)
    for plan, t0, n in [((nr, si + 1, nc, sj), 0, 1), ((nr, si, nc + 1, sj), 0, 1), ((nr, si, nc, sj), nr * nc, 1),
                        ((nr, si, nc, sj), 1, nr * nc), ((nr, si, nc, sj), -1, 2), ((nr, si, nc, sj), 0, 0)]:
        with pytest.raises(NBPError):
            _gather(img, ch, cw, plan, t0, n)
    with pytest.raises(NBPError):
        _blend(torch.zeros(nr * nc, 3, ch, cw, device=dev), h, w, (nr, si, nc, sj + 1))


def test_blend_is_the_reference_bit_for_bit(dev):
    g, plans = golden("grid_blend.npz"), plan_cases(golden("grid_plans.npz"))
    assert len(g["cases"]) == 4
    for k in (int(v) for v in g["cases"]):
        h, w, _, ch, cw, _, _ = plans[k]
        rc, *plan = c_plan(h, w, ch, cw)
        got = _blend(torch.from_numpy(g[f"outs_{k}"]).to(dev), h, w, plan).cpu().numpy()
        ref = g[f"out_{k}"][0]
        diff = got.view(np.int32) != ref.view(np.int32)
        assert not diff.any(), (k, int(diff.sum()), float(np.abs(got - ref).max()))


@pytest.mark.parametrize("k", range(7))
def test_blend_of_constant_tiles_is_the_constant(dev, k):
    """the number of addends and the divisor agree at every pixel: c + c = 2c and 2c + c + c = 4c are exact"""
    h, w, _, ch, cw, ii, _ = plan_cases(golden("grid_plans.npz"))[k]
    rc, *plan = c_plan(h, w, ch, cw)
    for value in (1.0, 0.3):
        out = _blend(torch.full((len(ii), 2, ch, cw), value, device=dev), h, w, plan)
        assert torch.equal(out, torch.full_like(out, value)), (k, value)


@pytest.mark.parametrize("h,w,ch,cw", [(64, 96, 32, 32), (65, 100, 32, 33), (70, 92, 32, 36)])
def test_blend_and_gather_take_unaligned_views(dev, h, w, ch, cw):
    """sources at any 4-byte alignment (16-byte loads still), destinations off 16 bytes (the 4-byte path): same bits"""
    rc, *plan = c_plan(h, w, ch, cw)
    T = plan[0] * plan[2]
    gen = torch.Generator(device=dev).manual_seed(77)
    outs = torch.randn(T * 3 * ch * cw + 1, device=dev, generator=gen)
    a = _blend(outs[:-1].view(T, 3, ch, cw), h, w, plan)
    shifted = torch.empty_like(outs)
    shifted[1:] = outs[:-1]
    c = _blend(shifted[1:].view(T, 3, ch, cw), h, w, plan)  # data_ptr() + 4
    assert shifted[1:].data_ptr() % 16 == 4
    assert torch.equal(_bits(a), _bits(c))
    d = _blend(outs[:-1].view(T, 3, ch, cw), h, w, plan, out=_unaligned((3, h, w), dev))
    assert torch.equal(_bits(a), _bits(d))
    img = torch.randn(3 * h * w + 1, device=dev, generator=gen)
    t_al = _gather(img[:-1].view(3, h, w), ch, cw, plan, 0, T)
    sh = torch.empty_like(img)
    sh[1:] = img[:-1]
    t_un = _gather(sh[1:].view(3, h, w), ch, cw, plan, 0, T)
    assert torch.equal(_bits(t_al), _bits(t_un))
    t_dst = _gather(img[:-1].view(3, h, w), ch, cw, plan, 0, T, tiles=_unaligned((T, 3, ch, cw), dev))
    assert torch.equal(_bits(t_al), _bits(t_dst))
    ref = torch.cat([img[:-1].view(3, h, w)[None, :, i:i + ch, j:j + cw]
                     for i in [*range(0, plan[1] * (plan[0] - 1), plan[1]), h - ch][:plan[0]]
                     for j in [*range(0, plan[3] * (plan[2] - 1), plan[3]), w - cw][:plan[2]]])
    assert torch.equal(_bits(t_al), _bits(ref))


# ---------------------------------------------------------------------------------------------- the whole path
_NETS = {}


def _case(k, dev):
    """(net, lq on the device, the reference's tiled output, val_opt), built once per case"""
    if k not in _NETS:
        from lowlight_image_enhancement_amd.nafnet import NAFNet
        from param_recipe import recipe_state
        g = golden("grid_nets.npz")
        net = NAFNet(**W8_CFG)
        net.load_state_dict(recipe_state([(n, tuple(v.shape)) for n, v in net.state_dict().items()], int(g[f"seed_{k}"])))
        net = net.to(dev)
        opt = {"crop_size_h": int(g[f"crop_{k}"][0]), "crop_size_w": int(g[f"crop_{k}"][1])}
        if int(g[f"minibatch_{k}"]) > 0:
            opt["max_minibatch"] = int(g[f"minibatch_{k}"])
        _NETS[k] = (net, torch.from_numpy(g[f"lq_{k}"]).to(dev), torch.from_numpy(g[f"out_{k}"]), opt)
    return _NETS[k]


@pytest.mark.parametrize("k", [0, 1])
def test_tiled_forward_fp32_against_the_reference(dev, k):
    from lowlight_image_enhancement_amd.tiling import tiled_forward, val_forward
    net, lq, ref, opt = _case(k, dev)
    net.precision = "fp32"
    out = tiled_forward(net, lq, opt)
    assert out.shape == lq.shape and out.dtype == torch.float32
    err = (out.cpu() - ref).abs().max().item()
    print(f"case {k}: fp32 max |tiled - reference| = {err:.3e}")
    assert err <= 1e-4, err
    assert torch.equal(val_forward(net, lq, dict(opt, grids=True)), out)
    if k == 0:  # other chunkings (the network's summation orders may depend on the batch): the same bound
        assert opt["max_minibatch"] == 4
        for m in (1, 9, 100):
            other = tiled_forward(net, lq, dict(opt, max_minibatch=m))
            assert (other.cpu() - ref).abs().max().item() <= 1e-4, m
    with torch.no_grad():
        plain = net(lq)
    miss = (plain.cpu() - ref).abs().max().item()
    print(f"case {k}: whole-frame forward max |plain - reference| = {miss:.3e}")
    assert miss > 1e-4, miss  # tiling happened: the whole-frame forward is another function


@pytest.mark.parametrize("dt", [1, 2])
@pytest.mark.parametrize("k", [0, 1])
def test_tiled_forward_16bit_modes(dev, k, dt):
    from lowlight_image_enhancement_amd.tiling import tiled_forward
    net, lq, ref, opt = _case(k, dev)
    net.precision = PREC[dt]
    try:
        out = tiled_forward(net, lq, opt)
    finally:
        net.precision = "fp32"
    assert out.dtype == torch.float32
    mse = ((out.cpu().double() - ref.double()) ** 2).mean().item()
    psnr = 10 * np.log10(1.0 / max(mse, 1e-30))
    print(f"case {k}: {PREC[dt]} PSNR against the reference's fp32 tiled output = {psnr:.2f} dB")
    assert psnr >= (35.0 if dt == 2 else 30.0), psnr


# The 16-bit tiled frame per element: block_oracle's U-shaped width-32 network (its crops take the fused plans the
# width-8 fixture never reaches: the tile path at C 32 / 64 with the fused FFN half, gemm_res_ln at C 128), a 49 x 41
# frame cut into 3 x 3 crops of 22 x 18 with ragged last rows and columns, in chunks of 4, 4 and 1 (block_oracle.TILED).
_U32 = {}


def _u32(dev):
    """(the network, the frame on the device), built once"""
    if not _U32:
        from lowlight_image_enhancement_amd.nafnet import NAFNet
        sd, lq, _ = bo.case_inputs(bo.TILED)
        net = NAFNet(**bo.TILED.ctor)
        net.load_state_dict(sd)
        _U32["v"] = (net.to(dev), lq.to(dev))
    return _U32["v"]


@functools.lru_cache(maxsize=None)
def _tiled_host(dtype):
    torch.set_num_threads(16)
    return bo.run_tiled(dtype)


@pytest.mark.parametrize("dt", [1, 2])
def test_tiled_forward_16bit_is_its_composition(dev, dt):
    """tiled_forward bit for bit what it is composed of: the crops by torch slicing at the plan's offsets, net(...) over
    them in the same chunks, nbp_grid_blend (pinned by test_blend_is_the_reference_bit_for_bit); val_forward with grids
    set is the same frame.  The crops' block plans are recorded: they are the fused ones."""
    from lowlight_image_enhancement_amd.tiling import tiled_forward, val_forward
    net, lq = _u32(dev)
    H, W = lq.shape[2:]
    ch, cw, at, crops = bo.tiled_crops(lq)
    rc, *plan = c_plan(H, W, ch, cw)
    assert rc == 0 and len(at) == plan[0] * plan[2] == 9
    assert at[-1] == (H - ch, W - cw) and (H - ch) % plan[1] and (W - cw) % plan[3]  # ragged last row and column
    m = bo.TILED_OPT["max_minibatch"]
    plans, plan_block = [], net._plan_block
    net.precision = PREC[dt]
    net._plan_block = lambda *a: plans.append((a[5], plan_block(*a))) or plans[-1][1]
    try:
        with torch.no_grad():
            outs = torch.cat([net(crops[t0:t0 + m]) for t0 in range(0, len(at), m)])
        del net._plan_block
        out = tiled_forward(net, lq, bo.TILED_OPT)
        again = val_forward(net, lq, dict(bo.TILED_OPT, grids=True))
    finally:
        net.__dict__.pop("_plan_block", None)
        net.precision = "fp32"
    assert outs.dtype == torch.float32 and out.dtype == torch.float32 and out.shape == lq.shape
    ref = _blend(outs, H, W, plan)[None]
    assert torch.equal(_bits(out), _bits(ref)), (out - ref).abs().max().item()
    assert torch.equal(_bits(again), _bits(ref))
    loc = bo.LOCAL_CASE["loc_u32"]  # the same network and crop size, run without a tape: the same plan fields
    assert [p for p, _ in plans] == bo.block_prefixes(bo.TILED.ctor) * 3
    for pre, bp in plans:
        assert bp.local is None
        for field, want in bo.expected_plan(loc, pre).items():
            assert getattr(bp, field) == want, (pre, field)


@pytest.mark.parametrize("dt", [1, 2])
def test_tiled_forward_16bit_per_element(dev, dt):
    """Every element of the tiled frame within block_oracle's bound of the float64 frame: the oracle per crop blended in
    float64, the bound from the emulation blended the same way.
    Measured worst error / bound on an MI355X: bf16 0.240, fp16 0.245."""
    from lowlight_image_enhancement_amd.tiling import tiled_forward
    net, lq = _u32(dev)
    net.precision = PREC[dt]
    try:
        out = tiled_forward(net, lq, bo.TILED_OPT)
    finally:
        net.precision = "fp32"
    _check_bound(f"tiled {PREC[dt]}", {"out": out.double().cpu()}, _tiled_host(None), _tiled_host(PREC[dt]))


def test_one_tile_is_the_plain_forward(dev):
    from lowlight_image_enhancement_amd.tiling import tiled_forward
    net, lq, _, _ = _case(0, dev)
    net.precision = "fp32"
    one = lq[:, :, :40, :48].contiguous()
    with torch.no_grad():
        ref = net(one)
    out = tiled_forward(net, one, {"crop_size_h": 40, "crop_size_w": 48})
    assert torch.equal(_bits(out), _bits(ref))
    out = tiled_forward(net, one, {"crop_size_h_ratio": 1.0, "crop_size_w_ratio": 1.0, "max_minibatch": 3})
    assert torch.equal(_bits(out), _bits(ref))


def test_val_forward_without_grids_is_the_plain_forward(dev):
    from lowlight_image_enhancement_amd.tiling import val_forward
    net, lq, _, opt = _case(0, dev)
    net.precision = "fp32"
    with torch.no_grad():
        ref = net(lq)
    assert torch.equal(_bits(val_forward(net, lq, {})), _bits(ref))
    assert torch.equal(_bits(val_forward(net, lq, dict(opt, grids=False))), _bits(ref))
    two = torch.cat([lq, lq.flip(3)])
    with torch.no_grad():
        ref2 = torch.cat([net(two[:1]), net(two[1:])])
    assert torch.equal(_bits(val_forward(net, two, {"max_minibatch": 1})), _bits(ref2))


def test_tiled_forward_argument_errors(dev):
    from lowlight_image_enhancement_amd.tiling import tiled_forward
    net, lq, _, opt = _case(0, dev)
    with pytest.raises(ValueError, match="b == 1"):
        tiled_forward(net, torch.cat([lq, lq]), opt)
    with pytest.raises(ValueError):
        tiled_forward(net, lq, {"crop_size_h": 71, "crop_size_w": 32})
    with pytest.raises(KeyError):
        tiled_forward(net, lq, {"crop_size_h": 32})
