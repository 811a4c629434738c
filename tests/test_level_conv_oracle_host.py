"""Host checks of tests/level_conv_oracle.py (no GPU), at the small shapes of tests/test_gpu_level_convs.py and in all
three storage types:

* the conv2d form and the matmul form of the oracle agree to 1e-12 relative on out, dx, dW, db and dskip;
* a torch emulation of a correct kernel (rounded operands, float32 conv2d, one rounding to the storage type) lies inside
  the bound at every element -- the condition under which the reference alone stays within the bound;
* each wrong variant of the operation leaves at least a stated share of the elements outside the bound -- what shows
  that the bound tells these mistakes apart on these inputs.

Shares.  A mistake that makes every output element the sum of other products (taps transposed, kh / kw swapped in the
weight, bias dropped, the last 8-channel chunk dropped) moves an element by O(1) against a bound of about u |ref|: at
least 96 % outside.  Skip dropped, and up rows left in the reference's channel-major order (the weight not passed
through _to_internal): at least 93 %.  PixelShuffle r1 / r2 swapped leaves the diagonal sub-pixels (half the elements)
exactly right: 96 % of the other half, 48 %.  Image b read at image 0's offset leaves image 0 exactly right: 96 % of
the other (B - 1) / B.
"""
import pytest
import torch
import torch.nn.functional as F

import level_conv_oracle as lo

torch.set_num_threads(16)

PRECS = ("bf16", "fp16", "fp32")
CASES = [(name, prec) for name in lo.SMALL_SHAPES for prec in PRECS]


def _inputs(name, prec):
    B, gh, gw, cs = lo.SMALL_SHAPES[name]
    return lo.Inputs(B, gh, gw, cs, prec, seed=1000 + 7 * list(lo.SMALL_SHAPES).index(name) + PRECS.index(prec))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("name,prec", CASES)
def test_conv_and_matmul_forms_agree(name, prec):
    inp = _inputs(name, prec)
    d = lo.down_conv(inp.f64("down_x"), inp.f64("down_w"), inp.f64("down_b"), inp.f64("down_dy"))
    m = lo.down_mm(inp.f64("down_x"), inp.f64("down_w"), inp.f64("down_b"), inp.f64("down_dy"))
    for k in ("out", "dx", "dW", "db"):
        assert d[k].shape == m[k].shape, k
        assert _rel(m[k], d[k]) <= 1e-12, ("down", k)
    u = lo.up_conv(inp.f64("up_x"), inp.f64("up_w"), inp.f64("up_skip"), inp.f64("up_dy"))
    m = lo.up_mm(inp.f64("up_x"), inp.f64("up_w"), inp.f64("up_skip"), inp.f64("up_dy"))
    for k in ("out", "dx", "dW", "dskip"):
        assert u[k].shape == m[k].shape, k
        assert _rel(m[k], u[k]) <= 1e-12, ("up", k)
    assert torch.equal(u["dskip"], inp.f64("up_dy"))  # the skip add is an identity branch


def _emu_down(x, W, b, prec):
    return F.conv2d(x.float(), W.float(), None if b is None else b.float(), stride=2).to(lo.STORAGE[prec]).double()


def _emu_up(x, W, skip, prec):
    y = F.pixel_shuffle(F.conv2d(x.float(), W.float()), 2)
    if skip is not None:
        y = y + skip.float()
    return y.to(lo.STORAGE[prec]).double()


def _emu_down_dx(dy, W, res, x_shape, prec):
    dx = torch.nn.grad.conv2d_input(x_shape, W.float(), dy.float(), stride=2) + res.float()
    return dx.to(lo.STORAGE[prec]).double()


def _emu_up_dx(dy, W, prec):
    return F.conv2d(F.pixel_unshuffle(dy.float(), 2), W.float().reshape(W.shape[0], -1).t()[:, :, None, None]).to(
        lo.STORAGE[prec]).double()


@pytest.mark.parametrize("name,prec", CASES)
def test_emulation_inside_bound(name, prec):
    inp = _inputs(name, prec)
    cs = inp.cs
    x, W, b, dy, res = (inp.f64(k) for k in ("down_x", "down_w", "down_b", "down_dy", "down_res"))
    ref, mag = lo.down_out_mm(x, W, b)
    assert lo.worst_ratio(_emu_down(x, W, b, prec), ref, lo.bound(ref, mag, 4 * cs, prec)) <= 1.0
    ref, mag = lo.down_dx_mm(dy, W)
    ref, mag = ref + res, mag + res.abs()
    assert lo.worst_ratio(_emu_down_dx(dy, W, res, x.shape, prec), ref, lo.bound(ref, mag, 2 * cs, prec)) <= 1.0
    x, W, skip, dy = (inp.f64(k) for k in ("up_x", "up_w", "up_skip", "up_dy"))
    ref, mag = lo.up_out_mm(x, W, skip)
    assert lo.worst_ratio(_emu_up(x, W, skip, prec), ref, lo.bound(ref, mag, 2 * cs, prec)) <= 1.0
    ref, mag = lo.up_dx_mm(dy, W)
    assert lo.worst_ratio(_emu_up_dx(dy, W, prec), ref, lo.bound(ref, mag, 4 * cs, prec)) <= 1.0


@pytest.mark.parametrize("name,prec", CASES)
def test_wrong_variants_outside_bound(name, prec):
    inp = _inputs(name, prec)
    B, cs = inp.B, inp.cs
    # ---- down
    x, W, b = inp.f64("down_x"), inp.f64("down_w"), inp.f64("down_b")
    ref, mag = lo.down_out_mm(x, W, b)
    bnd = lo.bound(ref, mag, 4 * cs, prec)
    xs = x.shape
    x_t = x.reshape(xs[0], xs[1], xs[2] // 2, 2, xs[3] // 2, 2).transpose(3, 5).reshape(xs)  # each 2x2 patch transposed
    x_last = x.clone()
    x_last[:, -8:] = 0
    wrong = {"taps transposed": (_emu_down(x_t, W, b, prec), 0.96),
             "kh/kw swapped in the weight": (_emu_down(x, W.transpose(2, 3), b, prec), 0.96),
             "bias dropped": (_emu_down(x, W, None, prec), 0.96),
             "last 8-channel chunk dropped": (_emu_down(x_last, W, b, prec), 0.96),
             "image b at image 0's offset": (_emu_down(x[:1].expand_as(x), W, b, prec), 0.96 * (B - 1) / B)}
    for what, (got, share) in wrong.items():
        assert lo.share_outside(got, ref, bnd) >= share, ("down", what, lo.share_outside(got, ref, bnd))
    # ---- up
    x, W, skip = inp.f64("up_x"), inp.f64("up_w"), inp.f64("up_skip")
    ref, mag = lo.up_out_mm(x, W, skip)
    bnd = lo.bound(ref, mag, 2 * cs, prec)
    W_sw = W.reshape(W.shape[0] // 4, 2, 2, W.shape[1]).transpose(1, 2).reshape(W.shape)  # PixelShuffle's r1 <-> r2
    # the device reading reference-order rows as if they were internal-order ones computes the reference operation with
    # the weight _to_reference makes of them
    W_cm = lo.to_reference("up", W.shape, W.reshape(-1))
    x_last = x.clone()
    x_last[:, -8:] = 0
    wrong = {"sub-pixels swapped": (_emu_up(x, W_sw, skip, prec), 0.48),
             "channel-major up rows": (_emu_up(x, W_cm, skip, prec), 0.93),
             "skip dropped": (_emu_up(x, W, None, prec), 0.93),
             "last 8-channel chunk dropped": (_emu_up(x_last, W, skip, prec), 0.96),
             "image b at image 0's offset": (_emu_up(x[:1].expand_as(x), W, skip, prec), 0.96 * (B - 1) / B)}
    for what, (got, share) in wrong.items():
        assert lo.share_outside(got, ref, bnd) >= share, ("up", what, lo.share_outside(got, ref, bnd))
    # the layout round trip the device tests rely on
    for kind, key in (("down", "down_w"), ("up", "up_w")):
        Wr = inp.f64(key)
        assert torch.equal(lo.to_reference(kind, Wr.shape, lo.to_internal(kind, Wr)), Wr)
