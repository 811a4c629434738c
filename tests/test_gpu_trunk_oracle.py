"""The VGG19 perceptual trunk and the LPIPS vgg / alex trunks in bf16, fp16 and fp32: every tensor the device stores,
forward and backward, per element against the float64 stage computed from the device's own stored inputs
(tests/trunk_oracle.py: the stages, the rounding points and the bound

    |dev - ref| <= K * 2^-24 * S + ulp_st(ref) / 2 + ulp_st(dev) / 2,

K the dot length, S the same operation on absolute values, ulp_st the storage type's spacing).  Nothing compounds: a
stage's inputs are what the device stored, so a tap gradient added one layer off, a wrong mask, a dropped ReLU mask
in a pool backward, a mis-scaled head or an error in one type's template shows at its own stage at full size.

Per case (trunk x type), with synthetic weights (nonzero biases) and 2 x 3 x 36 x 20 (VGG: a 9 x 5 map meets a pool,
the deepest convs have M = 4 rows and K = 4608) or 2 x 3 x 67 x 51 (AlexNet: overlapping pool windows over 16 x 12 and
7 x 5) images:
  * forward: the prepared input and every conv output within the bound; every pool output and argmax equal to the
    first-maximum route of its stored input (the pool kernel is run again on the stored input: its output is not on
    the tape; the argmax must equal the tape's);
  * heads: the loss / the per-image LPIPS values within 1e-5 |ref|; feat_dist_bwd / lpips_tap_bwd per element, with a
    non-uniform `up` per image;
  * backward: every traced tensor (the `trace` keyword of VGGStack.backward / AlexStack.backward /
    lpips._trunk_backward) within the bound, K = k k Cout; the 2x2 pool backward exact; the 3x3 / 2 pool backward with
    K = 3 (up to four contributions added in fp32); add_relu_masked from the traced copy of the value it overwrote,
    exact where the mask is off; d8 and the image gradient with the fp32 ulp;
  * closure: the expected number of trace entries, every stored tensor checked exactly once, the traced run bitwise
    equal to the untraced one, and the public paths (module(x, y).backward(up) for both inputs, value_and_grad) bitwise
    equal to vgg.input_grad of the last traced tensor.
Both inputs' walks are checked.  fp16 runs scale `up` by a power of two (trunk_oracle.make_up).  Each case prints its
worst error / bound ratio and the stage it occurred at before asserting (DESIGN §4 records them).
"""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trunk_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu

TRUNKS = ("perceptual", "lpips_vgg", "lpips_alex")


def _nchw(t):
    return t.detach().permute(0, 3, 1, 2).contiguous().cpu()


def _img3(t8):
    """The three image channels of an 8-channel NHWC map whose padding channels must be zero."""
    assert torch.count_nonzero(t8[..., 3:]).item() == 0, "padding channels 3..7 are not zero"
    return _nchw(t8[..., :3])


def _forward_records(stack, x8, tape, alex):
    """trunk_oracle's forward records from the device tape; every pool kernel is run again on its stored input for the
    output the tape does not keep."""
    from lowlight_image_enhancement_amd._lib import call
    recs = [("prep", _img3(x8))]
    for rec in tape:
        if rec[0] == "conv":
            recs.append(("conv", _nchw(rec[3])))
            continue
        _, (B, h, w, C), idx, pool_in = rec
        if alex:
            ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        else:
            ho, wo = h // 2, w // 2
        y = torch.empty(B, ho, wo, C, device=pool_in.device, dtype=pool_in.dtype)
        idx2 = torch.full((B, ho, wo, C), 255, device=pool_in.device, dtype=torch.uint8)
        if alex:
            call("maxpool_k_fwd", pool_in, B, h, w, C, 3, 2, y, idx2, stack.dtype)
        else:
            call("maxpool2_fwd", pool_in, B, h, w, C, y, idx2, stack.dtype)
        assert torch.equal(idx, idx2), "the pool's argmax is not repeatable"
        recs.append(("pool", _nchw(idx).long(), _nchw(y)))
    return recs


def _trace_cpu(trace):
    return [(n, _img3(t) if n == "d8" else _nchw(t)) for n, t in trace]


def _bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _run_perceptual(dev, st_name, feats, xs, up):
    from lowlight_image_enhancement_amd import vgg
    from lowlight_image_enhancement_amd._lib import call, query
    from lowlight_image_enhancement_amd.NewBP_model.losses import PerceptualLoss
    mod = PerceptualLoss(device=dev, weights=feats, precision=st_name)
    stack = mod.stack(dev)
    assert stack.tdt == T.ST[st_name]
    run = T.Run([x.cpu() for x in xs], up.cpu())
    tapes, feat = [], []
    for s in (0, 1):
        x8 = vgg.prep_input(xs[s], dtype=stack.dtype)
        f, tape, _ = stack.forward(x8, save=True)
        run.fwd[s] = _forward_records(stack, x8, tape, alex=False)
        tapes.append(tape)
        feat.append(f)
    n = feat[0].numel()
    scale = 1.0 / n
    ws = torch.empty(query("feat_dist_workspace_doubles", n), dtype=torch.float64, device=dev)
    out = torch.empty((), device=dev)
    call("feat_dist_fwd", feat[0], feat[1], n, 0, scale, ws, out, stack.dtype)
    run.value = out.cpu()
    for s in (0, 1):
        d = torch.empty_like(feat[s])
        call("feat_dist_bwd", feat[s], feat[1 - s], n, 0, float(scale), 1, up, d, stack.dtype)
        run.heads[s] = [_nchw(d)]
        trace = []
        d8 = stack.backward(tapes[s], d, trace=trace)
        assert _bitwise(d8, stack.backward(tapes[s], d)) and trace[-1][1] is d8
        run.trace[s] = _trace_cpu(trace)
        dx = vgg.input_grad(trace[-1][1], xs[s])
        run.dx[s] = dx.cpu()
    # the public paths
    g, t = xs[0].clone().requires_grad_(), xs[1].clone().requires_grad_()
    loss = mod(g, t)
    loss.backward(up.reshape(()))
    assert _bitwise(loss.detach().cpu(), run.value)
    assert _bitwise(g.grad.cpu(), run.dx[0]) and _bitwise(t.grad.cpu(), run.dx[1])
    out2 = torch.empty(1, device=dev)
    gv = mod.value_and_grad(xs[0], xs[1], up, out2)
    assert _bitwise(gv.cpu(), run.dx[0]) and _bitwise(out2.cpu().reshape(()), run.value)
    return run


def _run_lpips(dev, st_name, net, feats, lins, xs, up):
    from lowlight_image_enhancement_amd import lpips, vgg
    from lowlight_image_enhancement_amd._lib import call
    mod = lpips.LPIPS(net=net, weights=T.lpips_state_dict(feats, lins), precision=st_name)
    stack, dl = mod.parts(dev)
    assert stack.tdt == T.ST[st_name]
    alex = net == "alex"
    run = T.Run([x.cpu() for x in xs], up.cpu())
    N = xs[0].shape[0]
    tapes, taps = [], []
    for s in (0, 1):
        x8 = vgg.prep_input(xs[s], lpips.SHIFT, lpips.SCALE, clamp=False, dtype=stack.dtype)
        t, tape = lpips._trunk_taps(stack, xs[s], True)
        run.fwd[s] = _forward_records(stack, x8, tape, alex)
        tapes.append(tape)
        taps.append(t)
    out = torch.zeros(N, device=dev)
    lpips._tap_distances(stack, dl, taps[0], taps[1], out, False)
    run.value = out.cpu()
    for s in (0, 1):
        grads = []
        for k in range(5):
            a, b = taps[s][k], taps[1 - s][k]
            g = torch.full_like(a, float("nan"))
            call("lpips_tap_bwd", a, b, dl[k], N, a.shape[1] * a.shape[2], a.shape[3], up, g, stack.dtype)
            grads.append(g)
        run.heads[s] = [_nchw(g) for g in grads]
        trace = []
        d8 = lpips._trunk_backward(stack, tapes[s], grads, trace=trace)
        assert _bitwise(d8, lpips._trunk_backward(stack, tapes[s], grads)) and trace[-1][1] is d8
        assert all(_bitwise(_nchw(g), h) for g, h in zip(grads, run.heads[s])), "the walk changed a tap gradient"
        run.trace[s] = _trace_cpu(trace)
        run.dx[s] = vgg.input_grad(d8, xs[s], lpips.SCALE, clamp=False).cpu()
    # the public paths
    g0, g1 = xs[0].clone().requires_grad_(), xs[1].clone().requires_grad_()
    val = mod(g0, g1)
    val.backward(up.view(N, 1, 1, 1))
    assert _bitwise(val.detach().reshape(-1).cpu(), run.value)
    assert _bitwise(g0.grad.cpu(), run.dx[0]) and _bitwise(g1.grad.cpu(), run.dx[1])
    out2 = torch.empty(N, device=dev)
    gv = mod.value_and_grad(xs[0], xs[1], up, out2, clamp=False)
    assert _bitwise(gv.cpu(), run.dx[0]) and _bitwise(out2.cpu(), run.value)
    return run


@pytest.mark.parametrize("st_name", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("trunk", TRUNKS)
def test_trunk_every_stored_tensor_against_float64(dev, trunk, st_name):
    arch = T.ARCHS[trunk]
    feats, lins = T.make_weights(trunk)
    xs = [x.to(dev) for x in T.make_inputs(trunk)]
    up = T.make_up(trunk, st_name).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if trunk == "perceptual":
            run = _run_perceptual(dev, st_name, feats, xs, up)
        else:
            run = _run_lpips(dev, st_name, trunk.split("_")[1], feats, lins, xs, up)
    for s in (0, 1):
        assert len(run.trace[s]) == T.TRACE_ENTRIES[trunk]
    rep = T.verify(arch, feats, lins, run, st_name, collect=True)
    stage, worst = rep.worst()
    print(f"trunk oracle {trunk} {st_name}: worst error / bound {worst:.3f} at {stage}; largest share below the smallest "
          f"normal {max(rep.small.values()):.3%}; {len(rep.checked)} stored tensors checked")
    groups = {"prep": ".prep", "conv fwd": ".fwd.", "head": ".head.", "conv bwd": (".dn", ".dp", ".d8"),
              "pool bwd": ".pool", "add_relu_masked": ".tap", "dx": ".dx"}
    for g, pat in groups.items():  # the worst ratio per kind of stage (exact stages report 0)
        r = [v for k, v in rep.ratio.items() if (k.endswith(pat) if g in ("prep", "conv bwd", "pool bwd", "add_relu_masked",
                                                                          "dx") else pat in k and ".fwd.pool" not in k)]
        if r:
            print(f"    {g}: {max(r):.3f} over {len(r)} tensors")
    for f in rep.failures:
        print("  FAILED", f)
    assert not rep.failures, rep.failures
    assert len(rep.checked) == T.expected_checks(arch) == len(set(rep.checked))
    assert worst <= 1.0
