"""Host tests of tests/trunk_oracle.py: the per-stage float64 restatement of the VGG / AlexNet loss trunks.

* Pinning: the stages composed with the identity for a rounding function, and torch's own ReLU / max-pool decisions,
  equal oracle.losses.perceptual_loss / lpips_vgg / lpips_alex under float64 autograd: the value and both input
  gradients to 1e-12 relative.
* Stand-in: a float32 stand-in for the device (every stage in float32, rounded where the device rounds) passes every
  bound of verify() at the GPU test's shapes for bf16, fp16 and fp32, and the float64 reference alone keeps 99 % of
  every stage's nonzero elements above the storage type's smallest normal (the choice of `up`, make_up).
* Mutants: each planted error makes verify() fail, so the GPU test would notice a kernel wrong in the same way.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trunk_oracle as T  # noqa: E402
from oracle import losses as OL  # noqa: E402

TRUNKS = ("perceptual", "lpips_vgg", "lpips_alex")


@pytest.fixture(scope="module")
def models():
    return {t: (T.make_weights(t), T.make_inputs(t)) for t in TRUNKS}


def test_architectures_and_trace_names():
    for t in TRUNKS:
        assert len(T.trace_names(T.ARCHS[t])) == T.TRACE_ENTRIES[t]
    a = T.ARCHS["perceptual"]
    assert len(T.convs_of(a)) == 16 and len(a.ops) == 20
    assert T.ARCHS["lpips_vgg"].taps == (1, 3, 6, 9, 12) and len(T.ARCHS["lpips_vgg"].ops) == 17
    assert len(T.ARCHS["lpips_alex"].ops) == 7


def _autograd(trunk, feats, lins, x0, x1, up):
    x0, x1 = x0.double().requires_grad_(), x1.double().requires_grad_()
    f64 = {k: v.double() for k, v in feats.items()}
    if trunk == "perceptual":
        val = OL.perceptual_loss(f64, x0, x1).reshape(1)
    elif trunk == "lpips_vgg":
        val = OL.lpips_vgg(f64, lins, x0, x1).reshape(-1)
    else:
        val = OL.lpips_alex(f64, lins, x0, x1).reshape(-1)
    (val * up.double()).sum().backward()
    return val.detach(), x0.grad, x1.grad


@pytest.mark.parametrize("trunk", TRUNKS)
def test_composed_stages_equal_the_autograd_oracle(models, trunk):
    (feats, lins), (x0, x1) = models[trunk]
    arch = T.ARCHS[trunk]
    up = T.make_up(trunk, "fp32")
    run = T.standin(arch, feats, lins, (x0, x1), up, None, cd=torch.float64, torch_routes=True)
    val, g0, g1 = _autograd(trunk, feats, lins, x0, x1, up)
    assert g0.abs().max() > 0 and g1.abs().max() > 0
    for name, got, ref in (("value", run.value.reshape(-1), val), ("d in0", run.dx[0], g0), ("d in1", run.dx[1], g1)):
        err = (got - ref).abs().max().item()
        assert err <= 1e-12 * ref.abs().max().item(), (name, err, ref.abs().max().item())
    # the first-maximum route is torch's own on these inputs
    own = T.standin(arch, feats, lins, (x0, x1), up, None, cd=torch.float64)
    assert torch.equal(own.dx[0], run.dx[0]) and torch.equal(own.dx[1], run.dx[1])


_RUNS = {}


def _standin(models, trunk, st_name):
    if (trunk, st_name) not in _RUNS:
        (feats, lins), x = models[trunk]
        _RUNS[trunk, st_name] = T.standin(T.ARCHS[trunk], feats, lins, x, T.make_up(trunk, st_name), st_name)
    return _RUNS[trunk, st_name]


@pytest.mark.parametrize("st_name", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("trunk", TRUNKS)
def test_float32_standin_passes_every_bound(models, trunk, st_name):
    (feats, lins), _ = models[trunk]
    arch = T.ARCHS[trunk]
    run = _standin(models, trunk, st_name)
    rep = T.verify(arch, feats, lins, run, st_name)
    assert len(rep.checked) == T.expected_checks(arch) == len(set(rep.checked))
    stage, worst = rep.worst()
    small = max(rep.small.values())
    print(f"{trunk} {st_name}: worst error / bound {worst:.3f} at {stage}; largest share below the smallest normal "
          f"{small:.3%}")
    assert worst <= 1.0 and small <= T.SMALL_CAP
    assert all(t.abs().max() > 0 for _, t in run.trace[0] + run.trace[1])


@pytest.mark.parametrize("trunk", TRUNKS)
def test_fp16_up_keeps_the_reference_above_the_smallest_normal(models, trunk):
    """The 1 % cap on the float64 reference alone: the composed float64 stages, no rounding anywhere."""
    (feats, lins), x = models[trunk]
    run = T.standin(T.ARCHS[trunk], feats, lins, x, T.make_up(trunk, "fp16"), None, cd=torch.float64)
    tiny, big = torch.finfo(torch.float16).tiny, torch.finfo(torch.float16).max
    for s in (0, 1):
        for name, t in [(f"head{k}", h) for k, h in enumerate(run.heads[s])] + run.trace[s]:
            nz = t != 0
            share = ((t.abs() < tiny) & nz).sum().item() / max(1, nz.sum().item())
            assert share <= T.SMALL_CAP, (name, share)
            assert t.abs().max().item() < big / 4, (name, t.abs().max().item())


# (mutant, trunk, storage type): every planted error on a trunk that has the stage it breaks
MUTANT_CASES = [("pool_no_mask", "perceptual", "bf16"), ("pool_no_mask", "lpips_alex", "fp16"),
                ("tap_late", "lpips_vgg", "bf16"), ("tap_late", "lpips_vgg", "fp32"),
                ("no_flip", "lpips_alex", "bf16"), ("no_flip", "perceptual", "fp32"),
                ("unrounded_weights", "lpips_alex", "bf16"), ("unrounded_weights", "lpips_vgg", "fp16"),
                ("lin_shift", "lpips_alex", "fp16"), ("lin_shift", "lpips_vgg", "bf16"),
                ("fp16_as_bf16", "lpips_alex", "fp16"), ("fp16_as_bf16", "perceptual", "fp16")]


def test_every_mutant_is_covered():
    assert {m for m, _, _ in MUTANT_CASES} == set(T.MUTANTS)


@pytest.mark.parametrize("mutant,trunk,st_name", MUTANT_CASES)
def test_mutant_fails_a_bound(models, mutant, trunk, st_name):
    (feats, lins), x = models[trunk]
    arch = T.ARCHS[trunk]
    run = T.standin(arch, feats, lins, x, T.make_up(trunk, st_name), st_name, mutant=mutant)
    with pytest.raises(AssertionError, match=r"error / bound|must leave exact|not exact") as e:
        T.verify(arch, feats, lins, run, st_name)
    print(f"{mutant} on {trunk} {st_name}: {e.value}")
