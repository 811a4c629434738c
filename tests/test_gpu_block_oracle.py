"""Every NAFBlock executor path, forward and backward, per element against the float64 oracle (tests/block_oracle.py).

Each case is a small network (level-less, three blocks: the first, an inner and the last block differ in carry_next and
in the deferral of the conv1 input gradient; one U-shaped case) run through NAFNet.exec_forward / exec_backward in bf16
and in fp16 with the recipe weights (active beta / gamma), a torch.rand image and a torch.randn upstream gradient.  The
BlockPlan of every block record is asserted first, so a case cannot silently stop covering its path; the gradient
buffer is pre-filled with NaN, so a gradient no launch writes fails; then `out`, `dx` and every parameter gradient must
lie within bound = 4 * max|emulation - oracle| + 1e-5 * max|oracle| of the oracle, per tensor and for every element
(block_oracle's docstring: the emulation rounds where the executor stores, so its error is the storage type's own).

Plan fields asserted per case (all three blocks unless a position is named; carry_next: first / inner True, last False
wherever ln_fwd or rows_ffn holds, else False):
  c32, c32_wide       tile, ln_epilogue, ln_fwd, drop_t4, ffn, sg_rc_wg, ln_wg, sca_fold; no c1dw / rows_ffn / grouped /
                      chandot  (M = 240 is no multiple of 32; 9 x 70: several tiles across, ragged both ways)
  c32_stored_t4       as c32 but drop_t4 = ffn = sg_rc_wg = False (sg_rc off: stored t4, SimpleGate backward in the
                      dgrad epilogue)
  c32_unfolded        as c32 but ffn = sg_rc_wg = ln_wg = sca_fold = False, drop_t4 still True (switches; a case beyond the
                      issue's table: nbp_dgrad_sg_rc, nbp_dgrad_ln_bwd at C 32, nbp_c1dw_bwd_tile + nbp_sca_bwd_fused)
  c64, c64_wide       tile, ln_epilogue, ln_fwd, sca_fold; no drop_t4 / ffn / sg_rc_wg / ln_wg / grouped / chandot
  c64_stored_tape     as c64 but tile = False (fuse_c1dw_tile off), c1dw = False
  c128_rows, c256_rows  rows_ffn, rows_pre, grouped, sca_fold, ln_epilogue, chandot; no tile / c1dw / drop_t4 / ffn
  c128_launches       as c128_rows but rows_ffn = False (fuse_ffn_rows off), ln_fwd: gemm_res_ln + the chandot epilogue
  c128_hw60           rows_ffn = False, chandot = False (h * w = 60), ln_fwd, grouped
  c512_c1dw_rows      c1dw (chunks 1), rows_ffn, grouped, sca_fold; ln_epilogue = ln_fwd = False
  c512_rows           c1dw = False, rows_ffn, grouped; ln_epilogue = False (stand-alone LayerNorm backward)
  c512_hw60, c1024    nothing fused: no tile / c1dw / rows_ffn / ln_epilogue / chandot; grouped, sca_fold
  c24, c40            sca_fold = False (c % 16), grouped = False, nothing fused
  c48                 sca_fold, no ln_epilogue;  c48_sca_unfolded: sca_fold = False (switch)
  u32                 encoders.0.0 / decoders.1.0 as c32, encoders.1.0 / decoders.0.0 as c64, middle_blks.0 (C 128 at
                      6 x 5) as c128_hw60; carry_next False everywhere (one block per level); 22 x 18 padded to 24 x 20

Which case reaches which branch of the executor:
  _block_fwd   norm1 from the carry: the inner / last blocks of c32*, c64*, c128*, c256_rows, c512_*rows; stand-alone:
               every first block and every block of c512_hw60, c1024, c24, c40, c48*, u32
               conv1 chain: tile (c32*, c64, c64_wide, u32) / c1dw (c512_c1dw_rows) / GEMM + dw_sg_pool (the others)
               conv3: ffn_rows_fwd (c128_rows, c256_rows, c512_c1dw_rows, c512_rows) / gemm_res_ln (c32*, c64*,
               c128_launches, c128_hw60, u32) / GEMM + ln_fwd_nhwc (c512_hw60, c1024, c24, c40, c48*)
               conv4: gemm_ffn (c32, c32_wide, u32) / CM_SG, with t4 dropped (c32_unfolded) or stored (the other non-rows
               cases) / the fp32 pair of launches (fp32 controls)
               conv5: gemm_res_ln with the next norm1 (first / inner blocks of c32_stored_t4, c32_unfolded, c64*,
               c128_launches, c128_hw60) / plain GEMM (their last blocks, c512_hw60, c1024, c24, c40, c48*, u32)
               plan.local (TLSC): not reached -- NAFNetLocal is inference only, a taped forward raises (test_gpu_tlsc.py)
  _ffn_bwd_launches  dgrad_sg_rc_wg (c32, c32_wide, u32) / dgrad_sg_rc (c32_unfolded) / CM_SGBWD (the other 16-bit cases
               off the rows path) / fp32 (controls); dgrad_ln_bwd at C 32 .. 256 / GEMM + ln_bwd_nhwc (c512_hw60, c1024,
               c24, c40, c48*); chandot epilogue (c128_launches) / img_chan_dot (all others off the rows path)
  _ffn_bwd_rows  without pend (the last block) and with pend (first / inner) in c128_rows, c256_rows, c512_*rows
  _block_bwd   sca_bwd_fused (c24, c40, c48_sca_unfolded, c32_unfolded); sca_c1dw_bwd_tile (c32, c32_wide,
               c32_stored_t4, c64, c64_wide, u32) / c1dw_bwd_tile (c32_unfolded); sca_dw_bwd (c64_stored_tape, c128*,
               c256_rows, c512*, c1024, c48) / sca_sg_dw_bwd (c48_sca_unfolded) / sca_sg_bwd + dw_bwd (c24, c40);
               dgrad_ln_bwd_wg (c32*, u32 but c32_unfolded); defer (inner / last blocks of the rows cases) / _conv1_bwd with
               the epilogue (C 64 .. 256) or stand-alone (c512_rows' first block, c512_hw60, c1024, c24, c40, c48*)
               the two "not expected" resolutions of a pending deferral (a non-block record, or a block off the rows
               path, after a deferring block): not reachable, the walker defers only after looking at that very record

Worst error / bound over the tensors of a case, measured on an MI355X (bf16, fp16):
  c32 0.352 0.515 | c32_wide 0.515 0.347 | c32_stored_t4 0.275 0.385 | c32_unfolded 0.352 0.515
  c64 0.391 0.384 | c64_wide 0.435 0.381 | c64_stored_tape 0.426 0.426
  c128_rows 0.388 0.416 (hooked: the same) | c128_launches 0.455 0.345 | c128_hw60 0.420 0.397 | c256_rows 0.378 0.646
  c512_c1dw_rows 0.400 0.441 | c512_rows 0.367 0.434 | c512_hw60 0.502 0.361 | c1024 0.439 0.399
  c24 0.370 0.377 | c40 0.257 0.345 | c48 0.250 0.410 | c48_sca_unfolded 0.388 0.413
  u32 0.356 0.939 (fp16: decoders.0.0.conv2.bias[85]; the next tensor is at 0.570)
  fp32 controls: out <= 0.025 of its tolerance, gradients <= 0.002.
The U-shaped case is the one whose inputs matter: with inputs chosen on fewer host realisations it missed in bf16 (1.61
at encoders.1.0.conv1.bias[5], then 1.16 at encoders.0.0.conv2.bias[35]) while fp16 and every launch of those blocks in
c32 / c64 passed; host realisations of the emulation alone missed the same bound at those inputs, so they were replaced
under a stronger host condition (block_oracle._SEEDS).
"""
import functools

import pytest
import torch

import block_oracle as bo

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _oracle(name):
    torch.set_num_threads(16)
    case = {c.name: c for c in bo.CASES + bo.FP32_CASES}[name]
    return bo.run_case(case, None)


def _device_run(dev, case, precision, on_stage=None):
    """(results in reference layout on the host, {block prefix: BlockPlan}, the network, the gradient buffer).
    on_stage(stage, dflat): called as the gradient-ready hook."""
    from lowlight_image_enhancement_amd.nafnet import NAFNet
    sd, x, dout = bo.case_inputs(case)
    net = NAFNet(**case.ctor)
    net.load_state_dict(sd)
    net = net.to(dev)
    net.precision = precision
    for k, v in case.switches.items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    out, tape = net.exec_forward(x.to(dev), save=True)
    plans = {rec[1]: rec[4] for rec in tape if rec[0] == "block"}
    dflat = torch.full((net.numel,), float("nan"), device=dev)
    hook = None if on_stage is None else (lambda stage: on_stage(stage, dflat))
    dx = net.exec_backward(tape, dout.to(dev), dflat, need_dx=True, hook=hook)
    torch.cuda.synchronize()
    got = {"out": out.double().cpu(), "dx": dx.double().cpu()}
    for k, e in net.entries.items():
        got[k] = net._to_reference(e, dflat[e.offset:e.offset + e.numel]).double().cpu()
    return got, plans, net, dflat


def _check_plans(case, plans):
    assert list(plans) == bo.block_prefixes(case.ctor)
    for pre, plan in plans.items():
        for field, want in bo.expected_plan(case, pre).items():
            assert getattr(plan, field) == want, (case.name, pre, field, getattr(plan, field), want)


def _check_bound(tag, got, ref, emu):
    for name, t in got.items():
        assert torch.isfinite(t).all(), (tag, name, "not finite: a gradient element no launch wrote, or an overflow")
    r = bo.ratios(got, ref, emu)
    print(f"[{tag}] worst error / bound: " + ", ".join(f"{v:.3f} {n} {list(i)}" for v, n, i in r[:5]))
    over = [t for t in r if t[0] > 1.0]
    assert not over, (tag, over[:5])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", bo.CASES, ids=[c.name for c in bo.CASES])
def test_block_paths_per_element(dev, case, dtype):
    got, plans, _, _ = _device_run(dev, case, dtype)
    _check_plans(case, plans)
    torch.set_num_threads(16)
    _check_bound(f"{case.name} {dtype}", got, _oracle(case.name), bo.run_case(case, dtype))


@pytest.mark.parametrize("case", bo.FP32_CASES, ids=[c.name for c in bo.FP32_CASES])
def test_fp32_controls(dev, case):
    """The harness itself (weights, layouts, the tape walk) with nothing rounded: the suite's fp32 tolerances."""
    got, plans, _, _ = _device_run(dev, case, "fp32")
    assert list(plans) == bo.block_prefixes(case.ctor)
    ref = _oracle(case.name)
    worst = []
    for name, r in ref.items():
        assert torch.isfinite(got[name]).all(), name
        err = (got[name].reshape(r.shape) - r).abs().max().item()
        tol = 1e-4 if name == "out" else 1e-3 * r.abs().max().item() + 1e-7
        worst.append((err / tol, name))
        assert err <= tol, (name, err, tol)
    print(f"[{case.name}] worst error / tolerance:", sorted(worst, reverse=True)[:5])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gradient_ready_hook_sees_final_slices(dev, dtype):
    """With a gradient-ready hook every stage's slice is complete when the hook runs: cloned inside the hook it is
    bitwise what the buffer holds at the end, each stage is announced once, and the run passes the same bound."""
    case = bo.CASE["c128_rows"]
    seen = {}

    def on_stage(stage, dflat):
        assert stage.name not in seen, stage.name
        seen[stage.name] = (stage.lo, stage.hi, dflat[stage.lo:stage.hi].clone())

    got, plans, net, dflat = _device_run(dev, case, dtype, on_stage)
    _check_plans(case, plans)
    assert list(seen) == list(net.stages)
    for name, (lo, hi, snap) in seen.items():
        assert torch.equal(snap.view(torch.int32), dflat[lo:hi].view(torch.int32)), name
    torch.set_num_threads(16)
    _check_bound(f"{case.name} {dtype} hooked", got, _oracle(case.name), bo.run_case(case, dtype))
