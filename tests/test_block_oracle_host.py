"""The block oracle's own checks, on the host (tests/block_oracle.py; the device test is test_gpu_block_oracle.py).

* with the identity for q the emulation IS the oracle (1e-12), so every difference between the two is a rounding;
* an independent stand-in for the device -- the same rounding points, every operation between them in float32
  (correctly rounded: float64 operations, each result rounded to float32, the same numbers on every host) -- stays
  within 2 x the emulation's error + the floor on every tensor of every case and both 16-bit types: the condition under
  which the device bound's factor 4 leaves a margin of two; jittered realisations of it (3 per type, 12 at the U-shaped
  case) stay within 3 x;
* the bound has power: three planted errors of the kind a kernel or its launch could make, each in the second block of
  the stand-in, each push at least one tensor over the bound.

Measured ratios (worst tensor's error / bound, mutation in middle_blks.1):
    case        type   tap    sca    pair
    c32         fp16    9.5   93.0   92.7
    c32         bf16    1.3    7.3    8.6
    c128_rows   fp16   23.8   103    808
    c128_rows   bf16    1.8    8.1    158
The single-tap error is one pixel of one block: it clears the bf16 bound by little, but it does clear it at both widths,
so all three are required in both types.
"""
import functools

import pytest
import torch

import block_oracle as bo

DTYPES = ("bf16", "fp16")


@functools.lru_cache(maxsize=None)
def _ref(name):
    torch.set_num_threads(16)
    return bo.run_case(bo.CASE[name], None)


@functools.lru_cache(maxsize=None)
def _emu(name, dtype):
    torch.set_num_threads(16)
    return bo.run_case(bo.CASE[name], dtype)


@pytest.mark.parametrize("name", ["c32", "c24", "u32"])
def test_identity_q_is_the_oracle(name):
    ref = _ref(name)
    case = bo.CASE[name]
    sd, x, dout = bo.case_inputs(case)
    P = {n: v.double().requires_grad_(True) for n, v in sd.items()}
    x = x.double().requires_grad_(True)
    k = case.ctor
    out = bo.emulated_nafnet(P, x, k["enc_blk_nums"], k["middle_blk_num"], k["dec_blk_nums"], bo.make_q(None))
    out.backward(dout.double())
    got = {"out": out.detach(), "dx": x.grad, **{n: v.grad for n, v in P.items()}}
    assert set(got) == set(ref)
    for n, r in ref.items():
        err = (got[n] - r).abs().max().item()
        assert err <= 1e-12 * max(1.0, r.abs().max().item()), (n, err)


def _worst_ratio(alt, ref, emu, factor):
    """max over the tensors of err(alt) / (err(emu) + floor / factor), asserted <= factor on each."""
    worst = (0.0, None)
    for n, r in ref.items():
        e_emu = (emu[n] - r).abs().max().item()
        e_alt = (alt[n] - r).abs().max().item()
        floor = bo.FLOOR * r.abs().max().item()
        worst = max(worst, (e_alt / (e_emu + floor / factor) if e_emu + floor else 0.0, n))
        assert e_alt <= factor * e_emu + floor, (n, e_alt, e_emu)
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", bo.CASES, ids=[c.name for c in bo.CASES])
def test_float32_stand_in_within_twice_the_emulation(case, dtype):
    """The condition the inputs of a case must satisfy (block_oracle._SEEDS): the stand-in within 2 x the emulation's
    error + the floor on every tensor; and more realisations of the stand-in's rounding decisions (jitter 1, 2, ...:
    three, twelve at the U-shaped case) within 3 x, so that the one realisation the emulation is does not understate
    what the format costs a tensor."""
    ref, emu = _ref(case.name), _emu(case.name, dtype)
    worst = _worst_ratio(bo.run_case(case, dtype, torch.float32), ref, emu, 2.0)
    print(f"[{case.name} {dtype}] worst stand-in / emulation error ratio {worst[0]:.2f} ({worst[1]})")
    nj = 12 if case.ctor["enc_blk_nums"] else 3  # the U-shaped case's errors have a heavy tail (block_oracle._SEEDS)
    wj = max(_worst_ratio(bo.run_case(case, dtype, torch.float32, jitter=j), ref, emu, 3.0) for j in range(1, nj + 1))
    print(f"[{case.name} {dtype}] worst of {nj} jittered realisations {wj[0]:.2f} ({wj[1]})")


REQUIRED = [(c, d, m) for c in ("c32", "c128_rows") for d in DTYPES for m in bo.MUTATIONS]


@pytest.mark.parametrize("name,dtype,mutation", REQUIRED, ids=["-".join(r) for r in REQUIRED])
def test_planted_error_exceeds_the_bound(name, dtype, mutation):
    case = bo.CASE[name]
    ref, emu = _ref(name), _emu(name, dtype)
    alt = bo.run_case(case, dtype, torch.float32, mutate=("middle_blks.1.", mutation))
    r = bo.ratios(alt, ref, emu)
    over = [t for t in r if t[0] > 1.0]
    print(f"[{name} {dtype} {mutation}] {len(over)} of {len(r)} tensors over the bound, worst {r[0][0]:.1f} x ({r[0][1]})")
    assert over, r[:3]
