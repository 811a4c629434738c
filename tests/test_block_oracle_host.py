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

The local window (block_oracle.LOCAL_CASES, NAFNetLocal forward only, `out` alone):
* local_pool restates test_tlsc_host.tlsc_pool64 bit for bit, and the float64 local oracle reproduces the reference's
  NAFNetLocal outputs of tests/golden/tlsc_nets.npz at test_oracle_golden.py's tolerance for a network output (atol 2e-5,
  rtol 1e-5; measured 2.5e-6, 2.1e-6, 1.2e-6, 5.3e-6 at A .. D, the plain oracle 0.32, 0.14, the same, 0.22);
* the case table meets its window requirements (every block local, even and odd k1 / k2, one case local in width only,
  one in height only, B = 2);
* identity-q equals the local oracle (1e-12) at every case; the stand-in within 2 x and its jittered realisations
  (3, 12 at loc_u32) within 3 x the emulation's error in both types;
* three planted errors in one inner block of the stand-in (the second of three; the middle block of loc_u32) -- it pools
  globally / its gather is off by one both ways / every image takes image 0's attention map -- each exceed the bound at
  every case in BOTH types.  bf16 "shift" / "image" were to be asserted wherever the host ratio is >= 1 and listed
  where not: it is >= 1 at every case of the table (least 1.46, loc_c64 "shift"), so nothing is listed and all 96
  combinations are asserted.  The same holds for the blended frame of the tiled test (block_oracle.TILED).

Measured per case: stand-in / jittered ratio to the emulation's error, then error / bound of global, shift, image:
    case                 bf16                                fp16
    loc_c32              1.00 1.21 |  3.13  2.16  2.22       0.91 1.12 | 27.9  18.2  20.3
    loc_c32_wide         1.00 1.20 |  1.77  1.49  2.25       0.99 1.13 | 13.4  10.8  16.1
    loc_c64              1.00 1.40 |  3.62  1.46  1.97       1.01 1.17 | 21.3   9.8  11.9
    loc_c64_wide         1.00 1.10 |  4.16  2.59  2.99       1.07 1.13 | 34.7  21.8  24.9
    loc_c64_stored_tape  1.00 1.07 |  4.06  3.00  5.18       0.99 1.14 | 39.9  29.4  51.7
    loc_c128_rows        1.00 0.92 |  4.19  2.99  3.57       0.99 1.42 | 34.0  26.4  28.9
    loc_c128_launches    1.00 1.14 |  4.51  4.20  7.05       0.93 1.15 | 35.0  31.9  55.0
    loc_c128_hw60        1.00 1.00 |  3.00  3.00  1.73       0.99 1.00 | 24.8  26.1  14.8
    loc_c256_rows        1.00 1.01 |  5.28  3.20  4.34       1.22 1.31 | 44.6  26.9  35.8
    loc_c512_c1dw_rows   1.00 1.01 |  1.79  1.82  1.90       0.98 1.10 | 13.1  12.8  13.7
    loc_c512_rows        1.02 1.15 |  4.83  4.78  5.38       1.04 1.20 | 37.5  36.5  41.2
    loc_c1024            0.99 1.01 |  3.19  2.55  2.80       0.97 0.75 | 18.5  14.4  15.9
    loc_c24              1.00 1.17 |  3.61  2.56  2.84       0.99 1.43 | 27.6  21.3  22.8
    loc_c40              1.00 1.24 |  6.23  4.52  4.80       0.98 1.32 | 56.7  43.3  43.6
    loc_c48              1.00 1.17 |  3.06  2.30  2.44       0.99 1.02 | 22.3  18.1  17.9
    loc_u32              1.01 1.05 |  1.95  2.78  1.77       1.07 1.20 | 17.3  26.0  17.7
    tiled frame          1.00 1.11                           0.95 1.18
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


# ---------------------------------------------------------------------------------------------- the local window
@functools.lru_cache(maxsize=None)
def _lref(name):
    torch.set_num_threads(16)
    return bo.run_case(bo.LOCAL_CASE[name], None)


@functools.lru_cache(maxsize=None)
def _lemu(name, dtype):
    torch.set_num_threads(16)
    return bo.run_case(bo.LOCAL_CASE[name], dtype)


_LOCAL_IDS = [c.name for c in bo.LOCAL_CASES]


def test_local_pool_is_the_pinned_helper():
    """block_oracle.local_pool restates test_tlsc_host.tlsc_pool64 (pinned there to the reference's AvgPool2d)."""
    from test_tlsc_host import tlsc_pool64
    gen = torch.Generator().manual_seed(3)
    for shape, k in [((2, 3, 12, 10), (6, 6)), ((1, 2, 9, 70), (9, 3)), ((2, 2, 16, 16), (3, 16)), ((1, 4, 7, 9), (4, 7)),
                     ((1, 2, 6, 5), (2, 3))]:
        x = torch.randn(shape, generator=gen, dtype=torch.float64)
        V, iy, ix = bo.local_pool(x, k)
        rv, rp = tlsc_pool64(x, k)
        assert torch.equal(V, rv) and torch.equal(V[:, :, iy][:, :, :, ix], rp), (shape, k)


@pytest.mark.parametrize("c", list("ABCD"))
def test_local_oracle_against_the_reference(c):
    """block_oracle.local_nafnet in float64 against the reference's NAFNetLocal outputs (tests/golden/tlsc_nets.npz), at
    test_oracle_golden.py's tolerance for a network output (atol 2e-5, rtol 1e-5)."""
    from conftest import golden
    from param_recipe import recipe_state
    from test_tlsc_host import case_cfg
    g = golden("tlsc_nets.npz")
    cfg = case_cfg(g, c)
    shapes = bo.O.nafnet_param_shapes(cfg["img_channel"], cfg["width"], cfg["middle_blk_num"], cfg["enc_blk_nums"],
                                      cfg["dec_blk_nums"])
    P = {n: v.double() for n, v in recipe_state(shapes, int(g[c + "_seed"])).items()}
    kern = bo.tlsc_kernels(cfg, tuple(int(v) for v in g[c + "_train"]))
    lq = torch.from_numpy(g[c + "_lq"]).double()
    with torch.no_grad():
        out = bo.local_nafnet(P, lq, cfg["enc_blk_nums"], cfg["middle_blk_num"], cfg["dec_blk_nums"], kern)
        plain = bo.O.nafnet(P, lq, cfg["enc_blk_nums"], cfg["middle_blk_num"], cfg["dec_blk_nums"])
    ref = torch.from_numpy(g[c + "_out"]).double()
    err = (out - ref).abs().max().item()
    print(f"case {c}: max |local oracle - reference| = {err:.3e}, |plain oracle - reference| = "
          f"{(plain - ref).abs().max().item():.3e}")
    assert torch.allclose(out, ref, atol=2e-5, rtol=1e-5), err
    if c == "C":  # every block global
        assert torch.equal(out, plain)
    else:  # the fixture tells the local oracle from the global one
        assert not torch.allclose(plain, ref, atol=2e-5, rtol=1e-5)


def test_local_case_table_meets_its_requirements():
    """Every block of every local case has a window smaller than its map in at least one direction; even and odd k1
    and k2 occur; one case is local in width only and one in height only; B >= 2 everywhere."""
    k1s, k2s, width_only, height_only = set(), set(), [], []
    for case in bo.LOCAL_CASES:
        assert case.shape[0] >= 2, case.name
        L = len(case.ctor["enc_blk_nums"])
        wins = bo.block_windows(case)
        assert list(wins) == bo.block_prefixes(case.ctor)
        for pre, win in wins.items():
            assert win is not None, (case.name, pre)
            k1s.add(win[0] % 2)
            k2s.add(win[1] % 2)
        if L == 0:
            H, W = case.shape[1:]
            win = wins["middle_blks.0."]
            assert win[0] < H or win[1] < W
            if win[0] == H:
                width_only.append(case.name)
            if win[1] == W:
                height_only.append(case.name)
    assert k1s == {0, 1} and k2s == {0, 1}
    assert width_only == ["loc_c32_wide"] and height_only == ["loc_c512_c1dw_rows"]


@pytest.mark.parametrize("name", _LOCAL_IDS)
def test_local_identity_q_is_the_oracle(name):
    case = bo.LOCAL_CASE[name]
    sd, x, _ = bo.case_inputs(case)
    P = {n: v.double() for n, v in sd.items()}
    k = case.ctor
    with torch.no_grad():
        out = bo.emulated_nafnet(P, x.double(), k["enc_blk_nums"], k["middle_blk_num"], k["dec_blk_nums"],
                                 bo.make_q(None), kernels=bo.tlsc_kernels(k, case.train_size))
    ref = _lref(name)
    assert set(ref) == {"out"}
    err = (out - ref["out"]).abs().max().item()
    assert err <= 1e-12 * max(1.0, ref["out"].abs().max().item()), err


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _LOCAL_IDS)
def test_local_stand_in_within_twice_the_emulation(name, dtype):
    """test_float32_stand_in_within_twice_the_emulation for the local cases (forward only: `out` alone)."""
    case = bo.LOCAL_CASE[name]
    ref, emu = _lref(name), _lemu(name, dtype)
    worst = _worst_ratio(bo.run_case(case, dtype, torch.float32), ref, emu, 2.0)
    nj = 12 if case.ctor["enc_blk_nums"] else 3
    wj = max(_worst_ratio(bo.run_case(case, dtype, torch.float32, jitter=j), ref, emu, 3.0) for j in range(1, nj + 1))
    print(f"[{name} {dtype}] stand-in / emulation error ratio {worst[0]:.2f}, worst of {nj} jittered {wj[0]:.2f}")


LOCAL_REQUIRED = [(c, d, m) for c in _LOCAL_IDS for d in DTYPES for m in bo.LOCAL_MUTATIONS]


@pytest.mark.parametrize("name,dtype,mutation", LOCAL_REQUIRED, ids=["-".join(r) for r in LOCAL_REQUIRED])
def test_local_planted_error_exceeds_the_bound(name, dtype, mutation):
    case = bo.LOCAL_CASE[name]
    ref, emu = _lref(name), _lemu(name, dtype)
    alt = bo.run_case(case, dtype, torch.float32, mutate=(bo.mutated_block(case), mutation))
    r = bo.ratios(alt, ref, emu)[0][0]
    print(f"[{name} {dtype} {mutation}] error / bound {r:.2f}")
    assert r > 1.0, r  # in bf16 too: no case of the table is below 1 (module docstring)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiled_stand_in_within_twice_the_emulation(dtype):
    """The blended frame of the tiled test (block_oracle.TILED): the same two host conditions."""
    ref, emu = bo.run_tiled(None), bo.run_tiled(dtype)
    worst = _worst_ratio(bo.run_tiled(dtype, torch.float32), ref, emu, 2.0)
    wj = max(_worst_ratio(bo.run_tiled(dtype, torch.float32, jitter=j), ref, emu, 3.0) for j in range(1, 4))
    print(f"[tiled {dtype}] stand-in / emulation error ratio {worst[0]:.2f}, worst of 3 jittered {wj[0]:.2f}")


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
