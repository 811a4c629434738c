"""The down / up level convolutions on the device, per element against the float64 oracle of tests/level_conv_oracle.py.

The launches are the ones the executor issues (nafnet.py _down_fwd, _up_fwd and the "up" / "down" arms of
_walk_backward), through _lib.call:

  down_fwd    gemm   A = x [B,2gh,2gw,cs] (space-to-depth gather, a_mode 1)   C [M,2cs]              bias
  up_fwd      gemm   A = x [M,2cs]   C [B,2gh,2gw,cs] (depth-to-space scatter, c_mode 1)             R = skip
  up_dgrad    gemm   A = dfeat [B,2gh,2gw,cs] (a_mode 1), transposed weight   C [M,2cs]
  down_dgrad  gemm   A = dfeat [M,2cs], transposed weight   C [B,2gh,2gw,cs] (c_mode 1)              R = dskip
  dW / db     wgrad_f32 with the gathered operand (small shapes only)

"gemm" is nbp_gemm_bf16 for bf16 / fp16 (the 16-bit weight and its transposed copy made by nbp_weights_bf16 from a flat
fp32 buffer, as NAFNet._prep_weights does) and nbp_gemm_f32 for fp32 (b_nk 1 forward, b_nk 0 for the input gradients).
M = B gh gw; the S2D family (down_fwd, up_dgrad) has N = 2cs, K = 4cs, the D2S family (up_fwd, down_dgrad) N = 4cs,
K = 2cs.  Weights reach the device through NAFNet._to_internal, weight gradients return through _to_reference,
activations go NCHW <-> NHWC; this module holds no tap or sub-pixel permutation of its own.

Every output buffer is pre-filled with NaN and carries a 256-element sentinel tail that must be unchanged after the
launch.  Every element must lie inside the oracle's derived bound (level_conv_oracle.bound); nothing is excluded.
Every 16-bit case that can take the LDS-DMA kernel runs twice, as is and with NBP_GLDS=0 (the register-staged kernel),
both held to the oracle.  dW / db use the project's weight-gradient tolerances (_check of test_gpu_wgrad_full.py for
the 16-bit types, close(atol=2e-4, rtol=1e-5) of test_gemm_nt_nn_against_torch for fp32): a worst-case bound grows like
M where a wrong permutation is off by sqrt(M).

Each case asserts the kernel variant it is named for through a pure-Python mirror of dispatch() / launch() /
glds_auto_depth (csrc/gemm16_impl.h) and dispatch_tiles() (csrc/gemm.hip), with the device's CU count.  Variants:
("reg", BM, BN, BK) the register-staged 16-bit kernel, ("dma", BM, BN, ring depth, threads) the LDS-DMA one,
("f32", BM, BN) the fp32 kernel.  Case -> variant (256 CUs):

  case (B, gh x gw, cs)        16-bit S2D              16-bit D2S              fp32 S2D / D2S
  s8    3,   5 x 7,     8      reg 64x64 BK32          reg 64x64 BK32          64x64 / 64x64
  s16   3,   5 x 7,    16      dma 64x64 d4            reg 64x64 BK32          64x64 / 64x64
  s24   2,   9 x 6,    24      dma 64x64 d4 (K tail)   dma 64x64 d4 (K tail)   64x64 / 64x64   (N % 64 != 0, ragged M)
  s64   2,   7 x 11,   64      dma 64x64 d4            dma 64x64 d4            64x128 / 64x128
  s128  3,   5 x 7,   128      dma 64x64 d4            dma 64x64 d4            64x128 / 64x128
  a     3, 128 x 130,  32      dma 64x64 d2
  b     4, 128 x 128,  32      dma 128x64 d3 (exactly 512 tiles)
  c     4, 128 x 129,  32      dma 128x64 d2
  d     4,  64 x 64,  256      dma 128x128 d2, 512 threads
  e     2,  64 x 64,  256                              dma 128x128 d2, 512 threads
  f     1, 127 x 129,  48                              dma 64x128 d3, 512 threads (K tail)
  g     1, 100 x 82,   32                              dma 64x64 d4, 258 tiles
  h     2, 128 x 130,  32      dma 64x64 d3 (520 tiles)
  x     4,  64 x 64,  256                                                      64x128 / 128x128 (N 1024, K 512, M 16384)
  y     4, 128 x 256,  16                                                      128x64 / 128x64
  z     4, 128 x 256,  64                                                      128x128 / 128x128
  (each DMA variant also runs as ("reg", BM, BN, 64) under NBP_GLDS=0)

Measured on the MI355X, worst |device - oracle| / bound over the case's GEMM ops, per case and type (the DMA and the
NBP_GLDS=0 runs gave the same figure everywhere).  The 16-bit figures sit just under 1: the store's rounding is the
whole bound there; the fp32 figures show the accumulation term alone.  No check failed at the first run.

  case   bf16    fp16    fp32          case   bf16    fp16          case   fp32
  s8     0.975   0.968   0.073         a      0.985   0.935         x      0.006
  s16    0.982   0.973   0.045         b      0.988   0.932         y      0.076
  s24    0.991   0.947   0.029         c      0.987   0.938         z      0.025
  s64    0.984   0.897   0.019         d      0.853   0.438
  s128   0.958   0.843   0.009         e      0.949   0.730
                                       f      0.989   0.953
                                       g      0.991   0.972
                                       h      0.986   0.930
"""
import os

import pytest
import torch

import level_conv_oracle as lo
from test_gpu_wgrad_full import _check

pytestmark = pytest.mark.gpu

torch.set_num_threads(16)

S2D, D2S = "s2d", "d2s"
FAMILY = {"down_fwd": S2D, "up_dgrad": S2D, "up_fwd": D2S, "down_dgrad": D2S}
LDS = 160 * 1024


# ---------------------------------------------------------------------------------------------- dispatch mirror
def cdiv(a, b):
    return (a + b - 1) // b


def glds_auto_depth(blocks, stage_bytes, c_bytes, nmax, cus):
    per_cu = cdiv(blocks, cus)
    for d in range(nmax, 2, -1):
        if per_cu * max(d * stage_bytes, c_bytes) <= LDS:
            return d
    return 2


def variant16(M, N, K, fam, cs, cus, glds=True):
    """dispatch() + launch() of csrc/gemm16_impl.h for 16-bit A and C in the S2D / D2S modes (the skinny kernel and
    the 256 x 256 conv tiles serve neither)."""
    def blocks(bm, bn):
        return cdiv(M, bm) * cdiv(N, bn)
    n128, m128 = N > 64, M > 64
    if m128 and n128 and blocks(128, 128) >= 512:
        bm, bn = 128, 128
    elif m128 and blocks(128, 64) >= 512:
        bm, bn = 128, 64
    elif n128 and blocks(64, 128) >= 512:
        bm, bn = 64, 128
    else:
        bm, bn = 64, 64
    ldb = K
    aligned = cs % 8 == 0 if fam == S2D else K % 8 == 0  # S2D: the gathered rows; plain A: lda = K
    if glds and K > 32 and ldb % 8 == 0 and aligned:
        stb, cb = (bm + bn) * 128, bm * (bn + 4) * 4
        nmax = 4 if 4 * stb <= LDS and cb <= LDS else (3 if 3 * stb <= LDS else 2)
        return ("dma", bm, bn, glds_auto_depth(blocks(bm, bn), stb, cb, nmax, cus), 512 if bn >= 128 else 256)
    return ("reg", bm, bn, 32 if K <= 32 else 64)


def variant32(M, N):
    """dispatch_tiles() of csrc/gemm.hip"""
    bn128 = N >= 128
    bm128 = cdiv(M, 128) * cdiv(N, 128 if bn128 else 64) >= 1024
    return ("f32", 128 if bm128 else 64, 128 if bn128 else 64)


def test_dispatch_mirror_thresholds():
    """The mirror at the thresholds of the rules it restates (256 CUs)."""
    assert variant16(65536, 64, 128, S2D, 32, 256) == ("dma", 128, 64, 3, 256)  # exactly 512 tiles of 128 x 64
    assert variant16(65535 - 127, 64, 128, S2D, 32, 256)[1:3] == (64, 64)  # 511
    assert glds_auto_depth(512, 16384, 17408, 4, 256) == 4 and glds_auto_depth(513, 16384, 17408, 4, 256) == 3
    assert glds_auto_depth(769, 16384, 17408, 4, 256) == 2
    assert variant16(105, 16, 32, S2D, 8, 256) == ("reg", 64, 64, 32)
    assert variant16(105, 32, 64, S2D, 16, 256, glds=False) == ("reg", 64, 64, 64)
    assert variant32(16384, 1024) == ("f32", 128, 128) and variant32(16383 - 127, 1024) == ("f32", 64, 128)
    assert variant32(131072, 64) == ("f32", 128, 64) and variant32(131072 - 128, 64) == ("f32", 64, 64)


# ---------------------------------------------------------------------------------------------- cases
def _dma(bm, bn, d):
    return ("dma", bm, bn, d, 512 if bn >= 128 else 256)


# name -> (B, gh, gw, cs), {family: 16-bit variant}, {family: fp32 variant}; None: the case does not run that family /
# type.  The small shapes run everything.
CASES = {
    "s8": (lo.SMALL_SHAPES["s8"], {S2D: ("reg", 64, 64, 32), D2S: ("reg", 64, 64, 32)},
           {S2D: ("f32", 64, 64), D2S: ("f32", 64, 64)}),
    "s16": (lo.SMALL_SHAPES["s16"], {S2D: _dma(64, 64, 4), D2S: ("reg", 64, 64, 32)},
            {S2D: ("f32", 64, 64), D2S: ("f32", 64, 64)}),
    "s24": (lo.SMALL_SHAPES["s24"], {S2D: _dma(64, 64, 4), D2S: _dma(64, 64, 4)},
            {S2D: ("f32", 64, 64), D2S: ("f32", 64, 64)}),
    "s64": (lo.SMALL_SHAPES["s64"], {S2D: _dma(64, 64, 4), D2S: _dma(64, 64, 4)},
            {S2D: ("f32", 64, 128), D2S: ("f32", 64, 128)}),
    "s128": (lo.SMALL_SHAPES["s128"], {S2D: _dma(64, 64, 4), D2S: _dma(64, 64, 4)},
             {S2D: ("f32", 64, 128), D2S: ("f32", 64, 128)}),
    "a": ((3, 128, 130, 32), {S2D: _dma(64, 64, 2)}, None),
    "b": ((4, 128, 128, 32), {S2D: _dma(128, 64, 3)}, None),
    "c": ((4, 128, 129, 32), {S2D: _dma(128, 64, 2)}, None),
    "d": ((4, 64, 64, 256), {S2D: _dma(128, 128, 2)}, None),
    "e": ((2, 64, 64, 256), {D2S: _dma(128, 128, 2)}, None),
    "f": ((1, 127, 129, 48), {D2S: _dma(64, 128, 3)}, None),
    "g": ((1, 100, 82, 32), {D2S: _dma(64, 64, 4)}, None),
    "h": ((2, 128, 130, 32), {S2D: _dma(64, 64, 3)}, None),
    "x": ((4, 64, 64, 256), None, {S2D: ("f32", 64, 128), D2S: ("f32", 128, 128)}),
    "y": ((4, 128, 256, 16), None, {S2D: ("f32", 128, 64), D2S: ("f32", 128, 64)}),
    "z": ((4, 128, 256, 64), None, {S2D: ("f32", 128, 128), D2S: ("f32", 128, 128)}),
}
PRECS = ("bf16", "fp16", "fp32")


def _gemm_params():
    out = []
    for name, (_, v16, v32) in CASES.items():
        for prec in PRECS:
            table = v32 if prec == "fp32" else v16
            if table is None:
                continue
            for op, fam in FAMILY.items():
                if fam in table:
                    out.append(pytest.param(name, prec, op, id=f"{name}-{prec}-{op}"))
    return out


def _geometry(name, op):
    (B, gh, gw, cs), _, _ = CASES[name]
    M = B * gh * gw
    N, K = (2 * cs, 4 * cs) if FAMILY[op] == S2D else (4 * cs, 2 * cs)
    return B, gh, gw, cs, M, N, K


def _seed(name, prec):
    return 100 * list(CASES).index(name) + PRECS.index(prec)


# ---------------------------------------------------------------------------------------------- device helpers
SENTINEL = -7.0
TAIL = 256


def _guarded(shape, dtype, dev):
    """A NaN-filled output of `shape` in front of a 256-element sentinel tail: (view, whole buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.empty(n + TAIL, device=dev, dtype=dtype)
    buf[:n] = float("nan")
    buf[n:] = SENTINEL
    return buf[:n].view(shape), buf


def _tail_intact(buf):
    return bool((buf[-TAIL:] == SENTINEL).all())


def _device_weights(kind, w_ref, dt, dev):
    """(fp32 internal-layout weight, its 16-bit copy, the transposed 16-bit copy): a one-entry flat parameter buffer
    through nbp_weights_bf16, as NAFNet._prep_weights makes them."""
    from lowlight_image_enhancement_amd._lib import call
    flat = lo.to_internal(kind, w_ref.float()).to(dev)
    if dt == 0:
        return flat, None, None
    rows = w_ref.shape[0]
    desc = torch.tensor([[0, rows, flat.numel() // rows, -1]], dtype=torch.int64, device=dev)
    wb, wt = (torch.empty(flat.numel(), dtype=w_ref.dtype, device=dev) for _ in range(2))
    call("weights_bf16", flat, flat.numel(), wb, desc, 1, wt, dt)
    return flat, wb, wt


def _mm(dt, W, A, lda, amode, C, ldc, cmode, M, N, K, gh, gw, cs, bias=None, R=None, dgrad=False):
    """NAFNet._mm"""
    from lowlight_image_enhancement_amd._lib import call
    wf, wb, wt = W
    if dt == 0:
        call("gemm_f32", A, lda, amode, None, 1, wf, N if dgrad else K, 0 if dgrad else 1, C, ldc, cmode, M, N, K, gh,
             gw, cs, bias, R, None, None)
    else:
        call("gemm_bf16", A, lda, amode, None, 1, dt, wt if dgrad else wb, K, C, ldc, cmode, dt, M, N, K, gh, gw, cs,
             bias, R, None, None)


def _launch(op, inp, dt, dev):
    """One launch of `op` on the case's operands: (result as float64 NCHW, whole guarded buffer)."""
    B, gh, gw, cs = inp.B, inp.gh, inp.gw, inp.cs
    M, adt = B * gh * gw, lo.STORAGE[inp.prec]
    if op == "down_fwd":
        W = _device_weights("down", inp["down_w"], dt, dev)
        out, buf = _guarded((B, gh, gw, 2 * cs), adt, dev)
        _mm(dt, W, lo.nhwc(inp["down_x"]), 0, 1, out, 2 * cs, 0, M, 2 * cs, 4 * cs, gh, gw, cs, bias=inp["down_b"])
    elif op == "up_fwd":
        chan = 2 * cs
        W = _device_weights("up", inp["up_w"], dt, dev)
        out, buf = _guarded((B, 2 * gh, 2 * gw, chan // 2), adt, dev)
        _mm(dt, W, lo.nhwc(inp["up_x"]), chan, 0, out, 0, 1, M, 2 * chan, chan, gh, gw, chan // 2,
            R=lo.nhwc(inp["up_skip"]))
    elif op == "up_dgrad":
        chan = 2 * cs
        W = _device_weights("up", inp["up_w"], dt, dev)
        out, buf = _guarded((B, gh, gw, chan), adt, dev)
        _mm(dt, W, lo.nhwc(inp["up_dy"]), 0, 1, out, chan, 0, M, chan, 2 * chan, gh, gw, chan // 2, dgrad=True)
    else:
        W = _device_weights("down", inp["down_w"], dt, dev)
        out, buf = _guarded((B, 2 * gh, 2 * gw, cs), adt, dev)
        _mm(dt, W, lo.nhwc(inp["down_dy"]), 2 * cs, 0, out, 0, 1, M, 4 * cs, 2 * cs, gh, gw, cs,
            R=lo.nhwc(inp["down_res"]), dgrad=True)
    torch.cuda.synchronize()
    return lo.nchw(out).double(), buf


def _oracle(op, inp):
    """(ref, mag, Kc) of `op`: the matmul form, float64 on the operands' device."""
    cs = inp.cs
    if op == "down_fwd":
        return (*lo.down_out_mm(inp.f64("down_x"), inp.f64("down_w"), inp.f64("down_b")), 4 * cs)
    if op == "up_fwd":
        return (*lo.up_out_mm(inp.f64("up_x"), inp.f64("up_w"), inp.f64("up_skip")), 2 * cs)
    if op == "up_dgrad":
        return (*lo.up_dx_mm(inp.f64("up_dy"), inp.f64("up_w")), 4 * cs)
    dx, mag = lo.down_dx_mm(inp.f64("down_dy"), inp.f64("down_w"))
    res = inp.f64("down_res")
    return dx + res, mag + res.abs(), 2 * cs


def _with_glds(setting, fn):
    """fn() with NBP_GLDS unset ("auto") or "0"; the variable is restored (as run_modes of test_gpu_glds.py)."""
    old = os.environ.get("NBP_GLDS")
    try:
        if setting == "auto":
            os.environ.pop("NBP_GLDS", None)
        else:
            os.environ["NBP_GLDS"] = setting
        return fn()
    finally:
        if old is None:
            os.environ.pop("NBP_GLDS", None)
        else:
            os.environ["NBP_GLDS"] = old


# ---------------------------------------------------------------------------------------------- the GEMM ops
@pytest.mark.parametrize("name,prec,op", _gemm_params())
def test_level_conv_gemm(dev, name, prec, op):
    B, gh, gw, cs, M, N, K = _geometry(name, op)
    fam, dt = FAMILY[op], lo.DTYPE_CODE[prec]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    expect = CASES[name][2 if dt == 0 else 1][fam]
    if dt == 0:
        assert variant32(M, N) == expect, (variant32(M, N), expect)
        modes = ["auto"]
    else:
        got = variant16(M, N, K, fam, cs, cus)
        assert got == expect, (got, expect, cus)
        modes = ["auto"]
        if got[0] == "dma":  # the register-staged kernel on the same tile
            assert variant16(M, N, K, fam, cs, cus, glds=False) == ("reg", got[1], got[2], 64)
            modes.append("0")
    inp = lo.Inputs(B, gh, gw, cs, prec, _seed(name, prec), device=dev)
    ref, mag, kc = _oracle(op, inp)
    assert kc == K
    bnd = lo.bound(ref, mag, kc, prec)
    for mode in modes:
        got, buf = _with_glds(mode, lambda: _launch(op, inp, dt, dev))
        assert got.shape == ref.shape
        assert bool(torch.isfinite(got).all()), f"NBP_GLDS={mode}: NaN / inf left in the output"
        assert _tail_intact(buf), f"NBP_GLDS={mode}: the sentinel tail was written"
        ratio = lo.worst_ratio(got, ref, bnd)
        print(f"RATIO {name} {prec} {op} glds={mode} {ratio:.4f}")
        assert ratio <= 1.0, f"NBP_GLDS={mode}: worst |device - oracle| / bound = {ratio}"


# ---------------------------------------------------------------------------------------------- dW / db, dskip
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(lo.SMALL_SHAPES))
def test_level_conv_weight_gradients(dev, name, prec):
    from lowlight_image_enhancement_amd._lib import call, query
    from test_gpu_parity import close
    (B, gh, gw, cs), _, _ = CASES[name]
    M, dt = B * gh * gw, lo.DTYPE_CODE[prec]
    assert M <= 2048
    inp = lo.Inputs(B, gh, gw, cs, prec, _seed(name, prec), device=dev)
    host = {k: inp[k].cpu().double() for k in ("down_x", "down_w", "down_b", "down_dy", "up_x", "up_w", "up_skip",
                                               "up_dy")}
    d = lo.down_conv(host["down_x"], host["down_w"], host["down_b"], host["down_dy"])
    u = lo.up_conv(host["up_x"], host["up_w"], host["up_skip"], host["up_dy"])
    assert torch.equal(u["dskip"], host["up_dy"])  # d(skip) = d(up output): no launch

    def wgrad(G, ldg, gmode, X, ldx, xmode, N, K, csg, csx, bias):
        n_ws = query("wgrad_workspace_floats", M, N, K)
        ws = torch.full((n_ws,), float("nan"), device=dev)
        dW, wbuf = _guarded((N * K,), torch.float32, dev)
        db, bbuf = _guarded((N,), torch.float32, dev) if bias else (None, None)
        call("wgrad_f32", G, ldg, gmode, X, ldx, xmode, None, 1, M, N, K, gh, gw, csg, csx, dW, db, ws, n_ws, dt)
        torch.cuda.synchronize()
        assert _tail_intact(wbuf) and (bbuf is None or _tail_intact(bbuf))
        return dW, db

    def check(dW_ref_layout, db, ref, bref):
        assert bool(torch.isfinite(dW_ref_layout).all())
        if dt == 0:
            close(dW_ref_layout.double(), ref.numpy(), atol=2e-4, rtol=1e-5)
            if db is not None:
                close(db.double(), bref.numpy(), atol=2e-4, rtol=1e-5)
        else:
            zero = torch.zeros(1, dtype=torch.float64)
            _check(dW_ref_layout.cpu().reshape(-1), zero if db is None else db.cpu(), ref,
                   zero if db is None else bref, M)

    # up (nafnet.py _walk_backward "up"): G = the gathered PixelShuffle output gradient, X = the up conv's input
    chan = 2 * cs
    dW, _ = wgrad(lo.nhwc(inp["up_dy"]), 0, 1, lo.nhwc(inp["up_x"]), chan, 0, 2 * chan, chan, chan // 2, 0, False)
    check(lo.to_reference("up", host["up_w"].shape, dW), None, u["dW"], None)
    # down ("down"): G = the down conv's output gradient, X = the gathered input
    dW, db = wgrad(lo.nhwc(inp["down_dy"]), 2 * cs, 0, lo.nhwc(inp["down_x"]), 0, 1, 2 * cs, 4 * cs, 0, cs, True)
    check(lo.to_reference("down", host["down_w"].shape, dW), db, d["dW"], d["db"])
