"""NAFNet (Scenario B) on MI355X: one flat fp32 parameter buffer + an executor over the HIP C-ABI.

Reference: NAFNet_base/basicsr/models/archs/NAFNet_arch.py:22-162 (NAFNet, NAFBlock, SimpleGate) and
arch_util.py:264-300 (LayerNorm2d).  Same constructor signature, same state_dict keys and tensor shapes
(checkpoints interchange with the reference); different internals:

* activations are NHWC between the intro and ending convs (channels contiguous for the 1x1 GEMMs, the
  per-pixel LayerNorm and the depthwise conv);
* all parameters live in ONE flat fp32 buffer (`self.flat`, the module's only nn.Parameter), laid out in
  reverse backward order so that gradient buckets for the data-parallel all-reduce are contiguous slices that
  complete in order; the optimizer, the global-norm clip and the all-reduce all run over that buffer;
* two weights are stored in the layout their kernels read: downs.i.weight as [2C][kh][kw][C] (the GEMM's K
  order over a space-to-depth gather) and ups.i.0.weight with its output rows grouped by PixelShuffle
  sub-position (r1, r2, c').  state_dict()/load_state_dict() convert to and from the reference layout.

The forward/backward executor launches the kernels of include/nbp.h on the current stream and keeps the
tensors the backward needs in a tape.  Which kernels a NAFBlock takes is decided in one place, once per block and
forward (NAFNet._plan_block -> BlockPlan, from the precision, the fusion switches and the library's support
queries); the plan is stored in the block's tape record and the backward follows it.  What one run carries between
its launches (the weight copies, the LayerNorm carry, the tensors a deferred launch still reads) is a _Run object
that the executor methods pass along; the module holds no per-run state but the pinned precision.
"""
from __future__ import annotations

import contextlib
import math
import os
import warnings
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import call, query

AM_PLAIN, AM_S2D, AM_SCALE = 0, 1, 2
CM_SG, CM_SGBWD = 4, 5  # SimpleGate forward / backward fused into the GEMM epilogue (bf16 mode)
CM_CHANDOT = 8  # dgrad with the SCA channel-dot partials in the epilogue (bf16 mode, C > 64)
CM_PLAIN, CM_D2S = 0, 1
LN_EPS = 1e-6
# csrc/c1dw_tile.hip's A/B variants of nbp_c1dw_bwd_tile (read there): with either set the tile backward has no
# SCA-folding form, so the executor launches the SCA backward on its own
C1DW_BWD_VARIANT = bool(os.environ.get("NBP_C1DW_BWD_TH") or os.environ.get("NBP_C1DW_BWD_BAL"))


@dataclass
class PEntry:
    key: str
    ref_shape: Tuple[int, ...]
    offset: int
    numel: int
    kind: str = "plain"  # plain | down | up | sg (conv4: SimpleGate pairs interleaved)


@dataclass
class Stage:
    name: str
    lo: int  # flat offsets [lo, hi) of the parameters whose gradients this stage completes
    hi: int


def _block_keys(pre: str, c: int):
    return [(pre + "beta", (1, c, 1, 1)), (pre + "gamma", (1, c, 1, 1)),
            (pre + "conv1.weight", (2 * c, c, 1, 1)), (pre + "conv1.bias", (2 * c,)),
            (pre + "conv2.weight", (2 * c, 1, 3, 3)), (pre + "conv2.bias", (2 * c,)),
            (pre + "conv3.weight", (c, c, 1, 1)), (pre + "conv3.bias", (c,)),
            (pre + "sca.1.weight", (c, c, 1, 1)), (pre + "sca.1.bias", (c,)),
            (pre + "conv4.weight", (2 * c, c, 1, 1)), (pre + "conv4.bias", (2 * c,)),
            (pre + "conv5.weight", (c, c, 1, 1)), (pre + "conv5.bias", (c,)),
            (pre + "norm1.weight", (c,)), (pre + "norm1.bias", (c,)),
            (pre + "norm2.weight", (c,)), (pre + "norm2.bias", (c,))]


def _ceil4(v):
    return (v + 3) // 4 * 4


PRECISIONS = ("fp32", "bf16", "fp16")


def pick_precision(setting: str, autocast_on: bool, autocast_dtype, width: int) -> Tuple[str, bool]:
    """(precision of one forward, whether to warn) from a NAFNet.precision setting and the ambient CUDA autocast state.
    An explicit "fp32" / "fp16" / "bf16" is returned as it is: autocast is ignored (and `dt` raises for a 16-bit
    setting on a width that is no multiple of 8).  "auto" follows the region as the reference's fp32 module does under
    it (image_restoration_model.py:255-257): fp32 outside an enabled region, the region's dtype inside one; a width
    that is no multiple of 8 (the reference runs any width under autocast, the 16-bit kernels need 16-byte channel
    vectors) stays fp32 there, with the warning flag set."""
    if setting in PRECISIONS:
        return setting, False
    if setting != "auto":
        raise ValueError(f"NAFNet precision must be 'auto', 'fp32', 'bf16' or 'fp16', got {setting!r}")
    if not autocast_on:
        return "fp32", False
    if autocast_dtype == torch.float16:
        name = "fp16"
    elif autocast_dtype == torch.bfloat16:
        name = "bf16"
    else:
        raise ValueError(f"NAFNet under torch.autocast: dtype {autocast_dtype} has no 16-bit kernels (float16 or "
                         "bfloat16)")
    if width % 8:
        return "fp32", True
    return name, False


class Tape(list):
    """The executor's tape: the records of one forward plus the precision that forward ran in.  The backward runs in
    the tape's precision whatever the module's setting or the autocast state is by then."""

    def __init__(self, precision: str):
        super().__init__()
        self.precision = precision


class Weights(NamedTuple):
    """The parameters as one run's kernels read them.  fp32 runs carry f32 alone."""
    f32: torch.Tensor  # the flat parameters
    h: Optional[torch.Tensor] = None  # 16-bit copy
    ht: Optional[torch.Tensor] = None  # 16-bit copy, GEMM weights transposed (the dgrad operands; layer scales folded in)
    frag: Optional[torch.Tensor] = None  # fragment-ordered copy of h (nbp_ffn_rows_fwd), None when no level takes it
    frag_t: Optional[torch.Tensor] = None  # fragment-ordered copy of ht (nbp_ffn_rows_bwd)


@dataclass(frozen=True)
class BlockPlan:
    """The kernel path of one NAFBlock, decided once by NAFNet._plan_block in the forward and recorded in the block's
    tape record: the backward obeys it and reads no switch, query or saved-tensor presence again."""
    tile: bool  # conv1 -> depthwise -> SimpleGate -> pool on the tile path: t1 / t2 never stored, rebuilt in the backward
    c1dw: bool  # the same chain as one whole-image launch (nbp_c1_dw_sg_pool), t1 / t2 stored
    chunks: int  # pool partials per image
    ln_epilogue: bool  # 16-bit at a width whose GEMM epilogues hold a LayerNorm (forward if ln_fwd; backward always)
    ln_fwd: bool  # norm2 in conv3's epilogue, the next block's norm1 in conv5's
    drop_t4: bool  # t4 not stored (level 0): the backward rebuilds it (nbp_dgrad_sg_rc*)
    ffn: bool  # conv4 -> SimpleGate -> conv5 as nbp_gemm_ffn, g2 not stored either
    rows_ffn: bool  # the FFN half, forward and backward, as the row-stationary launches (nbp_ffn_rows_fwd / _bwd)
    local: Optional[Tuple[int, int]]  # the TLSC window, None: the SCA pools globally
    carry_next: bool  # this block's last launch also makes the next block's norm1
    # backward only
    sg_rc_wg: bool  # with drop_t4: U5 / V5 and conv4's weight gradients folded into the rebuild pass
    ln_wg: bool  # conv1's weight gradients folded into the conv1 dgrad + norm1 backward (level 0)
    sca_fold: bool  # the SCA backward inside the depthwise backward
    grouped: bool  # the wide weight gradients join the level's grouped launch
    chandot: bool  # the SCA channel dot in conv3's dgrad epilogue
    rows_pre: bool  # the conv1 input gradient may be deferred into the preceding block's nbp_ffn_rows_bwd


@dataclass
class _Run:
    """What one exec_forward or one exec_backward carries from launch to launch."""
    w: Weights
    tape: Optional[Tape] = None  # forward: where the records go, None without a backward
    ln_carry: Optional[tuple] = None  # forward: (x, n1, st1) a block's epilogue made for the next block
    keep: List[torch.Tensor] = field(default_factory=list)  # backward: tensors awaiting a deferred launch / reduction
    grouping: bool = False  # backward: inside a level whose weight gradients are queued (nbp_wgrad_group open)


class NAFNet(nn.Module):
    """NAFNet(img_channel=3, width=16, middle_blk_num=1, enc_blk_nums=[], dec_blk_nums=[]) (NAFNet_arch.py:85)."""

    def __init__(self, img_channel=3, width=16, middle_blk_num=1, enc_blk_nums=[], dec_blk_nums=[]):  # noqa: B006
        super().__init__()
        if width < 4 or width % 4:
            raise ValueError("the MI355X NAFNet needs a width that is a multiple of 4 (16-byte channel vectors; the "
                             "16-bit precision modes need a multiple of 8)")
        if len(dec_blk_nums) != len(enc_blk_nums):
            raise ValueError("enc_blk_nums and dec_blk_nums must have the same length (U-Net skips)")
        if img_channel > 4:
            raise ValueError("img_channel <= 4")
        self.img_channel = img_channel
        self.width = width
        self.enc_blk_nums = list(enc_blk_nums)
        self.middle_blk_num = int(middle_blk_num)
        self.dec_blk_nums = list(dec_blk_nums)
        self.padder_size = 2 ** len(self.enc_blk_nums)
        self._build_layout()
        self.flat = nn.Parameter(torch.zeros(self.numel, dtype=torch.float32))
        self._init_reference_like()
        self.grad_ready_hook: Optional[Callable[[Stage], None]] = None
        # Fused / folded forms of the executor, all on (each measured faster; no environment knob toggles
        # them).  The attributes stay so that the GPU tests can compare a fused form bit for bit with its unfused one
        # on the same network.  _plan_block reads them once per block in the forward; a backward follows its tape.
        # LayerNorm forward in the conv3 / conv5 epilogues at C in {32, 64, 128, 256}
        self.fuse_ln_fwd = True
        # the wide (C >= 128) weight gradients of a whole U-Net level (conv5's U, conv4, conv3's U, conv1 of every
        # NAFBlock of the level) queued during the level's backward and launched as ONE grouped launch at its end,
        # with M-splits chosen for the group (False: one launch per weight gradient)
        self.group_wgrad = True
        # level 0 (C = 32): the conv4 output t4 is not stored; the conv5 dgrad rebuilds it per tile on MFMA
        # (nbp_dgrad_sg_rc, bitwise equal) ...
        self.sg_rc = True
        # ... and folds conv5's U / V and conv4's weight / bias gradients into the same pass over dout / n2 / dt
        # (nbp_dgrad_sg_rc_wg; False: separate nbp_wgrad_f32 launches)
        self.sg_rc_wg = True
        # level 0 with that rebuild: conv4 -> SimpleGate -> conv5 (+ residual + next LayerNorm) as one pass
        # (nbp_gemm_ffn, bitwise the two launches, +0.1 % step), g2 never stored
        self.fuse_ffn = True
        # levels with C in {128, 256, 512} (16-bit): conv3 -> norm2 -> conv4 -> SimpleGate -> conv5 (-> the next norm1)
        # in one row-stationary launch (nbp_ffn_rows_fwd; bitwise the launches it replaces)
        self.fuse_ffn_rows = True
        # backward at those levels: a block's conv1 input gradient + norm1 backward deferred into the preceding block's
        # row-stationary launch (nbp_ffn_rows_bwd with dt1: its dx made in LDS as that block's dout)
        self.ffn_rows_pre = True
        # the SCA backward (ds, the SCA weight gradients) inside the fused depthwise backward (nbp_sca_dw_bwd, on the tile
        # path nbp_sca_c1dw_bwd_tile) instead of its own launch before it
        self.sca_fold = True
        # level 0: conv1's weight / bias gradients folded into the conv1 dgrad + norm1 backward pass (nbp_dgrad_ln_bwd_wg:
        # n1 rebuilt from x and the LN statistics, dt1 already in registers; False: a separate nbp_wgrad_f32 launch)
        self.ln_wg = True
        # the middle level (16 x 16 at C 512): conv1 -> depthwise -> SimpleGate -> pool as one whole-image launch
        # (nbp_c1_dw_sg_pool; t1 / t2 / g bitwise, the pool up to fp32 summation order)
        self.fuse_c1dw = True
        # levels 0 / 1 (C 32 / 64, 16-bit): conv1 -> depthwise -> SimpleGate -> pool as one row-walking tile launch that
        # keeps t1 / t2 on chip (nbp_c1dw_fwd_tile), and the mirror backward that rebuilds them from n1
        # (nbp_c1dw_bwd_tile): the 2C-wide tape never reaches HBM
        self.fuse_c1dw_tile = True
        # the levels (by channel count) that take it: 0 and 1.  The rebuild costs the backward more VALU work than the
        # stored-tape kernel (t1 epilogue + t2 recomputed: 172 vs 150 us at level 0, 102 vs 73 at level 1), which the
        # forward's saved tape traffic repays (58 vs 109 us, 49 vs 57): graph step +1.1 % with both levels, +0.7 / +0.3 %
        # with level 0 / 1 alone
        self.c1dw_tile_channels = (32, 64)
        # {block prefix: TLSC kernel size}: set by NAFNetLocal only; None = every SCA pools globally
        self._local_kernels: Optional[Dict[str, Tuple[int, int]]] = None
        # "fp32": fp32 operands everywhere (parity mode); "fp16" / "bf16": 16-bit activation storage and MFMA operands
        # with fp32 accumulation, statistics, parameters and gradients (fp16 = the reference's AMP autocast dtype,
        # image_restoration_model.py:255; the trainer adds GradScaler-style dynamic loss scaling for it).  "auto" (the
        # default): resolved once per forward from the ambient CUDA autocast region (pick_precision), so the reference's
        # AMP step selects the 16-bit kernels with no attribute of this module set.
        self.precision = "auto"
        # the precision of the forward / backward the executor is running (set by exec_forward / exec_backward for their
        # duration; dt / adt read it): a backward runs in its tape's precision, not in a newly resolved one
        self._active: Optional[str] = None
        self._warned_width = False

        # 16-bit modes: the layer scales beta / gamma are folded into the transposed conv3 / conv5 weight copies (the
        # dgrad operands: dh = (beta (.) dy) W3 = dy (diag(beta) W3)), so those dgrads read A unscaled
        def _scale_off(k):
            for wk, sk in (("conv3.weight", "beta"), ("conv5.weight", "gamma")):
                if k.endswith(wk):
                    return self.entries[k[:-len(wk)] + sk].offset
            return -1
        self._tdesc_cpu = torch.tensor([[e.offset, e.ref_shape[0], e.numel // e.ref_shape[0], _scale_off(k)]
                                        for k, e in self.entries.items() if self._is_gemm_weight(k)],
                                       dtype=torch.int64).reshape(-1, 4)
        self._tdesc = None
        # the weights nbp_ffn_rows_fwd / _bwd read (conv3 / conv4 / conv5, and conv1 for the backward's deferred input
        # gradient, of the levels with C in {128, 256, 512}), {offset, rows, cols}
        self._fdesc_cpu = torch.tensor([[e.offset, e.ref_shape[0], e.numel // e.ref_shape[0]]
                                        for k, e in self.entries.items()
                                        if k.endswith(("conv1.weight", "conv3.weight", "conv4.weight", "conv5.weight"))
                                        and e.numel // e.ref_shape[0] in (128, 256, 512)],
                                       dtype=torch.int64).reshape(-1, 3)
        self._fdesc = None

    # ------------------------------------------------------------------ layout
    def _build_layout(self):
        w = self.width
        # reference registration order (for state_dict key order)
        ref: List[Tuple[str, Tuple[int, ...]]] = [("intro.weight", (w, self.img_channel, 3, 3)), ("intro.bias", (w,)),
                                                  ("ending.weight", (self.img_channel, w, 3, 3)),
                                                  ("ending.bias", (self.img_channel,))]
        chan = w
        enc_keys, downs = [], []
        self.enc_chans = []
        for i, n in enumerate(self.enc_blk_nums):
            self.enc_chans.append(chan)
            for j in range(n):
                enc_keys += _block_keys(f"encoders.{i}.{j}.", chan)
            downs += [(f"downs.{i}.weight", (2 * chan, chan, 2, 2)), (f"downs.{i}.bias", (2 * chan,))]
            chan *= 2
        self.mid_chan = chan
        mid_keys = []
        for j in range(self.middle_blk_num):
            mid_keys += _block_keys(f"middle_blks.{j}.", chan)
        dec_keys, ups = [], []
        self.dec_chans = []
        for i, n in enumerate(self.dec_blk_nums):
            ups += [(f"ups.{i}.0.weight", (2 * chan, chan, 1, 1))]
            chan //= 2
            self.dec_chans.append(chan)
            for j in range(n):
                dec_keys += _block_keys(f"decoders.{i}.{j}.", chan)
        self.ref_order = [k for k, _ in ref + enc_keys + dec_keys + mid_keys + ups + downs]
        shapes = dict(ref + enc_keys + dec_keys + mid_keys + ups + downs)

        # flat layout in reverse backward order: ending, decoders (last first), ups, middle, enc/downs, intro
        # ending.bias (img_channel floats, not a multiple of 4) goes last so no alignment padding is needed and
        # the flat buffer holds exactly the reference's parameter count
        groups: List[Tuple[str, List[str]]] = [("ending", ["ending.weight"])]
        for i in reversed(range(len(self.dec_blk_nums))):
            for j in reversed(range(self.dec_blk_nums[i])):
                groups.append((f"decoders.{i}.{j}", [k for k, _ in _block_keys(f"decoders.{i}.{j}.", 1)]))
            groups.append((f"ups.{i}", [f"ups.{i}.0.weight"]))
        for j in reversed(range(self.middle_blk_num)):
            groups.append((f"middle_blks.{j}", [k for k, _ in _block_keys(f"middle_blks.{j}.", 1)]))
        for i in reversed(range(len(self.enc_blk_nums))):
            groups.append((f"downs.{i}", [f"downs.{i}.weight", f"downs.{i}.bias"]))
            for j in reversed(range(self.enc_blk_nums[i])):
                groups.append((f"encoders.{i}.{j}", [k for k, _ in _block_keys(f"encoders.{i}.{j}.", 1)]))
        groups.append(("intro", ["intro.weight", "intro.bias", "ending.bias"]))
        self.entries: Dict[str, PEntry] = OrderedDict()
        self.stages: Dict[str, Stage] = OrderedDict()
        off = 0
        for gname, keys in groups:
            lo = off
            for k in keys:
                shp = shapes[k]
                n = 1
                for s in shp:
                    n *= s
                kind = "down" if k.startswith("downs.") and k.endswith("weight") else (
                    "up" if k.startswith("ups.") else ("sg" if ".conv4." in k else "plain"))
                self.entries[k] = PEntry(k, shp, off, n, kind)
                off += n if k == "ending.bias" else _ceil4(n)  # 16-byte aligned slices for float4 access
            self.stages[gname] = Stage(gname, lo, off)
        self.numel = off

    @staticmethod
    def _is_gemm_weight(k: str) -> bool:
        return k.endswith(("conv1.weight", "conv3.weight", "conv4.weight", "conv5.weight")) or (
            k.startswith(("downs.", "ups.")) and k.endswith("weight"))

    def _prep_weights(self, P: torch.Tensor) -> Weights:
        """The weight set of one run: P alone in fp32; else + its 16-bit copy + transposed copies of the GEMM weights (for
        the dgrads) + fragment-ordered copies of the deep levels' conv3 / conv4 / conv5 weights (nbp_ffn_rows_fwd; None
        when no level takes it)."""
        if self.dt == 0:
            return Weights(P)
        if self._tdesc is None or self._tdesc.device != P.device:
            self._tdesc = self._tdesc_cpu.to(P.device)
            self._fdesc = self._fdesc_cpu.to(P.device) if self._fdesc_cpu.shape[0] else None
            self._fdesc_t = self._fdesc_cpu[:, [0, 2, 1]].contiguous().to(P.device)  # the transposed copies: [in][out]
        wb = torch.empty(self.numel, dtype=self.adt, device=P.device)
        wt = torch.empty(self.numel, dtype=self.adt, device=P.device)
        call("weights_bf16", P, self.numel, wb, self._tdesc, self._tdesc.shape[0], wt, self.dt)
        wf = wtf = None
        if self.fuse_ffn_rows and self._fdesc is not None:  # fragment-ordered copies (nbp_frag16): forward, transposed
            wf = torch.empty(self.numel, dtype=self.adt, device=P.device)
            call("frag16", wb, self._fdesc, self._fdesc.shape[0], wf)
            wtf = torch.empty(self.numel, dtype=self.adt, device=P.device)
            call("frag16", wt, self._fdesc_t, self._fdesc_t.shape[0], wtf)
        return Weights(P, wb, wt, wf, wtf)

    def resolved_precision(self) -> str:
        """The precision a forward started now would run in: the setting, or for "auto" what the ambient CUDA autocast
        region selects (pick_precision)."""
        name, warn = pick_precision(self.precision, torch.is_autocast_enabled("cuda"),
                                    torch.get_autocast_dtype("cuda"), self.width)
        if warn and not self._warned_width:
            self._warned_width = True
            warnings.warn(f"NAFNet(width={self.width}) under torch.autocast runs its fp32 kernels: the 16-bit modes need "
                          "a width that is a multiple of 8 (16-byte vectors of 16-bit channels)", RuntimeWarning,
                          stacklevel=2)
        return name

    @property
    def active_precision(self) -> str:
        """The pinned precision while the executor runs a forward or a backward, else resolved_precision()."""
        return self._active if self._active is not None else self.resolved_precision()

    @contextlib.contextmanager
    def _pinned(self, precision: str):
        """Run the executor in `precision`, out of reach of the ambient autocast region (as torch.amp.custom_fwd runs a
        function's body): dt / adt read the pin, no torch op inside is re-typed."""
        if precision not in PRECISIONS:
            raise ValueError(f"NAFNet executor precision must be 'fp32', 'bf16' or 'fp16', got {precision!r}")
        prev, self._active = self._active, precision
        try:
            with torch.autocast("cuda", enabled=False):
                yield
        finally:
            self._active = prev

    @property
    def adt(self) -> torch.dtype:
        """storage dtype of NHWC activations and activation gradients"""
        return {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[self.active_precision]

    @property
    def dt(self) -> int:
        """dtype code of the C-ABI: 0 fp32, 1 bf16, 2 fp16"""
        prec = self.active_precision
        d = {"fp32": 0, "bf16": 1, "fp16": 2}[prec]
        if d and self.width % 8:
            raise ValueError(f"precision {prec!r} needs a width that is a multiple of 8 (16-byte vectors of "
                             f"16-bit channels); width {self.width} runs in the fp32 mode")
        return d

    def _mm(self, W, A, lda, amode, ascale, rows, wkey, C, ldc, cmode, M, N, K, gh=0, gw=0, cs=0, bias=None,
            R=None, rscale=None, pre=None, dgrad=False):
        """One GEMM launch in the run's precision, W its Weights.
        forward: C[M,N] = A[M,K] . W[N,K]^T ; dgrad: C[M,N] = A[M,K] . W[K,N] (W stored [out=K][in=N])."""
        dt = self.dt
        if dt == 0:
            Wf = self._slice(W.f32, wkey)
            call("gemm_f32", A, lda, amode, ascale, rows, Wf, N if dgrad else K, 0 if dgrad else 1, C, ldc, cmode,
                 M, N, K, gh, gw, cs, bias, R, rscale, pre)
        else:
            Wb = self._slice(W.ht if dgrad else W.h, wkey)
            call("gemm_bf16", A, lda, amode, ascale, rows, dt, Wb, K, C, ldc, cmode, dt, M, N, K, gh, gw, cs,
                 bias, R, rscale, pre)

    # reference layout <-> internal layout
    def _to_internal(self, e: PEntry, t: torch.Tensor) -> torch.Tensor:
        if e.kind == "down":  # [2C, C, 2, 2] -> [2C, 2, 2, C]
            return t.permute(0, 2, 3, 1).reshape(-1)
        if e.kind == "sg":  # conv4 output rows h*C + c -> 2c + h: SimpleGate pairs adjacent (fused epilogues)
            n2 = t.shape[0]
            return t.reshape(2, n2 // 2, -1).permute(1, 0, 2).reshape(-1)
        if e.kind == "up":  # row n_ref = c'*4 + r1*2 + r2 -> n_int = (r1*2 + r2)*(C/2) + c'
            n2, c = t.shape[0], t.shape[1]
            return t.reshape(n2 // 4, 4, c).permute(1, 0, 2).reshape(-1)
        return t.reshape(-1)

    def _to_reference(self, e: PEntry, flat_slice: torch.Tensor) -> torch.Tensor:
        if e.kind == "sg":
            n2 = e.ref_shape[0]
            return flat_slice.view(n2 // 2, 2, -1).permute(1, 0, 2).reshape(e.ref_shape).contiguous()
        if e.kind == "down":
            o, c = e.ref_shape[0], e.ref_shape[1]
            return flat_slice.view(o, 2, 2, c).permute(0, 3, 1, 2).contiguous()
        if e.kind == "up":
            n2, c = e.ref_shape[0], e.ref_shape[1]
            return flat_slice.view(4, n2 // 4, c).permute(1, 0, 2).reshape(n2, c, 1, 1).contiguous()
        return flat_slice.view(e.ref_shape)

    def _slice(self, buf: torch.Tensor, key: str) -> torch.Tensor:
        e = self.entries[key]
        return buf[e.offset:e.offset + e.numel]

    def p(self, key: str) -> torch.Tensor:
        return self._slice(self.flat.data, key)

    @torch.no_grad()
    def _init_reference_like(self):
        """torch default init of the reference modules (Conv2d kaiming-uniform(a=sqrt(5)) weights and bias
        U(+-1/sqrt(fan_in)); LayerNorm2d ones/zeros; beta = gamma = 0, NAFNet_arch.py:56-57)."""
        for k, e in self.entries.items():
            leaf = k.rsplit(".", 1)[-1]
            if leaf in ("beta", "gamma"):
                v = torch.zeros(e.ref_shape)
            elif ".norm" in k:
                v = torch.ones(e.ref_shape) if leaf == "weight" else torch.zeros(e.ref_shape)
            elif leaf == "weight":
                fan_in = e.ref_shape[1] * e.ref_shape[2] * e.ref_shape[3]
                bound = 1.0 / fan_in ** 0.5
                v = torch.empty(e.ref_shape).uniform_(-bound, bound)
            else:  # bias: fan_in of the owning conv
                wk = k[:-4] + "weight"
                ws = self.entries[wk].ref_shape
                bound = 1.0 / (ws[1] * ws[2] * ws[3]) ** 0.5
                v = torch.empty(e.ref_shape).uniform_(-bound, bound)
            self.flat.data[e.offset:e.offset + e.numel] = self._to_internal(e, v)

    # ------------------------------------------------------------------ state dict in reference form
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        flat = self.flat if keep_vars else self.flat.detach()
        for k in self.ref_order:
            e = self.entries[k]
            destination[prefix + k] = self._to_reference(e, flat[e.offset:e.offset + e.numel])

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        seen = set()
        with torch.no_grad():
            for k in self.ref_order:
                e = self.entries[k]
                full = prefix + k
                if full not in state_dict:
                    missing_keys.append(full)
                    continue
                v = state_dict[full]
                if tuple(v.shape) != e.ref_shape:
                    error_msgs.append(f"size mismatch for {full}: copying {tuple(v.shape)}, expected {e.ref_shape}")
                    continue
                self.flat.data[e.offset:e.offset + e.numel] = self._to_internal(e, v.to(self.flat.device,
                                                                                        torch.float32))
                seen.add(full)
        if strict:
            for k in state_dict:
                if k.startswith(prefix) and k not in seen and k[len(prefix):] not in self.entries:
                    unexpected_keys.append(k)

    # ------------------------------------------------------------------ forward
    def check_image_size_hw(self, h: int, w: int) -> Tuple[int, int]:
        ps = self.padder_size
        return h + (ps - h % ps) % ps, w + (ps - w % ps) % ps

    def forward(self, inp: torch.Tensor) -> torch.Tensor:
        _lib.require_cuda(inp)
        if inp.dim() != 4 or inp.shape[1] != self.img_channel:
            raise ValueError(f"expected [B,{self.img_channel},H,W], got {tuple(inp.shape)}")
        inp = inp.contiguous()
        if torch.is_grad_enabled() and (self.flat.requires_grad or inp.requires_grad):
            return _NAFNetFn.apply(inp, self.flat, self)
        out, _ = self.exec_forward(inp, save=False)
        return out

    # The executor.  Every op appends a record to the tape when save=True.
    def exec_forward(self, x: torch.Tensor, save: bool, flat: Optional[torch.Tensor] = None,
                     precision: Optional[str] = None):
        """The forward.  `precision`: "fp32" / "fp16" / "bf16" to run in (a caller's own pin, NBPTrainer's); None: the
        module's setting, "auto" resolved here, once, from the ambient autocast region.  The returned tape carries it."""
        prec = self.resolved_precision() if precision is None else precision
        with self._pinned(prec):
            return self._forward_pinned(x, save, flat, prec)

    def _forward_pinned(self, x, save, flat, prec):
        P = self.flat.data if flat is None else flat
        B, Ci, H0, W0 = x.shape
        Hp, Wp = self.check_image_size_hw(H0, W0)
        tape = Tape(prec)
        run = _Run(self._prep_weights(P), tape if save else None)
        w = self.width
        feat = torch.empty(B, Hp, Wp, w, device=x.device, dtype=self.adt)
        call("intro_fwd", x, self._slice(P, "intro.weight"), self._slice(P, "intro.bias"), feat, B, Ci, H0, W0, Hp,
             Wp, w, self.dt)
        if save:
            tape.append(("intro", x, (B, Ci, H0, W0, Hp, Wp, w)))
        h, wd = Hp, Wp
        skips = []
        for i, n in enumerate(self.enc_blk_nums):
            c = self.enc_chans[i]
            for j in range(n):
                nxt = f"encoders.{i}.{j + 1}." if j + 1 < n else None
                feat = self._block_fwd(P, f"encoders.{i}.{j}.", feat, B, h, wd, c, run, nxt)
            skips.append(feat)
            feat = self._down_fwd(P, i, feat, B, h, wd, c, run)
            h, wd = h // 2, wd // 2
        for j in range(self.middle_blk_num):
            nxt = f"middle_blks.{j + 1}." if j + 1 < self.middle_blk_num else None
            feat = self._block_fwd(P, f"middle_blks.{j}.", feat, B, h, wd, self.mid_chan, run, nxt)
        for i, n in enumerate(self.dec_blk_nums):
            chan = self.dec_chans[i] * 2
            feat = self._up_fwd(P, i, feat, skips[::-1][i], B, h, wd, chan, run)
            h, wd = h * 2, wd * 2
            c = self.dec_chans[i]
            for j in range(n):
                nxt = f"decoders.{i}.{j + 1}." if j + 1 < n else None
                feat = self._block_fwd(P, f"decoders.{i}.{j}.", feat, B, h, wd, c, run, nxt)
        out = torch.empty(B, Ci, H0, W0, device=x.device)
        call("ending_fwd", feat, self._slice(P, "ending.weight"), self._slice(P, "ending.bias"), x, out, B, Ci, H0,
             W0, Hp, Wp, w, self.dt)
        if save:
            tape.append(("ending", feat, (B, Ci, H0, W0, Hp, Wp, w)))
            tape.append(("weights", run.w))
        return out, tape

    def _plan_block(self, W: Weights, B, h, w, c, pre, next_pre, save) -> BlockPlan:
        """Every path decision of one NAFBlock, forward and backward: the one place where the switches and the
        library's support queries are read for it."""
        dt = self.dt
        M, hw = B * h * w, h * w
        ln_epilogue = dt != 0 and c in (32, 64, 128, 256)
        ln_fwd = self.fuse_ln_fwd and ln_epilogue
        tile = self.tile_level(B, h, w, c)
        c1dw = not tile and self.fuse_c1dw and dt != 0 and query("c1dw_supported", h, w, c, dt) == 1
        chunks = (query("c1dw_tile_rows", h, w, c) if tile else
                  (1 if c1dw else query("dw_fwd_slab_rows", B, h, w, c, dt)))
        # level 0: t4 is dropped when the backward rebuilds it (sg_rc) or there is no backward, and g2 too (the fused FFN
        # half) wherever the backward rebuilds that as well (nbp_dgrad_sg_rc_wg)
        drop_t4 = dt != 0 and c == 32 and (not save or self.sg_rc)
        ffn = drop_t4 and self.fuse_ffn and (not save or self.sg_rc_wg)
        rows_ffn = (self.fuse_ffn_rows and W.frag is not None and not drop_t4
                    and query("ffn_rows_supported", M, c, hw, dt) == 1)
        return BlockPlan(
            tile=tile, c1dw=c1dw, chunks=chunks, ln_epilogue=ln_epilogue, ln_fwd=ln_fwd, drop_t4=drop_t4, ffn=ffn,
            rows_ffn=rows_ffn, local=self._local_window(pre, h, w),
            carry_next=(ln_fwd or rows_ffn) and next_pre is not None,
            sg_rc_wg=drop_t4 and self.sg_rc_wg, ln_wg=dt != 0 and c == 32 and self.ln_wg,
            # nbp_sca_dw_bwd on the stored tape, nbp_sca_c1dw_bwd_tile on the tile path
            sca_fold=(self.sca_fold and dt != 0 and c <= 1024 and B <= 256
                      and (not C1DW_BWD_VARIANT if tile else c % 16 == 0)),
            grouped=dt != 0 and c % 128 == 0 and self.group_wgrad,
            # tiled-GEMM levels (C > 64, per-64-row-tile partials); levels 0 / 1 (skinny GEMM) keep img_chan_dot
            chandot=dt != 0 and c > 64 and hw % 64 == 0, rows_pre=self.ffn_rows_pre)

    def _block_fwd(self, P, pre, x, B, h, w, c, run: _Run, next_pre=None):
        """One NAFBlock forward (NAFNet_arch.py:60-80) along its BlockPlan.  With plan.ln_fwd the LayerNorms run in the
        epilogue of the GEMM producing their input (nbp_gemm_res_ln): norm2 in conv3's, the next block's norm1 (next_pre)
        in conv5's; that block then takes (n1, st1) from run.ln_carry."""
        M = B * h * w
        hw = h * w
        dev = x.device
        E = lambda *s: torch.empty(*s, device=dev, dtype=self.adt)  # noqa: E731
        F = lambda *s: torch.empty(*s, device=dev)  # noqa: E731  (fp32 statistics)
        dt = self.dt
        W = run.w
        plan = self._plan_block(W, B, h, w, c, pre, next_pre, run.tape is not None)
        carry, run.ln_carry = run.ln_carry, None
        have_n1 = carry is not None and carry[0] is x
        n1, st1 = (carry[1], carry[2]) if have_n1 else (E(M, c), F(M, 2))
        # the tile path keeps no t1 / t2 (the backward rebuilds them from n1)
        t1 = None if plan.tile else E(M, 2 * c)
        t2 = None if plan.tile else E(M, 2 * c)
        g, pool = E(M, c), F(B * plan.chunks * c)
        mean, a = F(B, c), F(B, c)
        y, n2, st2 = E(M, c), E(M, c), F(M, 2)
        # t4 channel pairs interleaved (conv4 rows stored so)
        t4, g2 = (None if plan.drop_t4 else E(M, 2 * c)), (None if plan.ffn else E(M, c))
        out = E(M, c)
        nn1, nst1 = (E(M, c), F(M, 2)) if plan.carry_next else (None, None)
        lnw, lnb = ((self._slice(P, next_pre + "norm1.weight"), self._slice(P, next_pre + "norm1.bias"))
                    if plan.carry_next else (None, None))
        if not have_n1:
            call("ln_fwd_nhwc", x, self._slice(P, pre + "norm1.weight"), self._slice(P, pre + "norm1.bias"),
                 n1, st1, M, c, LN_EPS, dt)
        if plan.tile:
            call("c1dw_fwd_tile", n1, self._slice(W.h, pre + "conv1.weight"), self._slice(P, pre + "conv1.bias"),
                 self._slice(P, pre + "conv2.weight"), self._slice(P, pre + "conv2.bias"), None, None, g, pool, B, h, w,
                 c, dt)
        elif plan.c1dw:
            call("c1_dw_sg_pool", n1, self._slice(W.h, pre + "conv1.weight"), self._slice(P, pre + "conv1.bias"),
                 self._slice(P, pre + "conv2.weight"), self._slice(P, pre + "conv2.bias"), t1, t2, g, pool, B, h, w,
                 c, dt)
        else:
            self._mm(W, n1, c, AM_PLAIN, None, 1, pre + "conv1.weight", t1, 2 * c, CM_PLAIN, M, 2 * c,
                     c, bias=self._slice(P, pre + "conv1.bias"))
            call("dw_sg_pool_fwd", t1, self._slice(P, pre + "conv2.weight"), self._slice(P, pre + "conv2.bias"),
                 t2, g, pool, B, h, w, c, dt)
        if plan.local is None:
            call("sca_fwd", pool, plan.chunks, self._slice(P, pre + "sca.1.weight"), self._slice(P, pre + "sca.1.bias"),
                 mean, a, B, hw, c)
            gs, am, asc, arows = g, AM_SCALE, a, hw
        else:
            # TLSC local window (NAFNetLocal): the pool partials above are ignored; g (.) a is formed per pixel and
            # conv3 and the rest of the block run on it with a unit scale
            gs, am, asc, arows = self._local_sca(P, pre, g, B, h, w, c, plan.local, run.tape), AM_PLAIN, None, 1
            if plan.rows_ffn:
                asc = torch.ones(B, c, device=dev)
        if plan.rows_ffn:
            # conv3 -> norm2 -> conv4 -> SimpleGate -> conv5 (-> the next norm1) as ONE row-stationary launch
            call("ffn_rows_fwd", gs, asc, hw, x, self._slice(W.frag, pre + "conv3.weight"),
                 self._slice(P, pre + "conv3.bias"), self._slice(P, pre + "beta"), self._slice(P, pre + "norm2.weight"),
                 self._slice(P, pre + "norm2.bias"), self._slice(W.frag, pre + "conv4.weight"),
                 self._slice(P, pre + "conv4.bias"), self._slice(W.frag, pre + "conv5.weight"),
                 self._slice(P, pre + "conv5.bias"), self._slice(P, pre + "gamma"), lnw, lnb, y, n2, st2, t4, g2, out,
                 nn1, nst1, M, c, LN_EPS, dt)
        elif plan.ln_fwd:
            call("gemm_res_ln", gs, c, am, asc, arows, self._slice(W.h, pre + "conv3.weight"), c, y,
                 M, c, c, self._slice(P, pre + "conv3.bias"), x, self._slice(P, pre + "beta"),
                 self._slice(P, pre + "norm2.weight"), self._slice(P, pre + "norm2.bias"), n2, st2, LN_EPS,
                 dt)
        else:
            self._mm(W, gs, c, am, asc, arows, pre + "conv3.weight", y, c, CM_PLAIN, M, c, c,
                     bias=self._slice(P, pre + "conv3.bias"), R=x, rscale=self._slice(P, pre + "beta"))
            call("ln_fwd_nhwc", y, self._slice(P, pre + "norm2.weight"), self._slice(P, pre + "norm2.bias"),
                 n2, st2, M, c, LN_EPS, dt)
        if plan.rows_ffn:
            pass
        elif plan.ffn:
            call("gemm_ffn", n2, self._slice(W.h, pre + "conv4.weight"), self._slice(P, pre + "conv4.bias"),
                 self._slice(W.h, pre + "conv5.weight"), self._slice(P, pre + "conv5.bias"), y,
                 self._slice(P, pre + "gamma"), lnw, lnb, out, nn1, nst1, M, c, LN_EPS, dt)
        elif dt != 0:  # SimpleGate in the GEMM epilogue
            self._mm(W, n2, c, AM_PLAIN, None, 1, pre + "conv4.weight", t4, 2 * c, CM_SG, M, 2 * c, c,
                     bias=self._slice(P, pre + "conv4.bias"), pre=g2)
        else:
            self._mm(W, n2, c, AM_PLAIN, None, 1, pre + "conv4.weight", t4, 2 * c, CM_PLAIN, M, 2 * c,
                     c, bias=self._slice(P, pre + "conv4.bias"))
            call("sg_fwd", t4, g2, M, c, 1, dt)
        if plan.ffn or plan.rows_ffn:
            pass
        elif plan.carry_next:
            call("gemm_res_ln", g2, c, AM_PLAIN, None, 1, self._slice(W.h, pre + "conv5.weight"), c,
                 out, M, c, c, self._slice(P, pre + "conv5.bias"), y, self._slice(P, pre + "gamma"), lnw, lnb, nn1,
                 nst1, LN_EPS, dt)
        else:
            self._mm(W, g2, c, AM_PLAIN, None, 1, pre + "conv5.weight", out, c, CM_PLAIN, M, c, c,
                     bias=self._slice(P, pre + "conv5.bias"), R=y, rscale=self._slice(P, pre + "gamma"))

        out = out.view(B, h, w, c)
        if plan.carry_next:
            run.ln_carry = (out, nn1, nst1)
        if run.tape is not None:
            run.tape.append(("block", pre, (B, h, w, c), dict(x=x, n1=n1, st1=st1, t1=t1, t2=t2, g=g, mean=mean, a=a,
                                                              y=y, n2=n2, st2=st2, t4=t4, g2=g2), plan))
        return out

    def tile_level(self, B: int, h: int, w: int, c: int) -> bool:
        """Whether a block of this level takes the tile path (nbp_c1dw_fwd_tile / nbp_c1dw_bwd_tile: t1 / t2 rebuilt on
        chip): 16-bit modes, the channel counts in c1dw_tile_channels, and a level small enough for the kernels' 32-bit
        buffer offsets (nbp_c1dw_tile_supported depends on B: e.g. 16 images of 1024^2 at level 0 take the stored
        tape)."""
        dt = self.dt
        return (self.fuse_c1dw_tile and c in self.c1dw_tile_channels and dt != 0
                and query("c1dw_tile_supported", B, h, w, c, dt) == 1)

    def _local_window(self, pre: str, h: int, w: int) -> Optional[Tuple[int, int]]:
        """The TLSC window (k1, k2) of block `pre` on an h x w map, or None where the block pools globally: always in
        the plain NAFNet, and in NAFNetLocal where the block's kernel covers the map (local_arch.py:42-43, 64)."""
        if self._local_kernels is None:
            return None
        k = self._local_kernels[pre]
        if k[0] >= h and k[1] >= w:
            return None
        return min(h, k[0]), min(w, k[1])

    def _local_sca(self, P, pre, g, B, h, w, c, lk, tape):
        """g (.) a with the per-pixel attention map of a local window: nbp_tlsc_pool -> nbp_tlsc_sca_gate."""
        if tape is not None:
            raise RuntimeError(f"NAFNetLocal is inference only: block {pre[:-1]} pools over a local {lk[0]} x {lk[1]} "
                               f"window on its {h} x {w} map and has no backward (run under torch.no_grad())")
        k1, k2 = lk
        dt = self.dt
        if query("tlsc_supported", B, h, w, c, k1, k2, dt) != 1:
            raise _lib.NBPError(f"nbp_tlsc: shape not served (B {B}, {h} x {w} x {c}, window {k1} x {k2}, dtype {dt})")
        V = torch.empty(B, h - k1 + 1, w - k2 + 1, c, device=g.device)
        ws = torch.empty(query("tlsc_workspace_bytes", B, h, w, c, k1, k2), device=g.device, dtype=torch.uint8)
        ga = torch.empty(B * h * w, c, device=g.device, dtype=self.adt)
        call("tlsc_pool", g, V, ws, B, h, w, c, k1, k2, dt)
        call("tlsc_sca_gate", g, V, self._slice(P, pre + "sca.1.weight"), self._slice(P, pre + "sca.1.bias"), ga, ws,
             B, h, w, c, k1, k2, dt)
        return ga

    def _down_fwd(self, P, i, x, B, h, w, c, run: _Run):
        ho, wo = h // 2, w // 2
        M = B * ho * wo
        out = torch.empty(B, ho, wo, 2 * c, device=x.device, dtype=self.adt)
        self._mm(run.w, x, 0, AM_S2D, None, 1, f"downs.{i}.weight", out, 2 * c, CM_PLAIN, M, 2 * c, 4 * c, ho, wo,
                 c, bias=self._slice(P, f"downs.{i}.bias"))
        if run.tape is not None:
            run.tape.append(("down", i, (B, h, w, c), x))
        return out

    def _up_fwd(self, P, i, x, skip, B, h, w, chan, run: _Run):
        M = B * h * w
        out = torch.empty(B, 2 * h, 2 * w, chan // 2, device=x.device, dtype=self.adt)
        self._mm(run.w, x, chan, AM_PLAIN, None, 1, f"ups.{i}.0.weight", out, 0, CM_D2S, M, 2 * chan, chan, h, w,
                 chan // 2, R=skip)
        if run.tape is not None:
            run.tape.append(("up", i, (B, h, w, chan), x))
        return out

    # ------------------------------------------------------------------ backward
    def exec_backward(self, tape, dout: torch.Tensor, dflat: torch.Tensor, need_dx: bool,
                      flat: Optional[torch.Tensor] = None, hook: Optional[Callable[[Stage], None]] = None):
        """Walk the tape in reverse.  Writes every parameter gradient (exactly once) into dflat, calls
        hook(stage) as each stage's gradient slice is complete, returns d(input) or None.  Runs in the precision the
        tape's forward ran in (Tape.precision): the backward of an AMP step is called outside the autocast region
        (image_restoration_model.py:306-310), and autograd's backward thread does not see the forward's region either.
        Every block takes the path its tape record planned (BlockPlan), whatever the switches say by now."""
        P = self.flat.data if flat is None else flat
        prec = getattr(tape, "precision", None)
        with self._pinned(self.resolved_precision() if prec is None else prec):
            run = _Run(next((rec[1] for rec in tape if rec[0] == "weights"), Weights(P)))
            call("grad_reduce_defer")
            try:
                return self._walk_backward(tape, dout, dflat, need_dx, P, hook, run)
            finally:
                if run.grouping:  # an error inside a grouped level: launch what is queued so the library state is reset
                    call("wgrad_group", 0)
                call("grad_reduce_flush", 1)

    def _close_level(self, run: _Run, pending: List[str], hook):
        """Launch the level's queued weight gradients, then complete its stages (flush + DP hooks) in order."""
        run.grouping = False
        call("wgrad_group", 0)
        for name in pending:
            self._stage_done(run, name, hook)

    def _walk_backward(self, tape, dout, dflat, need_dx, P, hook, run: _Run):
        Wt = run.w
        dfeat = None
        dskips: List[torch.Tensor] = []
        dx_img = None
        level: Optional[List[str]] = None  # stages of the current grouped level, completed when it closes
        level_c = 0
        pend = None  # a block's deferred conv1 input gradient + norm1 backward (taken by the preceding block)
        recs = [r for r in reversed(tape) if r[0] != "weights"]
        for idx, rec in enumerate(recs):
            kind = rec[0]
            if pend is not None and kind != "block":  # not expected (deferral looks ahead to a block): resolve it
                dfeat, pend = self._conv1_bwd(P, run, dflat, **pend), None
            grouped = kind == "block" and rec[4].grouped
            if level is not None and not (grouped and rec[2][3] == level_c):
                self._close_level(run, level, hook)
                level = None
            if grouped and level is None:
                call("wgrad_group", 1)
                run.grouping = True
                level, level_c = [], rec[2][3]
            if kind == "ending":
                feat, (B, Ci, H0, W0, Hp, Wp, w) = rec[1], rec[2]
                dfeat = torch.empty(B, Hp, Wp, w, device=dout.device, dtype=self.adt)
                ws = self._ws(run, query("ending_bwd_workspace_floats", B, Ci, H0, W0, w), dout.device)
                call("ending_bwd", dout, feat, self._slice(P, "ending.weight"), dfeat,
                     self._slice(dflat, "ending.weight"), self._slice(dflat, "ending.bias"), ws, B, Ci, H0, W0, Hp,
                     Wp, w, self.dt)
                self._stage_done(run, "ending", hook)
            elif kind == "block":
                pre, geo, S, plan = rec[1], rec[2], rec[3], rec[4]
                # defer into the preceding block of the same (grouped) level when that one takes the row-stationary
                # backward: the norm1 gradients of this block then land before the level closes
                nxt = recs[idx + 1] if idx + 1 < len(recs) else None
                defer = (plan.rows_pre and level is not None and nxt is not None and nxt[0] == "block"
                         and tuple(nxt[2]) == tuple(geo) and nxt[4].rows_ffn)
                dfeat, pend = self._block_bwd(P, Wt, dflat, pre, geo, S, plan, run, dfeat, pend, defer)
                if level is not None:
                    level.append(pre[:-1])
                else:
                    self._stage_done(run, pre[:-1], hook)
            elif kind == "up":
                i, (B, h, w, chan), x = rec[1], rec[2], rec[3]
                dskips.append(dfeat)  # d(skip) = d(up output): the skip add is an identity branch
                M = B * h * w
                dx = torch.empty(B, h, w, chan, device=dout.device, dtype=self.adt)
                self._mm(Wt, dfeat, 0, AM_S2D, None, 1, f"ups.{i}.0.weight", dx, chan, CM_PLAIN, M, chan, 2 * chan,
                         h, w, chan // 2, dgrad=True)
                self._wgrad(run, dfeat, 0, AM_S2D, x, chan, AM_PLAIN, None, 1, M, 2 * chan, chan, h, w, chan // 2, 0,
                            self._slice(dflat, f"ups.{i}.0.weight"), None)
                self._stage_done(run, f"ups.{i}", hook)
                dfeat = dx
            elif kind == "down":
                i, (B, h, w, c), x = rec[1], rec[2], rec[3]
                ho, wo = h // 2, w // 2
                M = B * ho * wo
                dskip = dskips.pop()
                dx = torch.empty(B, h, w, c, device=dout.device, dtype=self.adt)
                # d enc = D2S(dout . Wd) + d skip
                self._mm(Wt, dfeat, 2 * c, AM_PLAIN, None, 1, f"downs.{i}.weight", dx, 0, CM_D2S, M, 4 * c, 2 * c,
                         ho, wo, c, R=dskip, dgrad=True)
                self._wgrad(run, dfeat, 2 * c, AM_PLAIN, x, 0, AM_S2D, None, 1, M, 2 * c, 4 * c, ho, wo, 0, c,
                            self._slice(dflat, f"downs.{i}.weight"), self._slice(dflat, f"downs.{i}.bias"))
                self._stage_done(run, f"downs.{i}", hook)
                dfeat = dx
            elif kind == "intro":
                x, (B, Ci, H0, W0, Hp, Wp, w) = rec[1], rec[2]
                ws = self._ws(run, query("intro_bwd_workspace_floats", B, Ci, Hp, Wp, w), dout.device)
                if need_dx:
                    dx_img = torch.empty(B, Ci, H0, W0, device=dout.device)
                call("intro_bwd", x, dfeat, self._slice(P, "intro.weight"), self._slice(dflat, "intro.weight"),
                     self._slice(dflat, "intro.bias"), dx_img, ws, B, Ci, H0, W0, Hp, Wp, w, self.dt)
                self._stage_done(run, "intro", hook)
        if level is not None:
            self._close_level(run, level, hook)
        if need_dx:
            # global residual x + inp (NAFNet_arch.py:153): d inp += d out
            call("add", dx_img, dout, dx_img, dx_img.numel(), 0)
        return dx_img

    def _stage_done(self, run: _Run, name, hook):
        """With a gradient-ready hook (the bucketed DP all-reduce) the stage's queued gradient reductions run before the
        hook reads its slice.  Without one nobody reads a slice early, and every deferred reduction waits for the
        backward's final flush: 26 latency-bound reduce launches per step become a few full ones."""
        if hook is None:
            return
        call("grad_reduce_flush", 0)
        run.keep.clear()
        hook(self.stages[name])

    def _ws(self, run: _Run, n, dev):
        """fp32 workspace that stays referenced until the next gradient-reduction flush (deferred reductions read
        it after this call returns)."""
        t = torch.empty(n, device=dev)
        run.keep.append(t)
        return t

    def _wgrad(self, run: _Run, G, ldg, gmode, X, ldx, xmode, xscale, rows, M, N, K, gh, gw, csg, csx, dW, db):
        """Weight gradient (its output only feeds the stage's deferred reductions)."""
        n_ws = query("wgrad_workspace_floats", M, N, K)
        ws = self._ws(run, n_ws, G.device)
        if run.grouping:  # the launch is deferred to the level's end: keep the operands
            run.keep.extend(t for t in (G, X, xscale) if t is not None)
        call("wgrad_f32", G, ldg, gmode, X, ldx, xmode, xscale, rows, M, N, K, gh, gw, csg, csx, dW, db, ws,
             n_ws, self.dt)

    def _reduce(self, slab, S, L, out):
        call("reduce_slab", slab, S, L, out)

    def _wgrad_layer_scale(self, run: _Run, P, dflat, pre, conv, scale, G, X, xmode, xscale, rows, M, c, UV=None):
        """The gradients of a layer-scaled conv, out = r + scale (.) conv(X): U = G^T X and V = colsum G (made here
        unless UV holds them), then dW = scale (.) U, db = scale (.) V, dscale = rowsum(W (.) U) + b (.) V
        (nbp_layer_scale_grad, after the reductions).  At C >= 128 the U launch is queued into the level's grouped one."""
        if UV is None:
            UV = self._ws(run, c * c, G.device), self._ws(run, c, G.device)
            self._wgrad(run, G, c, AM_PLAIN, X, c, xmode, xscale, rows, M, c, c, 0, 0, 0, 0, *UV)
        call("layer_scale_grad", *UV, self._slice(P, pre + conv + ".weight"), self._slice(P, pre + conv + ".bias"),
             self._slice(P, pre + scale), self._slice(dflat, pre + conv + ".weight"),
             self._slice(dflat, pre + conv + ".bias"), self._slice(dflat, pre + scale), c, c)

    def _ffn_bwd_launches(self, P, run: _Run, dflat, pre, B, h, w, c, S, plan: BlockPlan, dout):
        """The FFN half's backward as separate launches; returns (dy, dh, SCA channel-dot slab, its chunks per image)."""
        M = B * h * w
        HW = h * w
        dev = dout.device
        E = lambda *s: torch.empty(*s, device=dev, dtype=self.adt)  # noqa: E731
        F = lambda *s: self._ws(run, math.prod(s), dev)  # noqa: E731  (slabs live until the stage's flush)
        dt = self.dt
        Wt = run.w
        # out = y + gamma * conv5(g2): no stored pre-activation, no scaled-gradient pass.  dg2 = (gamma (.) dout) W5:
        # gamma / beta are already in the transposed 16-bit weights; fp32 takes gamma as the A-operand column scale
        dt4 = E(M, 2 * c)
        UV5 = None
        if plan.drop_t4:  # t4 = conv4(n2) rebuilt per tile inside the dgrad (level 0)
            args = (dout, c, self._slice(Wt.ht, pre + "conv5.weight"), c, S["n2"],
                    self._slice(Wt.h, pre + "conv4.weight"), self._slice(P, pre + "conv4.bias"), dt4, M, c, c)
            if plan.sg_rc_wg:  # + U5 / V5 and conv4's dW / db from the same tiles
                UV5 = F(c * c), F(c)
                n_ws = query("dgrad_sg_rc_wg_workspace_floats", M, c)
                call("dgrad_sg_rc_wg", *args, *UV5, self._slice(dflat, pre + "conv4.weight"),
                     self._slice(dflat, pre + "conv4.bias"), F(n_ws), n_ws, dt)
            else:
                call("dgrad_sg_rc", *args, dt)
        elif dt != 0:  # SimpleGate backward in the dgrad epilogue: dg2 never materialises
            self._mm(Wt, dout, c, AM_PLAIN, None, 1, pre + "conv5.weight", dt4, 2 * c, CM_SGBWD, M, c, c,
                     R=S["t4"], dgrad=True)
        else:
            dg2 = E(M, c)
            self._mm(Wt, dout, c, AM_SCALE, self._slice(P, pre + "gamma"), M, pre + "conv5.weight", dg2, c, CM_PLAIN,
                     M, c, c, dgrad=True)
            call("sg_bwd", dg2, S["t4"], dt4, M, c, 1, dt)
        self._wgrad_layer_scale(run, P, dflat, pre, "conv5", "gamma", dout, S["g2"], AM_PLAIN, None, 1, M, c, UV5)
        # conv4 input gradient + norm2 backward + residual
        dy = E(M, c)
        if not plan.sg_rc_wg:
            self._wgrad(run, dt4, 2 * c, AM_PLAIN, S["n2"], c, AM_PLAIN, None, 1, M, 2 * c, c, 0, 0, 0, 0,
                        self._slice(dflat, pre + "conv4.weight"), self._slice(dflat, pre + "conv4.bias"))
        if plan.ln_epilogue:  # LN backward in the dgrad's epilogue (dn never stored)
            self._dgrad_ln(run, dflat, P, pre, "conv4.weight", "norm2", dt4, S["y"].reshape(M, c), S["st2"], dout, dy,
                           M, c)
        else:
            dn2 = E(M, c)
            self._mm(Wt, dt4, 2 * c, AM_PLAIN, None, 1, pre + "conv4.weight", dn2, c, CM_PLAIN, M, c, 2 * c,
                     dgrad=True)
            lg = query("ln_nhwc_grid", M, c, dt)
            sw, sb = F(lg * c), F(lg * c)
            call("ln_bwd_nhwc", dn2, S["y"].reshape(M, c), S["st2"], self._slice(P, pre + "norm2.weight"), dout, dy,
                 sw, sb, M, c, dt)
            self._reduce(sw, lg, c, self._slice(dflat, pre + "norm2.weight"))
            self._reduce(sb, lg, c, self._slice(dflat, pre + "norm2.bias"))
        # y = x + beta * conv3(h), h = g (.) a: same layer-scale identity as conv5 (dh = (beta (.) dy) W3)
        dh = E(M, c)
        if plan.chandot:  # the SCA channel dot sum_p dh (.) g rides in the dgrad epilogue
            chunks = HW // 64
            da_slab = F(B * chunks * c)
            call("gemm_bf16", dy, c, AM_PLAIN, None, HW, dt, self._slice(Wt.ht, pre + "conv3.weight"), c, dh, c,
                 CM_CHANDOT, dt, M, c, c, 0, 0, 0, None, S["g"], None, da_slab)
        elif dt != 0:
            self._mm(Wt, dy, c, AM_PLAIN, None, 1, pre + "conv3.weight", dh, c, CM_PLAIN, M, c, c, dgrad=True)
        else:
            self._mm(Wt, dy, c, AM_SCALE, self._slice(P, pre + "beta"), M, pre + "conv3.weight", dh, c, CM_PLAIN, M,
                     c, c, dgrad=True)
        self._wgrad_layer_scale(run, P, dflat, pre, "conv3", "beta", dy, S["g"], AM_SCALE, S["a"], HW, M, c)
        # SCA
        if not plan.chandot:
            chunks = query("dw_chunks", B, h, w, c, 0)
            da_slab = F(B * chunks * c)
            call("img_chan_dot", dh, S["g"], da_slab, B, h, w, c, dt)
        return dy, dh, da_slab, chunks

    def _ffn_bwd_rows(self, P, run: _Run, dflat, pre, B, h, w, c, S, dout, pend=None):
        """The FFN half's backward in one row-stationary launch (nbp_ffn_rows_bwd: dt4, dy, dh bitwise the launches; the
        norm2 weight / bias and SCA channel-dot partials per 32-row block), then the weight gradients it feeds queued
        as in _ffn_bwd_launches.  With pend (the following block's deferred conv1 input gradient, dout None) the launch
        first makes that block's dx = this block's dout (bitwise _conv1_bwd), its norm1 partials reduced here.  Returns
        (dy, dh, SCA slab, chunks per image, dout)."""
        M = B * h * w
        HW = h * w
        dev = (dout if dout is not None else pend["dt1"]).device
        E = lambda *s: torch.empty(*s, device=dev, dtype=self.adt)  # noqa: E731
        F = lambda *s: self._ws(run, math.prod(s), dev)  # noqa: E731  (slabs live until the stage's flush)
        dt = self.dt
        Wf = run.w.frag_t
        nb = M // 32
        dt4, dy, dh = E(M, 2 * c), E(M, c), E(M, c)
        sw, sb, da_slab = F(nb * c), F(nb * c), F(nb * c)
        pre_args = (None,) * 9
        if pend is not None:
            q = pend["pre"]
            dout = E(M, c)
            sw1, sb1 = F(nb * c), F(nb * c)
            pre_args = (pend["dt1"], self._slice(Wf, q + "conv1.weight"), pend["x"], pend["st1"],
                        self._slice(P, q + "norm1.weight"), pend["dy"], dout, sw1, sb1)
        call("ffn_rows_bwd", None if pend is not None else dout, S["t4"], S["y"].reshape(M, c), S["st2"],
             self._slice(P, pre + "norm2.weight"), S["g"], self._slice(Wf, pre + "conv5.weight"),
             self._slice(Wf, pre + "conv4.weight"), self._slice(Wf, pre + "conv3.weight"), dt4, dy, dh, sw, sb,
             da_slab, *pre_args, M, c, HW, dt)
        if pend is not None:
            self._reduce(sw1, nb, c, self._slice(dflat, q + "norm1.weight"))
            self._reduce(sb1, nb, c, self._slice(dflat, q + "norm1.bias"))
        self._wgrad_layer_scale(run, P, dflat, pre, "conv5", "gamma", dout, S["g2"], AM_PLAIN, None, 1, M, c)
        self._wgrad(run, dt4, 2 * c, AM_PLAIN, S["n2"], c, AM_PLAIN, None, 1, M, 2 * c, c, 0, 0, 0, 0,
                    self._slice(dflat, pre + "conv4.weight"), self._slice(dflat, pre + "conv4.bias"))
        self._reduce(sw, nb, c, self._slice(dflat, pre + "norm2.weight"))
        self._reduce(sb, nb, c, self._slice(dflat, pre + "norm2.bias"))
        self._wgrad_layer_scale(run, P, dflat, pre, "conv3", "beta", dy, S["g"], AM_SCALE, S["a"], HW, M, c)
        return dy, dh, da_slab, HW // 32, dout

    def _block_bwd(self, P, Wt, dflat, pre, geo, S, plan: BlockPlan, run: _Run, dout, pend=None, defer=False):
        """One block's backward along the plan its forward recorded.  dout None: the following block's conv1 input
        gradient is pending (pend) and made by this block's row-stationary launch.  defer: this block's own conv1 input
        gradient + norm1 backward is left pending for the preceding block.  Returns (dx or None, pending or None)."""
        B, h, w, c = geo
        M = B * h * w
        HW = h * w
        dt = self.dt
        # the FFN half's backward: conv5 dgrad + SimpleGate backward, conv4 dgrad + norm2 backward, conv3 dgrad (+ the SCA
        # channel-dot partials) and the weight gradients they feed
        if pend is not None and not plan.rows_ffn:  # not expected (the walker's look-ahead reads the same plan): resolve
            dout, pend = self._conv1_bwd(P, run, dflat, **pend), None
        if plan.rows_ffn:
            dy, dh, da_slab, chunks, dout = self._ffn_bwd_rows(P, run, dflat, pre, B, h, w, c, S,
                                                               None if pend is not None else dout.reshape(M, c), pend)
        else:
            dout = dout.reshape(M, c)
            dy, dh, da_slab, chunks = self._ffn_bwd_launches(P, run, dflat, pre, B, h, w, c, S, plan, dout)
        dev = dout.device
        E = lambda *s: torch.empty(*s, device=dev, dtype=self.adt)  # noqa: E731
        F = lambda *s: self._ws(run, math.prod(s), dev)  # noqa: E731  (slabs live until the stage's flush)
        # ds = da . W_sca and the SCA weight gradients dW = da^T mean, db = colsum(da) in one launch (or inside the
        # depthwise backward below)
        sca_args = (da_slab, chunks, self._slice(P, pre + "sca.1.weight"), S["mean"])
        dsca = (self._slice(dflat, pre + "sca.1.weight"), self._slice(dflat, pre + "sca.1.bias"))
        if not plan.sca_fold:
            ds = F(B, c)
            call("sca_bwd_fused", *sca_args, ds, *dsca, B, c)
        # SimpleGate + depthwise conv2 (fused when the channel slicing allows: dt2 stays in LDS)
        dt1 = E(M, 2 * c)
        if plan.tile:  # t1 / t2 rebuilt from n1 on chip (nbp_c1dw_bwd_tile)
            ws = F(query("c1dw_bwd_workspace_floats", B, h, w, c))
            tail = (S["n1"], self._slice(Wt.h, pre + "conv1.weight"), self._slice(P, pre + "conv1.bias"),
                    self._slice(P, pre + "conv2.weight"), self._slice(P, pre + "conv2.bias"), dt1,
                    self._slice(dflat, pre + "conv2.weight"), self._slice(dflat, pre + "conv2.bias"), ws, B, h, w, c, dt)
            if plan.sca_fold:
                call("sca_c1dw_bwd_tile", dh, S["a"], *sca_args, *dsca, *tail)
            else:
                call("c1dw_bwd_tile", dh, S["a"], ds, *tail)
        else:
            ws = F(query("dw_bwd_workspace_floats", B, h, w, c))
            dw_args = (S["t1"], self._slice(P, pre + "conv2.weight"), dt1, self._slice(dflat, pre + "conv2.weight"),
                       self._slice(dflat, pre + "conv2.bias"), ws, B, h, w, c, dt)
            if plan.sca_fold:
                call("sca_dw_bwd", dh, S["a"], *sca_args, *dsca, S["t2"], *dw_args)
            elif c % (16 if dt != 0 else 8) == 0:
                call("sca_sg_dw_bwd", dh, S["a"], ds, S["t2"], *dw_args)
            else:
                dt2 = E(M, 2 * c)
                call("sca_sg_bwd", dh, S["a"], ds, S["t2"], dt2, M, c, HW, dt)
                call("dw_bwd", dt2, *dw_args)
        # conv1 input gradient + norm1 backward + residual
        if plan.ln_wg:  # + conv1's dW / db from the same tiles (n1 rebuilt from x / stats)
            dx = E(M, c)
            n_ws = query("dgrad_ln_bwd_wg_workspace_floats", M, c)
            call("dgrad_ln_bwd_wg", dt1, 2 * c, self._slice(Wt.ht, pre + "conv1.weight"), 2 * c, M, c, 2 * c,
                 S["x"].reshape(M, c), S["st1"], self._slice(P, pre + "norm1.weight"),
                 self._slice(P, pre + "norm1.bias"), dy, dx, self._slice(dflat, pre + "norm1.weight"),
                 self._slice(dflat, pre + "norm1.bias"), self._slice(dflat, pre + "conv1.weight"),
                 self._slice(dflat, pre + "conv1.bias"), F(n_ws), n_ws, dt)
            return dx.view(B, h, w, c), None
        self._wgrad(run, dt1, 2 * c, AM_PLAIN, S["n1"], c, AM_PLAIN, None, 1, M, 2 * c, c, 0, 0, 0, 0,
                    self._slice(dflat, pre + "conv1.weight"), self._slice(dflat, pre + "conv1.bias"))
        pend = dict(pre=pre, geo=geo, ln_epilogue=plan.ln_epilogue, dt1=dt1, x=S["x"].reshape(M, c), st1=S["st1"], dy=dy)
        if defer:
            return None, pend
        return self._conv1_bwd(P, run, dflat, **pend), None

    def _conv1_bwd(self, P, run: _Run, dflat, pre, geo, ln_epilogue, dt1, x, st1, dy):
        """conv1 input gradient + norm1 backward + the residual dy: a block's dx."""
        B, h, w, c = geo
        M = B * h * w
        dt = self.dt
        dx = torch.empty(M, c, device=dt1.device, dtype=self.adt)
        if ln_epilogue:  # LN backward in the conv1 dgrad's epilogue (dn1 never stored)
            self._dgrad_ln(run, dflat, P, pre, "conv1.weight", "norm1", dt1, x, st1, dy, dx, M, c)
        else:
            dn1 = torch.empty(M, c, device=dt1.device, dtype=self.adt)
            self._mm(run.w, dt1, 2 * c, AM_PLAIN, None, 1, pre + "conv1.weight", dn1, c, CM_PLAIN, M, c, 2 * c,
                     dgrad=True)
            lg = query("ln_nhwc_grid", M, c, dt)
            sw, sb = self._ws(run, lg * c, dt1.device), self._ws(run, lg * c, dt1.device)
            call("ln_bwd_nhwc", dn1, x, st1, self._slice(P, pre + "norm1.weight"), dy, dx, sw, sb, M, c, dt)
            self._reduce(sw, lg, c, self._slice(dflat, pre + "norm1.weight"))
            self._reduce(sb, lg, c, self._slice(dflat, pre + "norm1.bias"))
        return dx.view(B, h, w, c)

    def _dgrad_ln(self, run: _Run, dflat, P, pre, wkey, norm, dt, x, st, dres, out, M, c):
        """dn = dt . W (16-bit transposed weight copy) and the LayerNorm2d backward + residual in one launch
        (nbp_dgrad_ln_bwd); the LN weight / bias gradients are slab-reduced with the stage's deferred reductions."""
        n_ws = query("dgrad_ln_workspace_floats", M, c)
        ws = self._ws(run, n_ws, dt.device)
        call("dgrad_ln_bwd", dt, 2 * c, self._slice(run.w.ht, pre + wkey), 2 * c, M, c, 2 * c, x, st,
             self._slice(P, pre + norm + ".weight"), dres, out, self._slice(dflat, pre + norm + ".weight"),
             self._slice(dflat, pre + norm + ".bias"), ws, n_ws, self.dt)


class _NAFNetFn(torch.autograd.Function):
    """The whole network as one autograd node: forward and backward run the HIP executor."""

    @staticmethod
    def forward(ctx, inp, flat, net: NAFNet):
        out, tape = net.exec_forward(inp, save=True, flat=flat.detach())
        ctx.tape = tape
        ctx.net = net
        ctx.flat = flat.detach()
        ctx.need_dx = ctx.needs_input_grad[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        net: NAFNet = ctx.net
        dflat = torch.zeros_like(ctx.flat)
        dx = net.exec_backward(ctx.tape, dout.contiguous(), dflat, ctx.need_dx, flat=ctx.flat,
                               hook=net.grad_ready_hook)
        ctx.tape = None
        return dx, dflat, None


def tlsc_kernel_sizes(train_size: Sequence[int], levels: int) -> List[Tuple[int, int]]:
    """TLSC kernel size per U-Net level 0 .. levels (the middle), as the reference's conversion fixes them by one
    forward at train_size (NAFNet_arch.py:169-174, local_arch.py:30-36): base = (int(1.5 Ht), int(1.5 Wt)), and a block
    whose map at the padded train size is (ht, wt) gets (ht base[0] // Ht, wt base[1] // Wt)."""
    Ht, Wt = int(train_size[-2]), int(train_size[-1])
    base = (int(Ht * 1.5), int(Wt * 1.5))
    ps = 2 ** levels
    hp, wp = Ht + (ps - Ht % ps) % ps, Wt + (ps - Wt % ps) % ps
    return [((hp >> lv) * base[0] // Ht, (wp >> lv) * base[1] // Wt) for lv in range(levels + 1)]


class NAFNetLocal(NAFNet):
    """NAFNetLocal(*args, train_size=(1, 3, 256, 256), fast_imp=False, **kwargs) (NAFNet_arch.py:164-174): NAFNet with
    the test-time local converter (TLSC, local_arch.py:10-104) for inference on images larger than the training crops.
    Every SCA whose kernel (1.5 x the block's map at train_size) does not cover its map pools over that sliding window
    instead of the whole map (nbp_tlsc_pool / nbp_tlsc_sca_gate); blocks whose kernel covers the map take NAFNet's
    global path unchanged.  Same state_dict keys as NAFNet.  Inference only: a forward that would record a backward
    through a local block raises; an input on which every block is global behaves exactly as NAFNet."""

    def __init__(self, *args, train_size=(1, 3, 256, 256), fast_imp=False, **kwargs):
        if fast_imp:
            raise NotImplementedError("NAFNetLocal: fast_imp=True (the reference's non-equivalent shortcut, "
                                      "local_arch.py:45-59) is not implemented; use the exact path (fast_imp=False)")
        super().__init__(*args, **kwargs)
        self._set_train_size(train_size)

    def _set_train_size(self, train_size):
        self.train_size = tuple(int(v) for v in train_size)
        L = len(self.enc_blk_nums)
        ks = tlsc_kernel_sizes(self.train_size, L)
        kern: Dict[str, Tuple[int, int]] = OrderedDict()
        for i, n in enumerate(self.enc_blk_nums):
            for j in range(n):
                kern[f"encoders.{i}.{j}."] = ks[i]
        for j in range(self.middle_blk_num):
            kern[f"middle_blks.{j}."] = ks[L]
        for i, n in enumerate(self.dec_blk_nums):
            for j in range(n):
                kern[f"decoders.{i}.{j}."] = ks[L - 1 - i]
        self._local_kernels = kern

    @property
    def local_kernels(self) -> Dict[str, Tuple[int, int]]:
        """{block prefix: (k[0], k[1])}, the reference's AvgPool2d.kernel_size of that block's SCA"""
        return dict(self._local_kernels)

    def local_blocks(self, H: int, W: int) -> Dict[str, bool]:
        """{block prefix: whether the block pools locally} for an H x W input (local_arch.py:42)."""
        hp, wp = self.check_image_size_hw(H, W)
        L = len(self.enc_blk_nums)
        out = OrderedDict()
        for pre in self._local_kernels:
            kind, i = pre.split(".")[0], int(pre.split(".")[1])
            lv = i if kind == "encoders" else (L if kind == "middle_blks" else L - 1 - i)
            out[pre] = self._local_window(pre, hp >> lv, wp >> lv) is not None
        return out

    @classmethod
    def from_net(cls, net: NAFNet, train_size=(1, 3, 256, 256)) -> "NAFNetLocal":
        """A local view of `net` for validation inside a training loop: it shares net.flat (the same Parameter, no
        copy, so it follows the trainer's updates) and takes over net's precision setting ("auto" stays "auto": each
        forward of the view resolves it anew, nothing is cached) and fusion switches."""
        view = cls.__new__(cls)
        view.__dict__.update(net.__dict__)  # shallow: _parameters is net's own dict, flat the same Parameter
        view._active = None
        view._set_train_size(train_size)
        return view

    def forward(self, inp: torch.Tensor) -> torch.Tensor:
        if inp.dim() == 4 and torch.is_grad_enabled() and (self.flat.requires_grad or inp.requires_grad):
            loc = [p for p, v in self.local_blocks(inp.shape[2], inp.shape[3]).items() if v]
            if loc:
                raise RuntimeError(f"NAFNetLocal is inference only: {len(loc)} block(s) (first: {loc[0][:-1]}) pool over "
                                   f"a local window for a {inp.shape[2]} x {inp.shape[3]} input and have no backward; "
                                   "run under torch.no_grad()")
        return super().forward(inp)
