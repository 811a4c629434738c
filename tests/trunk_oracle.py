"""The VGG / AlexNet loss trunks restated stage by stage in plain torch, for per-element bounds on every stored tensor.

Test infrastructure only; pure torch, imports on the CPU.  A whole 16-bit trunk cannot be held to a float64 run of the
same network: rounding, differing ReLU / max-pool decisions and cancellation compound over 16 layers.  So
nothing is chained here.  Every stage below takes its inputs AS GIVEN -- the tensors the device itself stored -- and
returns the float64 result of that one stage together with S = sum |w| |x|, the same operation on absolute values.
verify() then holds every stored tensor of a run to

    |dev - ref| <= K * 2^-24 * S + ulp_st(ref) / 2 + ulp_st(dev) / 2

K * 2^-24 * S is the standard bound on a length-K fp32 dot product in any summation order (K fp32 roundings, each at
most 2^-24 of the running sum of absolute values); the two half-ulps are the one rounding to the storage type st
(ulp_st: the type's spacing at the value, by torch.nextafter in that type; fp32 for the fp32 trunk and for the two
fp32 outputs of the 16-bit trunks).  Both are derived, not measured.

A run (the device's in tests/test_gpu_trunk_oracle.py, the float32 stand-in standin() on the host) is a Run: per input
the forward records, the head gradients, the traced backward tensors and the image gradient.

Where the device rounds to the storage type (vgg.py, lpips.py, NewBP_model/losses.py, csrc/vgg.hip, conv16.hip,
gemm16_impl.h, gemm.hip):
  * the prepared input: (clamp01(x) - mean) / std in fp32, rounded once (vgg_prep_kernel `(HT)((v0 - m0) / s0)`);
    channels 3..7 are zero; mean and std arrive as C floats;
  * the weights: `wf` and `wt` (AlexStack `w`, `wt`) are the same fp32 weight rounded once each (`.to(tdt)` after the
    permute / flip, which move values and round nothing), so the forward and the input gradient multiply by the same
    rounded weight; biases, `lin` weights and AlexNet's conv0 gradient weights `wd` stay fp32;
  * every conv output: fp32 accumulator + fp32 bias, ReLU, one rounding (gemm16_impl.h epilogue `v[j] = fmaxf(v[j], 0.f)`
    then the store; gemm.hip `p.C[off] = fmaxf(v, 0.f)` for fp32);
  * max pools move stored values: the output is one of the inputs, bit for bit (first maximum in row-major window order);
  * feat_dist_bwd: g = up * scale (one fp32 rounding; scale arrives as a C float), d = a - b (one), g * 2 d (one), the
    last ReLU's mask `a > 0`, one rounding to st; the loss value reduces the fp32 squares in double;
  * lpips_tap_bwd: squared norms by fmaf over the channels, sqrt, + 1e-10f, reciprocals, the channel dot gs, then
    sc * (g * ia - a * k2) rounded once to st; an all-zero feature vector gets zero gradient; the value accumulates the
    fp32 per-pixel distances in double;
  * add_relu_masked: where post > 0 the fp32 sum of two stored values is rounded again; elsewhere d is left untouched;
  * the conv input gradients (`dn`, `dp`): fp32 accumulator, mode 2 selects by the stored post map (`rv[j] > 0.f`), one
    rounding; mode 1 nothing but the rounding;
  * maxpool2_bwd copies (a 2x2 / 2 window has one contributor: exact) and masks by !(post <= 0); maxpool_k_bwd sums the
    up to four contributions of the overlapping 3x3 / 2 windows in fp32 (`acc[q] += (float)g[q]`), masks, rounds once:
    three fp32 additions;
  * `d8` (conv mode 1 with an fp32 output / alex_conv0_dgrad_kernel: fmaf over <= 3 x 3 taps x Cout in fp32) and the
    image gradient (vgg_input_grad_kernel: one fp32 division, the clamp's pass mask) are fp32.

Small values: an element whose reference is nonzero and below st's smallest normal is held to that smallest normal as
an absolute bound only (the MFMA and the conversions may flush there); no stage may have more than 1 % of its nonzero
reference elements in that range, which is why the fp16 runs scale `up` by a power of two, as a GradScaler does.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch
import torch.nn.functional as F

from block_oracle import _rnd, make_q

U = 2.0 ** -24
ST = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SMALL_CAP = 0.01

VGG19_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]
VGG16_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
LPIPS_SHIFT, LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)


class Conv(NamedTuple):
    label: str   # the production trace's name of this conv
    key: str     # state_dict prefix
    cin: int
    cout: int
    k: int
    stride: int
    pad: int


class Pool(NamedTuple):
    k: int
    stride: int


class Arch(NamedTuple):
    name: str
    ops: tuple          # Conv / Pool in forward order
    taps: tuple         # indices (among the convs) of the tapped post-ReLU maps; () for the feature-distance head
    mean: tuple
    std: tuple
    clamp: bool
    shape: tuple        # the test's input shape


def _vgg_ops(cfg, n_modules):
    ops, idx, cin = [], 0, 3
    for v in cfg:
        if idx >= n_modules:
            break
        if v == "M":
            ops.append(Pool(2, 2))
            idx += 1
        else:
            ops.append(Conv(f"features.{idx}", str(idx), cin, v, 3, 1, 1))
            idx, cin = idx + 2, v
    return tuple(ops)


_ALEX = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
         (10, 256, 256, 3, 1, 1))


def _alex_ops():
    ops = []
    for i, (idx, cin, cout, k, st, pad) in enumerate(_ALEX):
        if i in (1, 2):
            ops.append(Pool(3, 2))
        ops.append(Conv(f"conv{i}", str(idx), cin, cout, k, st, pad))
    return tuple(ops)


def _tap_convs(ops, relus):
    convs = [op for op in ops if isinstance(op, Conv)]
    return tuple(i for i, c in enumerate(convs) if int(c.key) + 1 in relus)


ARCHS: Dict[str, Arch] = {
    "perceptual": Arch("perceptual", _vgg_ops(VGG19_CFG, 36), (), IMAGENET_MEAN, IMAGENET_STD, True, (2, 3, 36, 20)),
    "lpips_vgg": Arch("lpips_vgg", _vgg_ops(VGG16_CFG, 30), _tap_convs(_vgg_ops(VGG16_CFG, 30), (3, 8, 15, 22, 29)),
                      LPIPS_SHIFT, LPIPS_SCALE, False, (2, 3, 36, 20)),
    "lpips_alex": Arch("lpips_alex", _alex_ops(), (0, 1, 2, 3, 4), LPIPS_SHIFT, LPIPS_SCALE, False, (2, 3, 67, 51)),
}
# trace entries per input: one per stored gradient (see trace_names)
TRACE_ENTRIES = {"perceptual": 20, "lpips_vgg": 22, "lpips_alex": 12}


def convs_of(arch: Arch) -> List[Conv]:
    return [op for op in arch.ops if isinstance(op, Conv)]


def _pad8(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------- weights and inputs
def make_weights(trunk: str, seed: int = 3):
    """Deterministic synthetic weights with nonzero biases: ({'N.weight', 'N.bias'} fp32, [five lin vectors] or None).
    VGG: kaiming-normal fan-in (it keeps the activations' scale through all 16 layers, so the deep maps of two images
    still differ by much more than a rounding; torchvision's fan-out init shrinks them); AlexNet: torch's default
    U(+-1/sqrt(fan_in)); biases N(0, 0.05) / the default uniform; lin = |N(0, 0.1)| (non-negative, as lpips keeps them)."""
    arch = ARCHS[trunk]
    g = torch.Generator().manual_seed(seed)
    feats = {}
    for c in convs_of(arch):
        if trunk == "lpips_alex":
            bound = 1.0 / (c.cin * c.k * c.k) ** 0.5
            feats[c.key + ".weight"] = (torch.rand(c.cout, c.cin, c.k, c.k, generator=g) * 2 - 1) * bound
            feats[c.key + ".bias"] = (torch.rand(c.cout, generator=g) * 2 - 1) * bound
        else:
            feats[c.key + ".weight"] = torch.randn(c.cout, c.cin, 3, 3, generator=g) * (2.0 / (c.cin * 9)) ** 0.5
            feats[c.key + ".bias"] = torch.randn(c.cout, generator=g) * 0.05
    lins = None
    if arch.taps:
        cs = convs_of(arch)
        lins = [(torch.randn(cs[i].cout, generator=g) * 0.1).abs() for i in arch.taps]
    return feats, lins


def lpips_state_dict(feats, lins):
    """The lpips-style state_dict LPIPS(weights=...) takes."""
    sd = {f"net.slice1.{k}": v for k, v in feats.items()}
    sd.update({f"lin{k}.model.1.weight": w.view(1, -1, 1, 1) for k, w in enumerate(lins)})
    return sd


def make_inputs(trunk: str, seed: int = 5):
    """Two images: rand * 1.1 - 0.05 where the clamp applies (some pixels outside [0, 1]), [-1, 1] for LPIPS."""
    arch = ARCHS[trunk]
    g = torch.Generator().manual_seed(seed)
    x0, x1 = torch.rand(arch.shape, generator=g), torch.rand(arch.shape, generator=g)
    if arch.clamp:
        return x0 * 1.1 - 0.05, x1 * 1.1 - 0.05
    return x0 * 2 - 1, x1 * 2 - 1


def make_up(trunk: str, st_name: str) -> torch.Tensor:
    """The upstream gradient: one value for the scalar feature distance, a non-uniform one per image for LPIPS.  fp16
    runs scale it by a power of two (as a GradScaler would) so that the float64 reference itself keeps at least 99 % of
    every stage's nonzero gradients above fp16's smallest normal (asserted in tests/test_trunk_oracle_host.py)."""
    base = torch.tensor([0.8125]) if trunk == "perceptual" else torch.tensor([0.75, 1.375])
    return base * (FP16_UP_SCALE[trunk] if st_name == "fp16" else 1.0)


FP16_UP_SCALE = {"perceptual": 2.0 ** 18, "lpips_vgg": 2.0 ** 15, "lpips_alex": 2.0 ** 12}


def rounded_weights(arch: Arch, feats, st: Optional[torch.dtype], dtype=torch.float64):
    """[(w [Cout, Cin, k, k] rounded once to st, bias fp32)] per conv, as `dtype`."""
    out = []
    for c in convs_of(arch):
        w = feats[c.key + ".weight"].float()
        out.append((_rnd(w, st, False).to(dtype), feats[c.key + ".bias"].float().to(dtype)))
    return out


# ---------------------------------------------------------------------------------------------- the stages
# NCHW tensors of any float dtype; each returns (result, S) unless noted.
def _c3(vals, like, cfloat=True):
    """Per-channel constants; cfloat: as the C float the kernel receives."""
    return torch.tensor(vals, dtype=torch.float32 if cfloat else torch.float64).to(like.dtype).view(1, 3, 1, 1)


def prep(x, mean, std, clamp, cfloat=True):
    v = x.clamp(0, 1) if clamp else x
    m, s = _c3(mean, x, cfloat), _c3(std, x, cfloat)
    return (v - m) / s, (v.abs() + m.abs()) / s.abs()


def conv_fwd(x, w, b, stride, pad, relu=True):
    y = F.conv2d(x, w, b, stride, pad)
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride, pad)
    return (y.relu() if relu else y), S


def pool_route(x, k, stride):
    """(y, idx): the k x k / stride max pool (floor) and the row-major window position of the FIRST maximum."""
    B, C, H, W = x.shape
    cols = F.unfold(x.reshape(B * C, 1, H, W), k, stride=stride)  # [B C, k k, L]
    top = cols.max(1, keepdim=True).values
    eq = cols == top
    first = eq & (eq.cumsum(1) == 1)
    idx = first.to(torch.uint8).argmax(1)
    Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
    return top.reshape(B, C, Ho, Wo), idx.reshape(B, C, Ho, Wo)


def torch_pool_route(x, k, stride):
    """The same route from torch's own max_pool2d decision (the pinning test)."""
    B, C, H, W = x.shape
    y, flat = F.max_pool2d(x, k, stride, return_indices=True)
    Ho, Wo = y.shape[2:]
    ii, jj = flat // W, flat % W
    oi = torch.arange(Ho).view(1, 1, Ho, 1) * stride
    oj = torch.arange(Wo).view(1, 1, 1, Wo) * stride
    return y, (ii - oi) * k + (jj - oj)


def pool_bwd(dy, idx, k, stride, in_hw, post):
    """Scatter dy along the route (overlapping windows add), times the ReLU mask !(post <= 0) of the pool input."""
    B, C, Ho, Wo = dy.shape
    L = Ho * Wo

    def scatter(v):
        cols = torch.zeros(B * C, k * k, L, dtype=v.dtype)
        cols.scatter_(1, idx.reshape(B * C, 1, L).long(), v.reshape(B * C, 1, L))
        return F.fold(cols, in_hw, k, stride=stride).reshape(B, C, *in_hw)
    m = ~(post <= 0)
    return scatter(dy) * m, scatter(dy.abs()) * m


def conv_bwd(d, w, pad, post=None, flip=False):
    """Input gradient of a stride-1 'same' conv; post: the mode-2 epilogue's mask (stored post-ReLU map > 0)."""
    if flip:  # a planted error: the weights without the tap flip
        w = w.flip(2, 3)
    g, S = F.conv_transpose2d(d, w, padding=pad), F.conv_transpose2d(d.abs(), w.abs(), padding=pad)
    if post is not None:
        m = post > 0
        g, S = g * m, S * m
    return g, S


def conv0_bwd(d, w, stride, pad, in_hw):
    """Input gradient of the first conv (any stride): d8's three image channels."""
    k = w.shape[2]
    op = tuple(in_hw[a] - ((d.shape[2 + a] - 1) * stride - 2 * pad + k) for a in (0, 1))
    return (F.conv_transpose2d(d, w, stride=stride, padding=pad, output_padding=op),
            F.conv_transpose2d(d.abs(), w.abs(), stride=stride, padding=pad, output_padding=op))


def add_relu_masked(d, g, post):
    """(d + g where post > 0 else d, S, mask)"""
    m = post > 0
    return d + g * m, (d.abs() + g.abs()) * m, m


def feat_dist(a, b, mode, scale):
    d = a - b
    return (d * d if mode == 0 else d.abs()).sum() * scale


def feat_dist_bwd(a, b, mode, scale, up, relu_mask=True):
    g = up.to(a.dtype).reshape(()) * torch.tensor(scale, dtype=torch.float32).to(a.dtype)
    d = a - b
    v, av = (2 * d, 2 * (a.abs() + b.abs())) if mode == 0 else (d.sign(), d.sign().abs())
    m = (a > 0) if relu_mask else torch.ones_like(a, dtype=torch.bool)
    return g * v * m, g.abs() * av * m


def lpips_tap(a, b, w):
    """[N] per-image tap distance: normalize over channels (eps 1e-10), squared difference, lin, spatial mean."""
    u = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    v = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((u - v) ** 2 * w.to(a.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_tap_bwd(a, b, w, up):
    """d (sum_n up[n] tap[n]) / d a, and S from the absolute values of the same formula's terms."""
    HW = a.shape[2] * a.shape[3]
    w2 = 2 * w.to(a.dtype).view(1, -1, 1, 1)
    ra = a.pow(2).sum(1, keepdim=True).sqrt()
    live = ra > 0
    ras = torch.where(live, ra, torch.ones_like(ra))
    na = ras + 1e-10
    ia, ib = 1 / na, 1 / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    g, ga = w2 * (a * ia - b * ib), w2 * (a.abs() * ia + b.abs() * ib)
    k2 = (g * a).sum(1, keepdim=True) / (na * na * ras)
    k2a = (ga * a.abs()).sum(1, keepdim=True) / (na * na * ras)
    sc = up.to(a.dtype).view(-1, 1, 1, 1) / HW
    return sc * (g * ia - a * k2) * live, sc.abs() * (ga * ia + a.abs() * k2a) * live


def input_grad(d3, x, std, clamp, cfloat=True):
    ok = ((x >= 0) & (x <= 1)) if clamp else torch.ones_like(x, dtype=torch.bool)
    g = d3 / _c3(std, d3, cfloat) * ok
    return g, g.abs()


# ---------------------------------------------------------------------------------------------- a run
class Run:
    """What a device (or stand-in) stored for one trunk, NCHW on the CPU.  Per input side s in (0, 1):
    fwd[s] = [("prep", x8[:, :3]), ("conv", y) | ("pool", idx, y) ...] in forward order; heads[s] = the head
    gradients ([d_last] or the five tap gradients); trace[s] = [(name, tensor)]; dx[s] = the image gradient."""

    def __init__(self, x, up):
        self.x, self.up = list(x), up
        self.fwd: List[list] = [[], []]
        self.heads: List[list] = [[], []]
        self.trace: List[list] = [[], []]
        self.dx: List[Optional[torch.Tensor]] = [None, None]
        self.value: Optional[torch.Tensor] = None


def head_consts(arch: Arch, run: Run):
    """(mode, scale) of the feature distance: MSE, reduction 'mean'."""
    return 0, 1.0 / run.fwd[0][-1][-1].numel()


def trace_names(arch: Arch) -> List[str]:
    """The names the production walk records, in order."""
    ops = arch.ops
    convs = convs_of(arch)
    pos = [k for k, op in enumerate(ops) if isinstance(op, Conv)]
    names = ["last.tap"] if arch.taps else []
    for ci in range(len(convs) - 1, 0, -1):
        lab = convs[ci].label
        names += [lab + ".dn"] if isinstance(ops[pos[ci] - 1], Conv) else [lab + ".dp", lab + ".pool"]
        if ci - 1 in arch.taps:
            names.append(lab + ".tap")
    return names + ["d8"]


# ---------------------------------------------------------------------------------------------- the bound
def ulp(t: torch.Tensor, st: torch.dtype) -> torch.Tensor:
    q = t.to(st).abs()
    return torch.nextafter(q, torch.full_like(q, float("inf"))).double() - q.double()


class Report:
    """collect: gather every failed check in `failures` (the GPU test prints them all) instead of raising at the first."""

    def __init__(self, collect: bool = False):
        self.ratio: Dict[str, float] = {}   # stage -> worst error / bound
        self.small: Dict[str, float] = {}   # stage -> share of nonzero reference elements below the smallest normal
        self.checked: List[str] = []
        self.collect = collect
        self.failures: List[str] = []

    def worst(self):
        return max(self.ratio.items(), key=lambda kv: kv[1])

    def fail(self, msg: str):
        if not self.collect:
            raise AssertionError(msg)
        self.failures.append(msg)


def check(rep: Report, name: str, dev, ref, S, K: int, st: torch.dtype, exact=None):
    """Every element of dev within the bound of ref (module docstring); exact: a mask of elements that must be equal."""
    assert name not in rep.checked, f"{name}: checked twice"
    dev, ref = dev.double(), ref.double()
    assert dev.shape == ref.shape, f"{name}: shape {tuple(dev.shape)} vs {tuple(ref.shape)}"
    rep.checked.append(name)
    if not torch.isfinite(dev).all():
        rep.ratio[name], rep.small[name] = float("inf"), 0.0
        return rep.fail(f"{name}: non-finite device values")
    tiny = torch.finfo(st).tiny
    bound = K * U * S.double() + 0.5 * ulp(ref, st) + 0.5 * ulp(dev, st)
    nz = ref != 0
    small = nz & (ref.abs() < tiny)
    bound = torch.where(small, torch.full_like(bound, tiny), bound)
    share = small.sum().item() / max(1, nz.sum().item())
    err = (dev - ref).abs()
    r = (err / bound).max().item()
    rep.ratio[name], rep.small[name] = r, share
    if share > SMALL_CAP:
        rep.fail(f"{name}: {share:.2%} of the nonzero reference elements are below {tiny:.3e}")
    if exact is not None and not torch.equal(dev[exact], ref[exact]):
        rep.fail(f"{name}: elements the stage must leave exact differ")
    if not r <= 1.0:
        i = (err / bound).argmax().item()
        rep.fail(f"{name}: error / bound = {r:.3f} (dev {dev.flatten()[i].item():.9e}, ref {ref.flatten()[i].item():.9e}, "
                 f"bound {bound.flatten()[i].item():.3e}, K {K}; {(err > bound).sum().item()} of {err.numel()} elements)")


def check_exact(rep: Report, name: str, dev, ref):
    assert name not in rep.checked, f"{name}: checked twice"
    assert dev.shape == ref.shape, f"{name}: shape {tuple(dev.shape)} vs {tuple(ref.shape)}"
    rep.checked.append(name)
    same = torch.equal(dev.double(), ref.double())
    rep.ratio[name], rep.small[name] = (0.0 if same else float("inf")), 0.0
    if not same:
        rep.fail(f"{name}: not exact ({(dev.double() != ref.double()).sum().item()} of {ref.numel()} elements differ)")


# ---------------------------------------------------------------------------------------------- the verifier
def verify(arch: Arch, feats, lins, run: Run, st_name: str, sides=(0, 1), collect: bool = False) -> Report:
    """Every stored tensor of `run` against its float64 stage computed from the run's own stored inputs."""
    st = ST[st_name]
    f32 = torch.float32
    W = rounded_weights(arch, feats, st)
    convs = convs_of(arch)
    rep = Report(collect)
    mode, scale = head_consts(arch, run)
    up = run.up.double()
    # ---- forward, every layer
    for s in sides:
        recs = run.fwd[s]
        assert len(recs) == 1 + len(arch.ops), f"forward records: {len(recs)} for {len(arch.ops)} layers"
        x = run.x[s].double()
        ref, S = prep(x, arch.mean, arch.std, arch.clamp)
        check(rep, f"in{s}.prep", recs[0][-1], ref, S, 2, st)
        h, ci = recs[0][-1].double(), 0
        for op, rec in zip(arch.ops, recs[1:]):
            if isinstance(op, Conv):
                assert rec[0] == "conv"
                w, b = W[ci]
                ref, S = conv_fwd(h, w, b, op.stride, op.pad)
                check(rep, f"in{s}.fwd.{op.label}", rec[-1], ref, S, op.k * op.k * _pad8(op.cin) + 1, st)
                ci += 1
            else:
                assert rec[0] == "pool"
                y, idx = pool_route(h, op.k, op.stride)
                check_exact(rep, f"in{s}.fwd.pool{ci}.idx", rec[1], idx)
                check_exact(rep, f"in{s}.fwd.pool{ci}", rec[-1], y)
            h = rec[-1].double()
    # ---- heads
    pos = [k for k, op in enumerate(arch.ops) if isinstance(op, Conv)]
    posts = [[run.fwd[s][1 + p][-1].double() for p in pos] for s in (0, 1)]  # post-ReLU map of every conv
    if arch.taps:
        val = sum(lpips_tap(posts[0][t], posts[1][t], lins[k].double()) for k, t in enumerate(arch.taps))
    else:
        val = feat_dist(posts[0][-1], posts[1][-1], mode, scale).reshape(1)
    dv = run.value.double().reshape(-1)
    if not (dv.shape == val.shape and ((dv - val).abs() <= 1e-5 * val.abs()).all()):
        rep.fail(f"value: {dv.tolist()} vs {val.tolist()}, more than 1e-5 relative")
    for s in sides:
        mine, other = posts[s], posts[1 - s]
        if arch.taps:
            assert len(run.heads[s]) == len(arch.taps)
            for k, t in enumerate(arch.taps):
                ref, S = lpips_tap_bwd(mine[t], other[t], lins[k].double(), up)
                check(rep, f"in{s}.head.tap{k}", run.heads[s][k], ref, S, 2 * convs[t].cout + 16, st)
        else:
            ref, S = feat_dist_bwd(mine[-1], other[-1], mode, scale, up)
            check(rep, f"in{s}.head.d_last", run.heads[s][0], ref, S, 3, st)
    # ---- backward, every traced tensor
    names = trace_names(arch)
    for s in sides:
        tr = run.trace[s]
        assert [n for n, _ in tr] == names, f"trace names {[n for n, _ in tr]} != {names}"
        it = iter(tr)
        heads = [h.double() for h in run.heads[s]]
        tapg = dict(zip(arch.taps, heads))

        def nxt(suffix):
            n, t = next(it)
            assert n.endswith(suffix)
            return f"in{s}.bwd.{n}", t

        if arch.taps:
            n, t = nxt("last.tap")
            ref, S, m = add_relu_masked(torch.zeros_like(heads[-1]), heads[-1], posts[s][-1])
            check(rep, n, t, ref, S, 1, st, exact=~m)
            d = t.double()
        else:
            d = heads[0]
        for ci in range(len(convs) - 1, 0, -1):
            op, (w, _) = convs[ci], W[ci]
            K = op.k * op.k * op.cout
            post = posts[s][ci - 1]
            if isinstance(arch.ops[pos[ci] - 1], Conv):
                n, t = nxt(".dn")
                ref, S = conv_bwd(d, w, op.pad, post=post)
                check(rep, n, t, ref, S, K, st, exact=~(post > 0))
            else:
                pool = arch.ops[pos[ci] - 1]
                n, t = nxt(".dp")
                ref, S = conv_bwd(d, w, op.pad)
                check(rep, n, t, ref, S, K, st)
                idx = run.fwd[s][pos[ci]][1]  # the pool's record sits right before this conv's
                n, t2 = nxt(".pool")
                ref, S = pool_bwd(t.double(), idx, pool.k, pool.stride, post.shape[2:], post)
                if pool.k == pool.stride:  # disjoint windows: one contributor, a copy
                    check_exact(rep, n, t2, ref)
                else:  # up to (k / stride rounded up)^2 = 4 contributors summed in fp32: three additions
                    check(rep, n, t2, ref, S, 3, st, exact=(post <= 0))
                t = t2
            if ci - 1 in arch.taps:
                n, t3 = nxt(".tap")
                ref, S, m = add_relu_masked(t.double(), tapg[ci - 1], post)
                check(rep, n, t3, ref, S, 1, st, exact=~m)
                t = t3
            d = t.double()
        n, t = nxt("d8")
        op, (w, _) = convs[0], W[0]
        if arch.name == "lpips_alex":  # the direct transposed conv reads the fp32 weights
            w = feats[op.key + ".weight"].double()
        ref, S = conv0_bwd(d, w, op.stride, op.pad, run.x[s].shape[2:])
        taps_per_axis = -(-op.k // op.stride)
        check(rep, n, t, ref, S, taps_per_axis * taps_per_axis * op.cout, f32)
        assert next(it, None) is None
        ref, S = input_grad(t.double(), run.x[s].double(), arch.std, arch.clamp)
        check(rep, f"in{s}.dx", run.dx[s], ref, S, 1, f32)
    return rep


def expected_checks(arch: Arch, sides=2) -> int:
    """Stage outputs verify() must have checked: prep, every conv, two per pool, the heads, the trace, dx."""
    n_pool = sum(isinstance(op, Pool) for op in arch.ops)
    n_conv = len(arch.ops) - n_pool
    heads = len(arch.taps) if arch.taps else 1
    return sides * (1 + n_conv + 2 * n_pool + heads + len(trace_names(arch)) + 1)


# ---------------------------------------------------------------------------------------------- the stand-in
MUTANTS = ("pool_no_mask", "tap_late", "no_flip", "unrounded_weights", "lin_shift", "fp16_as_bf16")


def standin(arch: Arch, feats, lins, x, up, st_name: Optional[str], cd=torch.float32, mutant: Optional[str] = None,
            torch_routes: bool = False) -> Run:
    """The device's walk with every stage computed in `cd` (float32: a stand-in for the device) and rounded where the
    device rounds; st_name None with cd float64: the composed stages with q the identity (the pinning test).
    mutant: one planted error of the kind a kernel or its launch could make."""
    st = ST[st_name] if st_name else None
    cfloat = st is not None  # the kernels receive mean / std as C floats; the pinning run keeps the oracle's doubles
    if mutant == "fp16_as_bf16":
        st = torch.bfloat16
    q0 = make_q(None if st in (None, torch.float32) else st)

    def q(t):
        return q0(t.to(cd), False) if st is not None else t
    W = rounded_weights(arch, feats, None if mutant == "unrounded_weights" else st, cd)
    convs = convs_of(arch)
    pos = [k for k, op in enumerate(arch.ops) if isinstance(op, Conv)]
    run = Run([t.to(cd) for t in x], up.to(cd))
    route = torch_pool_route if torch_routes else pool_route
    for s in (0, 1):
        h = q(prep(run.x[s], arch.mean, arch.std, arch.clamp, cfloat)[0])
        run.fwd[s].append(("prep", h))
        ci = 0
        for op in arch.ops:
            if isinstance(op, Conv):
                h = q(conv_fwd(h, W[ci][0], W[ci][1], op.stride, op.pad)[0])
                run.fwd[s].append(("conv", h))
                ci += 1
            else:
                h, idx = route(h, op.k, op.stride)
                run.fwd[s].append(("pool", idx, h))
    posts = [[run.fwd[s][1 + p][-1] for p in pos] for s in (0, 1)]
    mode, scale = head_consts(arch, run)
    if arch.taps:
        L = [w.to(cd) for w in lins]
        if mutant == "lin_shift":  # one tap's lin weight off by one channel, in the gradient
            Lb = list(L)
            Lb[2] = L[2].roll(1)
        else:
            Lb = L
        run.value = sum(lpips_tap(posts[0][t], posts[1][t], L[k]).double() for k, t in enumerate(arch.taps))
        for s in (0, 1):
            run.heads[s] = [q(lpips_tap_bwd(posts[s][t], posts[1 - s][t], Lb[k], run.up)[0])
                            for k, t in enumerate(arch.taps)]
    else:
        run.value = feat_dist(posts[0][-1].double(), posts[1][-1].double(), mode, scale)
        for s in (0, 1):
            run.heads[s] = [q(feat_dist_bwd(posts[s][-1], posts[1 - s][-1], mode, scale, run.up)[0])]
    for s in (0, 1):
        tr = run.trace[s]
        tapg = dict(zip(arch.taps, run.heads[s]))
        if arch.taps:
            d = q(add_relu_masked(torch.zeros_like(run.heads[s][-1]), run.heads[s][-1], posts[s][-1])[0])
            tr.append(("last.tap", d))
        else:
            d = run.heads[s][0]
        late = None
        for ci in range(len(convs) - 1, 0, -1):
            op, w = convs[ci], W[ci][0]
            post = posts[s][ci - 1]
            flip = mutant == "no_flip" and ci == 2
            if isinstance(arch.ops[pos[ci] - 1], Conv):
                t = conv_bwd(d, w, op.pad, post=post, flip=flip)[0]
                if late is not None and late.shape == t.shape:  # the tap that was due one conv earlier arrives here
                    t, late = t + late * (post > 0), None
                t = q(t)
                tr.append((op.label + ".dn", t))
            else:
                pool = arch.ops[pos[ci] - 1]
                t = q(conv_bwd(d, w, op.pad, flip=flip)[0])
                tr.append((op.label + ".dp", t))
                idx = run.fwd[s][pos[ci]][1]
                mask_by = torch.ones_like(post) if mutant == "pool_no_mask" else post
                t = q(pool_bwd(t, idx, pool.k, pool.stride, post.shape[2:], mask_by)[0])
                tr.append((op.label + ".pool", t))
            if ci - 1 in arch.taps:
                if mutant == "tap_late" and late is None and isinstance(arch.ops[pos[ci - 1] - 1], Conv) \
                        and convs[ci - 2].cout == convs[ci - 1].cout:
                    late = tapg[ci - 1]
                else:
                    t = q(add_relu_masked(t, tapg[ci - 1], post)[0])
                tr.append((op.label + ".tap", t))
            d = t
        op = convs[0]
        w0 = feats[op.key + ".weight"].to(cd) if arch.name == "lpips_alex" else W[0][0]
        d8 = conv0_bwd(d, w0, op.stride, op.pad, run.x[s].shape[2:])[0]
        tr.append(("d8", d8))
        run.dx[s] = input_grad(d8, run.x[s], arch.std, arch.clamp, cfloat)[0]
    return run
