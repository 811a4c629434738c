"""Cases and seeded inputs of the pixel-loss fixture (tests/golden/pixel_losses.npz), shared by its generator
(tests/golden/make_golden_pixel_losses.py) and by tests/test_gpu_pixel_losses.py.  numpy only."""
import itertools
import zlib

import numpy as np

SHAPES = {
    "A": (2, 3, 9, 37),      # CHW = 999: odd image extent, head and tail
    "B": (1, 3, 1, 1),       # smallest input
    "C": (3, 1, 5, 7),       # single channel
    "D": (2, 3, 64, 64),     # fully aligned
    "E": (4, 3, 128, 160),   # many work-groups and the grid stride
}
KINDS = ("l1", "mse", "charbonnier")
REDUCTIONS = ("mean", "sum", "none")
WMODES = ("none", "full", "one")   # no weight, [N,C,H,W], [N,1,H,W]
LOSS_WEIGHT = {"l1": 0.7, "mse": 1.3, "charbonnier": 0.45}
CHARBONNIER_EPS = 1e-12
GRAD_FULL_MAX = 4096  # larger gradients (and maps) are stored at grad_index() only


def elementwise_cases():
    """[(name, shape key, kind, reduction, wmode)]: the full kind x reduction x weight cross on A, B and C, and on the
    two large shapes one case per kind / reduction / weight mode."""
    out = []
    for sk in ("A", "B", "C"):
        for kind, red, wm in itertools.product(KINDS, REDUCTIONS, WMODES):
            out.append((f"{sk}_{kind}_{red}_{wm}", sk, kind, red, wm))
    for sk, kind, red, wm in (("D", "l1", "mean", "none"), ("D", "mse", "mean", "one"), ("D", "charbonnier", "sum", "full"),
                              ("D", "l1", "none", "full"), ("D", "charbonnier", "none", "one"),
                              ("E", "l1", "mean", "none"), ("E", "mse", "sum", "one"), ("E", "charbonnier", "mean", "full"),
                              ("E", "mse", "none", "none")):
        out.append((f"{sk}_{kind}_{red}_{wm}", sk, kind, red, wm))
    return out


PSNR_SHAPES = {"P1": (1, 3, 1, 1), "P1b": (1, 3, 9, 37), "P2": (2, 3, 9, 37), "P3": (3, 3, 9, 37), "P3c": (3, 1, 5, 7),
               "PD": (2, 3, 64, 64), "PE": (4, 3, 128, 160)}
PSNR_LOSS_WEIGHT = 0.5


def psnr_cases():
    """[(name, shape key, toY)]: N in {1, 2, 3}, toY false and true (three-channel shapes)."""
    out = []
    for sk, shape in PSNR_SHAPES.items():
        out.append((f"{sk}_rgb", sk, False))
        if shape[1] == 3:
            out.append((f"{sk}_y", sk, True))
    return out


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def inputs(shape_key, shape):
    """(pred, target) float32 in [0, 1); every 7th element of target equals pred exactly (sign(0), Charbonnier at 0)."""
    rs = np.random.RandomState(_seed("in:" + shape_key))
    pred = rs.rand(*shape).astype(np.float32)
    target = rs.rand(*shape).astype(np.float32)
    tf, pf = target.reshape(-1), pred.reshape(-1)
    tf[::7] = pf[::7]
    return pred, target


def psnr_inputs(shape_key, shape):
    rs = np.random.RandomState(_seed("psnr:" + shape_key))
    return rs.rand(*shape).astype(np.float32), rs.rand(*shape).astype(np.float32)


def weight(shape_key, shape, wmode):
    """float32 weights in [0, 1) with elements 1, 6, 11, ... exactly zero; None for wmode 'none'."""
    if wmode == "none":
        return None
    ws = tuple(shape) if wmode == "full" else (shape[0], 1) + tuple(shape[2:])
    rs = np.random.RandomState(_seed(f"w:{shape_key}:{wmode}"))
    w = rs.rand(*ws).astype(np.float32)
    w.reshape(-1)[1::5] = 0.0
    return w


def upstream_map(name, shape):
    """the upstream gradient of a reduction-'none' case: float32 in [0.5, 1.5)"""
    rs = np.random.RandomState(_seed("up:" + name))
    return (rs.rand(*shape) + 0.5).astype(np.float32)


UPSTREAM_SCALAR = 1.75  # the upstream gradient of a 'mean' / 'sum' case: loss.backward(gradient=1.75)


def grad_index(n):
    """flat positions at which a gradient or map of n elements is stored: all of them up to GRAD_FULL_MAX, else the
    first and last 8 and every 61st"""
    if n <= GRAD_FULL_MAX:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(8), np.arange(0, n, 61), np.arange(n - 8, n)]))


def checksum(*arrays):
    c = 0
    for a in arrays:
        if a is not None:
            c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c
