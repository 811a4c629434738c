"""Input frames shared by the NIQE golden generator (tests/golden/make_golden_niqe.py) and the NIQE tests.

Test infrastructure only.  Every frame is built from numpy PCG64 integers and integer arithmetic alone, so the
generator (which runs the reference on the build machine) and the tests (which regenerate the frame from its seed)
hold bit-identical inputs on every platform; each frame comes with an integer checksum that the fixture stores.
"""
from __future__ import annotations

import numpy as np

# case -> (kind, height, width, seed, crop_border, input_order)
CASES = {
    "A": ("tex", 192, 192, 9101, 0, "HWC"),      # 2 x 2 blocks: the minimum for a covariance
    "B": ("tex", 200, 301, 9102, 0, "HWC"),      # 2 x 3: the floor crop, an odd width, the idx_w-outer row order
    "C": ("tex", 296, 392, 9103, 4, "HWC"),      # 3 x 4: the border offset
    "D": ("flat", 200, 301, 9104, 0, "HWC"),     # as B with a constant 110 x 110 corner: exact zeros, NaN features
    "E": ("dark", 192, 288, 9105, 0, "HWC"),     # values 0 .. 12, about half of them clipped to 0
    "F": ("tex", 480, 672, 9107, 0, "HWC"),      # 5 x 7 blocks: 700 fits
    "G_chw": ("tex", 192, 192, 9101, 0, "CHW"),  # A transposed
    "G_hw": ("tex", 192, 192, 9101, 0, "HW"),    # A's green plane
    "G_f32": ("texf", 200, 301, 9102, 0, "HWC"),  # B as float32 with non-integer values (multiples of 1/64)
}
GOLDEN_CASES = ("A", "B", "C", "D", "E", "F", "G_hw", "G_f32")  # G_chw is held to A's own numbers


def _triangle(t, period):
    """integer triangle wave of the given even period over integer t: 0 .. period // 2 .. 0"""
    r = t % period
    return np.minimum(r, period - r)


def _tex(h, w, rng):
    """an integer sinusoid-like pattern (two triangle waves) plus integer noise, uint8 [h, w, 3]"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    base = 64 + (_triangle(xx, 44) * 128) // 22 // 2 + (_triangle(yy + xx // 3, 70) * 102) // 35 // 2
    noise = rng.integers(-38, 39, size=(h, w, 3), dtype=np.int64)
    return np.clip(base[..., None] + noise, 0, 255)


def _checksum(q):
    q = np.asarray(q, dtype=np.int64).ravel()
    return int((q * (np.arange(q.size, dtype=np.int64) % 251 + 1)).sum())


def frame(case):
    """(image, checksum, crop_border, input_order) of a case: uint8 (float32 for G_f32) in the case's layout"""
    kind, h, w, seed, crop_border, order = CASES[case]
    rng = np.random.default_rng(seed)
    if kind in ("tex", "flat", "texf"):
        q = _tex(h, w, rng)
        if kind == "flat":
            q[:110, :110] = 77
    elif kind == "dark":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
        q = np.clip(rng.integers(-12, 13, size=(h, w, 3), dtype=np.int64) + _triangle(xx + yy, 64)[..., None] // 16 - 1,
                    0, 12)
    else:
        raise KeyError(kind)
    if kind == "texf":
        q64 = np.minimum(q * 64 + rng.integers(0, 64, size=q.shape, dtype=np.int64), 255 * 64)
        img = (q64.astype(np.float32) / np.float32(64.0)).astype(np.float32)  # exact: at most 14 significant bits
        return img, _checksum(q64), crop_border, order
    img = q.astype(np.uint8)
    if order == "CHW":
        img = np.ascontiguousarray(img.transpose(2, 0, 1))
    elif order == "HW":
        img = np.ascontiguousarray(img[..., 1])
    return img, _checksum(img), crop_border, order
