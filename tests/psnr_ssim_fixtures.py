"""Input frames shared by the PSNR / SSIM golden generator (tests/golden/make_golden_psnr_ssim.py) and its tests.

Test infrastructure only.  Every frame pair is built from numpy PCG64 integers and integer arithmetic alone (the one
float32 case divides exact integers by 255 once), so the generator and the tests hold bit-identical inputs on every
platform; each pair comes with an integer checksum that the fixture stores.
"""
from __future__ import annotations

import numpy as np

# case -> (kind, height, width, channels, seed)
CASES = {
    "n7x9": ("noise", 7, 9, 3, 7101),         # smaller than the window radius: every tap clamped, by more than one pixel
    "n10x12": ("noise", 10, 12, 3, 7102),     # the valid map is empty: NaN
    "n11x11": ("noise", 11, 11, 3, 7103),     # the valid map is one pixel
    "n12x13": ("noise", 12, 13, 3, 7104),     # the valid map is 2 x 3
    "n23x37": ("noise", 23, 37, 3, 7105),     # odd sizes inside one tile
    "s48x64": ("smooth", 48, 64, 3, 7106),    # several tiles
    "s96x80": ("smooth", 96, 80, 3, 7107),    # several tiles, partial ones on both edges; cropped and as CHW too
    "flat64": ("flat", 64, 64, 3, 7108),      # 204 +- 2 (0.8 +- 0.008 in bytes): E[x^2] - mu^2 cancels
    "st23x37": ("noise", 23, 37, 6, 7109),    # a stereo pair
    "left23x80": ("noise", 23, 80, 6, 7110),  # for the _left variants: 16 columns right of the first 64
    "f48x64": ("unit", 48, 64, 3, 7106),      # s48x64 as float32 in [0, 1]: max_value 1
    "le1": ("le1", 23, 37, 3, 7111),          # uint8 values 0 and 1 only: max_value 1 from the data
    "same": ("same", 48, 64, 3, 7106),        # s48x64 against itself: PSNR inf, SSIM exactly 1
    "g23x37": ("noise", 23, 37, 1, 7112),     # one channel, passed as a 2-D array
}
TEXTURED = ("n7x9", "n11x11", "n12x13", "n23x37", "s48x64", "s96x80", "st23x37", "f48x64", "le1", "g23x37")
FLAT = ("flat64",)

# run -> (case, crop_border, input_order): what the generator evaluates in every mode
RUNS = {name: (name, 0, "HWC") for name in CASES if name != "left23x80"}
RUNS["s96x80_cb3"] = ("s96x80", 3, "HWC")   # an odd byte offset of the first pixel
RUNS["s96x80_cb4"] = ("s96x80", 4, "HWC")
RUNS["s96x80_chw"] = ("s96x80", 0, "CHW")
MODES = ("psnr", "psnr_y", "ssim3d", "ssim_valid", "ssim_y")


def mode_kwargs(mode):
    """(is_ssim, keyword arguments of calculate_psnr / calculate_ssim) of a mode"""
    return {"psnr": (False, dict(test_y_channel=False)), "psnr_y": (False, dict(test_y_channel=True)),
            "ssim3d": (True, dict(test_y_channel=False, ssim3d=True)),
            "ssim_valid": (True, dict(test_y_channel=False, ssim3d=False)),
            "ssim_y": (True, dict(test_y_channel=True))}[mode]


def _triangle(t, period):
    r = t % period
    return np.minimum(r, period - r)


def _checksum(*arrays):
    total = 0
    for q in arrays:
        q = np.asarray(q, dtype=np.int64).ravel()
        total += int((q * (np.arange(q.size, dtype=np.int64) % 251 + 1)).sum())
    return total


def _base(kind, h, w, c, rng):
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, c), dtype=np.int64)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
        # a dark frame: the float32 conv3d of the reference loses E[x^2] - mu^2 to cancellation on a bright one
        base = 24 + (_triangle(xx, 36) * 64) // 18 // 2 + (_triangle(yy + xx // 2, 50) * 48) // 25 // 2
        return np.clip(base[..., None] + rng.integers(-24, 25, size=(h, w, c), dtype=np.int64), 0, 255)
    if kind == "flat":
        return 204 + rng.integers(-2, 3, size=(h, w, c), dtype=np.int64)
    if kind == "le1":
        return rng.integers(0, 2, size=(h, w, c), dtype=np.int64)
    raise KeyError(kind)


def pair(case):
    """(img1, img2, checksum) of a case in HWC (2-D for one channel): uint8, or float32 in [0, 1] for kind 'unit'"""
    kind, h, w, c, seed = CASES[case]
    rng = np.random.default_rng(seed)
    gen = {"unit": "smooth", "same": "smooth"}.get(kind, kind)
    q1 = _base(gen, h, w, c, rng)
    if kind == "same":
        q2 = q1.copy()
    elif gen == "flat":
        q2 = 204 + rng.integers(-2, 3, size=q1.shape, dtype=np.int64)
    elif gen == "le1":
        q2 = rng.integers(0, 2, size=q1.shape, dtype=np.int64)
    else:  # the second image: the first with a smaller disturbance on top
        q2 = np.clip(q1 + rng.integers(-9, 10, size=q1.shape, dtype=np.int64), 0, 255)
    checksum = _checksum(q1, q2)
    if kind == "unit":
        f = np.float32(255.0)
        return q1.astype(np.float32) / f, q2.astype(np.float32) / f, checksum
    a, b = q1.astype(np.uint8), q2.astype(np.uint8)
    if c == 1:
        a, b = a[..., 0], b[..., 0]
    return np.ascontiguousarray(a), np.ascontiguousarray(b), checksum


def run_inputs(run):
    """(img1, img2, checksum, crop_border, input_order) of a run, in the run's layout"""
    case, cb, order = RUNS[run]
    a, b, checksum = pair(case)
    if order == "CHW":
        a, b = np.ascontiguousarray(a.transpose(2, 0, 1)), np.ascontiguousarray(b.transpose(2, 0, 1))
    return a, b, checksum, cb, order
