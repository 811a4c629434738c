"""Oracles and inputs shared by tests/test_imgout_host.py and tests/test_gpu_imgout.py.

The reference's tensor2img needs cv2 and torchvision, which are not here, so its arithmetic is restated in numpy
(basicsr/utils/img_util.py:73-74,99-100: clamp, (x - min) / (max - min), (img * 255.0).round(), astype(uint8)), and the
PNG filter is restated from the PNG specification (sections 6.3 and 9: filter types 0-4 on bytes modulo 256, the
minimum-sum-of-absolute-differences choice, ties to the lowest type).
"""
import io
import struct
import zlib

import numpy as np


# ------------------------------------------------------------------------------------------------ quantiser oracle
def quantize_ref(x, lo=0.0, hi=1.0, reverse=False):
    """float32 [C,H,W] -> uint8 [H,W,C]: every operation in float32, rounded on its own; rint is half to even.
    NaN is left out of the contract here (the numpy cast is undefined): callers mask it."""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    t = np.minimum(np.maximum(x, lo), hi)
    t = (t - lo) / (hi - lo)
    v = np.rint(t * np.float32(255.0))
    assert v.dtype == np.float32
    v = np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)
    if reverse:
        v = v[::-1]
    return np.ascontiguousarray(v.transpose(1, 2, 0))


def hard_values():
    """float32 values that sit where the rounding can go wrong: the 255 exact ties (2k+1)/510, k/255 and its two
    neighbours, negatives, values above 1, infinities, -0.0 and denormals."""
    k = np.arange(255, dtype=np.float32)
    ties = (2 * k + 1) / np.float32(510)
    grid = np.arange(256, dtype=np.float32) / np.float32(255)
    extra = np.array([-0.0, 0.0, -1.0, -0.25, -1e-30, 1.0, 1.5, 2.0, 3.0, 1e30, np.inf, -np.inf, 1e-45, -1e-45, 1e-39,
                      1.1754942e-38, 0.5, 0.49999997, 0.50000006, 0.99999994, 1.0000001, -0.5, -0.50000006,
                      -0.49999997, 1.9999999], dtype=np.float32)
    return np.concatenate([ties, grid, np.nextafter(grid, np.float32(2)), np.nextafter(grid, np.float32(-2)), extra])


def quant_input(C, H, W, seed):
    """[C,H,W] float32: uniform over [-0.7, 2.2] with the hard values scattered in (all of them when there is room)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.7, 2.2, size=(C, H, W)).astype(np.float32)
    hv = hard_values()
    flat = x.reshape(-1)
    n = min(hv.size, flat.size)
    flat[rng.permutation(flat.size)[:n]] = hv[rng.permutation(hv.size)[:n]]
    return x


# ------------------------------------------------------------------------------------------------ filter oracle
def png_filter_ref(img):
    """uint8 [H,W,C] -> (scanlines uint8 [H, 1 + W*C], the chosen types [H])"""
    img = np.asarray(img, dtype=np.uint8)
    H, W, C = img.shape
    L = W * C
    x = img.reshape(H, L).astype(np.int32)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C] if L > C else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :-C] if L > C else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    filt = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255            # [5][H][L]
    cost = np.minimum(filt, 256 - filt).sum(axis=2)                                    # [5][H]
    types = np.argmin(cost, axis=0)                                                    # first minimum: lowest type
    out = np.empty((H, 1 + L), dtype=np.uint8)
    out[:, 0] = types
    out[:, 1:] = filt[types, np.arange(H)].astype(np.uint8)
    return out, types


def smooth_frame(H, W, seed):
    """the smooth field of scripts/val_time.py:frame on the CPU: a low-resolution random image upsampled bilinearly,
    2 % noise, clamped to [0, 1]; float32 [3,H,W]"""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 3, max(H // 16, 2), max(W // 16, 2), generator=g)
    x = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=False)
    return (x + 0.02 * torch.randn(1, 3, H, W, generator=g)).clamp(0.0, 1.0)[0].contiguous().numpy()


def crafted_image():
    """40 x 64 x 3 uint8 whose rows choose every filter type: the smooth field quantised, with row 5 uniform noise,
    row 6 values below 4, rows 10-11 a constant 77 and row 20 the ramp 3x mod 256"""
    img = quantize_ref(smooth_frame(40, 64, 1))
    rng = np.random.default_rng(1)  # a noise row for which None (type 0) wins
    img[5] = rng.integers(0, 256, size=(64, 3), dtype=np.uint8)
    img[6] = rng.integers(0, 4, size=(64, 3), dtype=np.uint8)
    img[10:12] = 77
    img[20] = ((3 * np.arange(64 * 3)) % 256).astype(np.uint8).reshape(64, 3)
    return img


# ------------------------------------------------------------------------------------------------ PNG files
PNG_SIG = b"\x89PNG\r\n\x1a\n"


def png_chunks(data):
    """[(type, payload)] of a PNG file's chunks; asserts the signature and every chunk's CRC"""
    data = bytes(data)
    assert data[:8] == PNG_SIG
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(typ + body) == crc, typ
        out.append((typ, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def pil_pixels(data):
    """the pixels PIL decodes from the bytes of a PNG file: [H,W,3] or [H,W]"""
    from PIL import Image
    with Image.open(io.BytesIO(bytes(data))) as im:
        assert im.mode in ("RGB", "L"), im.mode
        return np.array(im)
