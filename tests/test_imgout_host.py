"""CPU tests of the image output path: the host PNG encoder (csrc/png_write.cpp), tensor2img on CPU tensors and the
file naming of Validator.run(save_dir=...).  No kernel launches; the scanlines come from the numpy filter oracle."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from imgout_fixtures import (crafted_image, png_chunks, png_filter_ref, pil_pixels, quant_input, quantize_ref)

SHAPES = [(1, 1, 3), (2, 5, 3), (7, 33, 1), "crafted", (300, 1500, 3)]


def _image(shape):
    if shape == "crafted":
        return crafted_image()
    H, W, C = shape
    rng = np.random.default_rng(H * 1000 + W)
    if H >= 100:  # smooth enough to compress, noisy enough that the rows differ
        base = (np.add.outer(np.arange(H), np.arange(W)) // 3 % 256)[:, :, None] + np.arange(C) * 40
        return ((base + rng.integers(0, 6, size=(H, W, C))) % 256).astype(np.uint8)
    return rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)


def _encode(scan, H, W, C, level=1, nthreads=8):
    from lowlight_image_enhancement_amd.imgout import png_encode
    return png_encode(scan, H, W, C, level, nthreads).tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_encoder_round_trip(shape):
    from lowlight_image_enhancement_amd import _lib
    img = _image(shape)
    H, W, C = img.shape
    scan, _ = png_filter_ref(img)
    png = _encode(scan, H, W, C)
    chunks = png_chunks(png)  # signature and every CRC
    assert [t for t, _ in chunks] == [b"IHDR"] + [b"IDAT"] * (len(chunks) - 2) + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)
    assert chunks[-1][1] == b""
    if shape == (300, 1500, 3):
        assert len(chunks) - 2 >= 2  # 1.35 MB of scanlines: more than one stripe
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))  # checks the combined Adler-32 too
    assert raw == scan.tobytes()
    want = img if C == 3 else img[:, :, 0]
    assert np.array_equal(pil_pixels(png), want)
    if C == 3:  # the project's own decoder: 8-bit samples promoted by * 257
        out = np.empty((H, W, 3), dtype=np.uint16)
        buf = np.frombuffer(png, dtype=np.uint8)
        _lib.host_call("png_decode_rgb16", buf.ctypes.data, buf.size, out.ctypes.data, 0, 0, 0, 0)
        assert np.array_equal(out, img.astype(np.uint16) * 257)


def test_encoder_bytes_do_not_depend_on_the_thread_count():
    img = _image((300, 1500, 3))
    H, W, C = img.shape
    scan, _ = png_filter_ref(img)
    for level in (0, 1, 6, 9):
        files = [_encode(scan, H, W, C, level, nt) for nt in (1, 3, 8)]
        assert files[0] == files[1] == files[2], level
        assert np.array_equal(pil_pixels(files[0]), img), level
    assert len(_encode(scan, H, W, C, 9, 1)) < len(_encode(scan, H, W, C, 1, 1)) < len(_encode(scan, H, W, C, 0, 1))


def test_encoder_errors():
    from lowlight_image_enhancement_amd import _lib
    from lowlight_image_enhancement_amd._lib import NBPError
    from lowlight_image_enhancement_amd.imgout import png_encode
    L = _lib.lib().dll
    img = _image((7, 33, 1))
    H, W, C = img.shape
    scan, _ = png_filter_ref(img)
    good = png_encode(scan, H, W, C, 1, 2)
    n = good.size

    def raw(scanlines, h, w, c, level, nthreads, cap):
        out = np.full(cap + 64, 0xA5, dtype=np.uint8)
        got = ctypes.c_long(-7)
        rc = L.nbp_png_encode(scanlines.ctypes.data, h, w, c, level, nthreads, out.ctypes.data, cap, ctypes.byref(got))
        assert np.all(out[cap:] == 0xA5), "wrote past cap"
        return rc, got.value, out[:cap], L.nbp_last_error_string()

    rc, got, out, _ = raw(scan, H, W, C, 1, 2, n)  # an exact cap is enough
    assert rc == 0 and got == n and np.array_equal(out, good)
    rc, got, out, msg = raw(scan, H, W, C, 1, 2, n - 1)  # one byte short
    assert rc == -1 and got == 0 and b"cap" in msg
    assert L.nbp_png_encode_bound(H, W, C) >= n
    bad = scan.copy()
    bad[3, 0] = 5
    rc, _, _, msg = raw(bad, H, W, C, 1, 2, n)
    assert rc == -1 and b"filter type 5" in msg
    with pytest.raises(NBPError, match="filter type 5"):
        png_encode(bad, H, W, C)
    for h, w, c, level, nthreads in [(H, W, 2, 1, 2), (0, W, C, 1, 2), (H, 0, C, 1, 2), (H, W, C, 10, 2),
                                     (H, W, C, -1, 2), (H, W, C, 1, 0)]:
        rc, _, out, msg = raw(scan, h, w, c, level, nthreads, n)
        assert rc == -1 and b"nbp_png_encode" in msg, (h, w, c, level, nthreads)
        assert np.all(out == 0xA5)
    assert L.nbp_png_encode_bound(H, W, 2) < 0 and L.nbp_png_encode_bound(0, W, C) < 0
    with pytest.raises(ValueError):
        png_encode(scan[:-1], H, W, C)


def test_tensor2img_cpu_matches_the_oracle():
    from lowlight_image_enhancement_amd import tensor2img
    x = quant_input(3, 37, 211, 3)
    x[0, 0, :3] = np.nan
    for min_max in ((0, 1), (-0.5, 2.0)):
        bgr = tensor2img(torch.from_numpy(x), min_max=min_max)
        assert bgr.dtype == np.uint8 and bgr.shape == (37, 211, 3)
        assert np.array_equal(bgr, quantize_ref(x, *min_max, reverse=True))
        rgb = tensor2img(torch.from_numpy(x)[None], rgb2bgr=False, min_max=min_max)
        assert np.array_equal(rgb, quantize_ref(x, *min_max))
    assert np.all(bgr[0, :3, 2] == 0)  # NaN -> 0
    gray = quant_input(1, 7, 33, 4)
    ref = quantize_ref(gray)[:, :, 0]
    assert np.array_equal(tensor2img(torch.from_numpy(gray)), ref)          # [1,H,W] -> HW
    assert np.array_equal(tensor2img(torch.from_numpy(gray[0])), ref)       # [H,W]
    both = tensor2img([torch.from_numpy(x), torch.from_numpy(gray)])
    assert isinstance(both, list) and both[0].shape == (37, 211, 3) and both[1].shape == (7, 33)
    one = tensor2img([torch.from_numpy(gray)])  # the reference returns the only image of a list of one
    assert isinstance(one, np.ndarray)
    with pytest.raises(NotImplementedError):
        tensor2img(torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        tensor2img(torch.zeros(3, 4, 4), out_type=np.float32)
    with pytest.raises(TypeError):
        tensor2img(np.zeros((3, 4, 4)))
    with pytest.raises(TypeError):
        tensor2img(torch.zeros(4))
    with pytest.raises(ValueError):
        tensor2img(torch.zeros(3, 4, 4), min_max=(1, 1))


def test_exports_and_alias():
    import sys

    import lowlight_image_enhancement_amd as pkg
    from lowlight_image_enhancement_amd import imgout
    for name in ("tensor2img", "imwrite", "ImageWriter"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(imgout, name)
    before = set(sys.modules)
    try:
        pkg.install_aliases()
        assert sys.modules["basicsr.utils.img_util"].tensor2img is imgout.tensor2img
    finally:  # the aliases are process-wide: leave the other tests' imports as they were
        for name in ("NewBP_model", "metrics", "basicsr"):
            for key in [k for k in sys.modules if k not in before and (k == name or k.startswith(name + "."))]:
                del sys.modules[key]
    for kw in (dict(nthreads=0), dict(level=10), dict(depth=0)):
        with pytest.raises(ValueError):
            imgout.ImageWriter(**kw)


def test_save_paths_follow_the_reference():
    from lowlight_image_enhancement_amd.validation import Validator, image_name, save_paths
    assert image_name({"lq_path": "/data/Sony/short/00001_00_0.1s.png"}) == "00001_00_0.1s"
    assert image_name({"lq_path": ["/data/Sony/short/10003_00_0.04s.png"]}) == "10003_00_0.04s"
    assert image_name({"lq_path": "frame"}) == "frame"
    for bad in ({}, {"lq_path": None}, {"lq_path": ["a.png", "b.png"]}, {"lq_path": 3}):
        with pytest.raises(ValueError):
            image_name(bad)
    j = os.path.join
    assert save_paths("vis", "n1") == (j("vis", "val", "n1.png"), j("vis", "val", "n1_gt.png"))
    assert save_paths("vis", "n1", "SID-test") == (j("vis", "SID-test", "n1.png"), j("vis", "SID-test", "n1_gt.png"))
    assert save_paths("vis", "n1", "SID-test", 5000) == (j("vis", "n1", "n1_5000.png"), j("vis", "n1", "n1_5000_gt.png"))
    with pytest.raises(NotImplementedError, match="save_dir"):
        Validator({"save_img": True}, device="cpu")
