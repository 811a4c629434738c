"""GPU tests of the image output path: nbp_img_quantize and nbp_png_filter bit for bit against the numpy oracles of
tests/imgout_fixtures.py, their guard bytes, ImageWriter's pipeline and Validator.run(save_dir=...)."""
import os

import numpy as np
import pytest
import torch

from imgout_fixtures import crafted_image, pil_pixels, png_filter_ref, quant_input, quantize_ref

pytestmark = pytest.mark.gpu

QUANT_SHAPES = [(3, 1, 1), (3, 2, 5), (1, 7, 33), (3, 37, 211), (3, 16, 4256)]
GUARD = 64


def _guarded(n, dev):
    """n output bytes between two runs of GUARD bytes of 0xA5"""
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    b = buf.cpu().numpy()
    return bool(np.all(b[:GUARD] == 0xA5) and np.all(b[-GUARD:] == 0xA5))


def _quantize(x, lo, hi, reverse, dev, offset=0):
    """nbp_img_quantize on x [C,H,W] (numpy); offset = element offset of the source inside a larger buffer"""
    from lowlight_image_enhancement_amd._lib import call
    C, H, W = x.shape
    big = torch.zeros(x.size + offset, dtype=torch.float32, device=dev)
    src = big[offset:].view(C, H, W)
    src.copy_(torch.from_numpy(x))
    assert src.data_ptr() % 16 == (4 * offset) % 16
    buf, dst = _guarded(H * W * C, dev)
    call("img_quantize", src, dst, C, H, W, float(lo), float(hi), int(reverse))
    assert _guards_intact(buf)
    return dst.cpu().numpy().reshape(H, W, C)


def _filter(img, dev):
    from lowlight_image_enhancement_amd._lib import call
    H, W, C = img.shape
    buf, dst = _guarded(H * (1 + W * C), dev)
    call("png_filter", torch.from_numpy(img).to(dev), dst, H, W, C)
    assert _guards_intact(buf)
    return dst.cpu().numpy().reshape(H, 1 + W * C)


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("shape", QUANT_SHAPES, ids=str)
def test_quantize_bit_for_bit(dev, shape):
    C, H, W = shape
    x = quant_input(C, H, W, seed=H * 7 + W)
    for lo, hi in ((0.0, 1.0), (-0.5, 2.0)):
        for reverse in (0, 1):
            for offset in (0, 1):  # 16-byte aligned planes, and a source that is only 4-byte aligned
                got = _quantize(x, lo, hi, reverse, dev, offset)
                ref = quantize_ref(x, lo, hi, bool(reverse))
                assert np.array_equal(got, ref), (shape, lo, hi, reverse, offset, int((got != ref).sum()))


def test_quantize_every_tie_and_neighbour(dev):
    """the 255 exact ties (2k+1)/510 (128 of them round down to even), k/255 and its neighbours, the specials: all of
    them in one row, through the 16-byte path, the scalar path and the one-plane tail"""
    from imgout_fixtures import hard_values
    hv = hard_values()
    ties = hv[:255] * np.float32(255)
    assert np.all(ties - np.floor(ties) == 0.5) and int((np.rint(ties) < ties).sum()) == 128
    for C, n in ((3, hv.size // 3 // 4 * 4), (1, hv.size)):  # 1048 values: C = 3 takes 3 x 348, C = 1 all with no tail
        x = hv[-C * n:].reshape(C, 1, n) if C == 3 else hv.reshape(1, 1, n)
        for offset in (0, 1):
            assert np.array_equal(_quantize(x, 0.0, 1.0, 0, dev, offset), quantize_ref(x))
    x = hv[:1047].reshape(1, 1, 1047)  # one plane, N % 4 == 3: 16-byte body and a scalar tail in one launch
    assert np.array_equal(_quantize(x, 0.0, 1.0, 0, dev), quantize_ref(x))
    x = hv[:3 * 349].reshape(3, 1, 349)  # the ties and the grid in the scalar path (N % 4 == 1)
    assert np.array_equal(_quantize(x, 0.0, 1.0, 1, dev), quantize_ref(x, reverse=True))


def test_quantize_nan_stores_zero(dev):
    x = np.full((3, 4, 8), 0.75, dtype=np.float32)
    x[0, 1, 2] = np.nan
    x[2, 3, 7] = -np.nan
    for offset in (0, 1):
        got = _quantize(x, 0.0, 1.0, 0, dev, offset)
        assert got[1, 2, 0] == 0 and got[3, 7, 2] == 0
        got[1, 2, 0] = got[3, 7, 2] = 191
        assert np.all(got == 191)  # rint(0.75 * 255 = 191.25)


def test_quantize_argument_errors(dev):
    from lowlight_image_enhancement_amd._lib import NBPError, call
    src = torch.zeros(3 * 4 * 4, device=dev)
    dst = torch.zeros(3 * 4 * 4, dtype=torch.uint8, device=dev)
    for C, H, W, lo, hi in [(2, 4, 4, 0.0, 1.0), (4, 2, 2, 0.0, 1.0), (3, 0, 4, 0.0, 1.0), (3, 4, 0, 0.0, 1.0),
                            (3, 4, 4, 1.0, 1.0), (3, 4, 4, 1.0, 0.0), (3, 4, 4, 0.0, float("nan"))]:
        with pytest.raises(NBPError, match="nbp_img_quantize"):
            call("img_quantize", src, dst, C, H, W, lo, hi, 0)
    with pytest.raises(NBPError, match="nbp_png_filter"):
        call("png_filter", dst, dst, 4, 4, 2)
    with pytest.raises(NBPError, match="nbp_png_filter"):
        call("png_filter", dst, dst, 0, 4, 3)


def test_tensor2img_on_the_device(dev):
    from lowlight_image_enhancement_amd import tensor2img
    x = quant_input(3, 37, 211, 11)
    t = torch.from_numpy(x).to(dev)
    assert np.array_equal(tensor2img(t), quantize_ref(x, reverse=True))
    assert np.array_equal(tensor2img(t[None], rgb2bgr=False, min_max=(-0.5, 2.0)), quantize_ref(x, -0.5, 2.0))
    assert np.array_equal(tensor2img(t), tensor2img(t.cpu()))
    g = quant_input(1, 7, 33, 12)
    assert np.array_equal(tensor2img(torch.from_numpy(g[0]).to(dev)), quantize_ref(g)[:, :, 0])
    half = t.to(torch.float16)  # any float dtype: converted to float32 first, as the reference's .float()
    assert np.array_equal(tensor2img(half), quantize_ref(half.float().cpu().numpy(), reverse=True))


# ------------------------------------------------------------------------------------------------ filter
def _filter_images():
    rng = np.random.default_rng(7)
    out = {}
    for C, H, W in QUANT_SHAPES:
        out[f"{H}x{W}x{C}"] = quantize_ref(np.clip(quant_input(C, H, W, 5), 0, 1))
    smooth = (np.add.outer(np.arange(3), np.arange(30000)) // 5 % 256)[:, :, None] + np.arange(3) * 30
    out["zeros 3x4x3"] = np.zeros((3, 4, 3), dtype=np.uint8)
    out["noise 9x1000x3"] = rng.integers(0, 256, size=(9, 1000, 3), dtype=np.uint8)
    # rows of 30000 bytes are staged in LDS, rows of 90000 bytes are re-read from global memory (kLdsRowMax = 32000)
    out["lds side 3x10000x3"] = ((smooth[:, :10000] + rng.integers(0, 3, size=(3, 10000, 3))) % 256).astype(np.uint8)
    out["global side 3x30000x3"] = ((smooth + rng.integers(0, 3, size=(3, 30000, 3))) % 256).astype(np.uint8)
    out["threshold 2x32000x1"] = rng.integers(0, 256, size=(2, 32000, 1), dtype=np.uint8)
    out["threshold + 1 2x32001x1"] = rng.integers(0, 256, size=(2, 32001, 1), dtype=np.uint8)
    out["crafted"] = crafted_image()
    return out


FILTER_IMAGES = _filter_images()


def test_crafted_image_uses_every_filter_type():
    """on the numpy reference alone"""
    _, types = png_filter_ref(FILTER_IMAGES["crafted"])
    assert np.bincount(types, minlength=5).tolist() == [1, 6, 17, 13, 3]
    _, types = png_filter_ref(FILTER_IMAGES["zeros 3x4x3"])
    assert types.tolist() == [0, 0, 0]  # every cost is 0: the tie goes to type 0


@pytest.mark.parametrize("name", list(FILTER_IMAGES), ids=lambda s: s.replace(" ", "_"))
def test_filter_bit_for_bit(dev, name):
    img = FILTER_IMAGES[name]
    ref, types = png_filter_ref(img)
    got = _filter(img, dev)
    assert got[:, 0].tolist() == types.tolist(), name
    assert np.array_equal(got, ref), name


# ------------------------------------------------------------------------------------------------ ImageWriter
def test_image_writer_pipeline(dev, tmp_path):
    from lowlight_image_enhancement_amd import ImageWriter
    frames = [quant_input(3, 37, 211, 20 + i) for i in range(4)] + [quant_input(1, 7, 33, 30)]
    with ImageWriter(nthreads=3, level=1, depth=2) as w:  # five frames through two pinned buffers
        for i, x in enumerate(frames):
            w.write(torch.from_numpy(x).to(dev), str(tmp_path / "a" / f"f{i}.png"))
        w.write(torch.from_numpy(frames[0]).to(dev)[None], str(tmp_path / "swapped.png"), rgb2bgr=False,
                min_max=(-0.5, 2.0))
        w.flush()
        assert w.frames == 6
    for i, x in enumerate(frames):
        want = quantize_ref(x)  # rgb2bgr=True and cv2.imwrite: the file holds the tensor's channel order
        got = pil_pixels((tmp_path / "a" / f"f{i}.png").read_bytes())
        assert np.array_equal(got, want if x.shape[0] == 3 else want[:, :, 0]), i
    got = pil_pixels((tmp_path / "swapped.png").read_bytes())
    assert np.array_equal(got, quantize_ref(frames[0], -0.5, 2.0, reverse=True))
    assert not [p for p in os.listdir(tmp_path / "a") if ".tmp" in p]
    with pytest.raises(RuntimeError):
        w.write(torch.zeros(3, 4, 4, device=dev), str(tmp_path / "late.png"))


def test_image_writer_reports_an_unwritable_path_at_close(dev, tmp_path):
    from lowlight_image_enhancement_amd import ImageWriter
    (tmp_path / "file").write_bytes(b"not a directory")
    x = torch.from_numpy(quant_input(3, 8, 8, 1)).to(dev)
    w = ImageWriter(depth=2)
    w.write(x, str(tmp_path / "file" / "x.png"))
    w.write(x, str(tmp_path / "good.png"))  # the ring goes on turning after the failure
    with pytest.raises(OSError):
        w.close()
    assert np.array_equal(pil_pixels((tmp_path / "good.png").read_bytes()), quantize_ref(x.cpu().numpy()))


def test_imwrite_takes_bgr(dev, tmp_path):
    from lowlight_image_enhancement_amd import imwrite, tensor2img
    x = quant_input(3, 37, 211, 40)
    bgr = tensor2img(torch.from_numpy(x).to(dev))
    assert imwrite(bgr, str(tmp_path / "n" / "numpy.png")) is True
    assert imwrite(torch.from_numpy(bgr).to(dev), str(tmp_path / "tensor.png")) is True
    for name in ("n/numpy.png", "tensor.png"):
        assert np.array_equal(pil_pixels((tmp_path / name).read_bytes()), quantize_ref(x))
    gray = quantize_ref(quant_input(1, 7, 33, 41))[:, :, 0]
    imwrite(gray, str(tmp_path / "gray.png"))
    assert np.array_equal(pil_pixels((tmp_path / "gray.png").read_bytes()), gray)


# ------------------------------------------------------------------------------------------------ Validator
def test_validator_saves_under_the_reference_names(dev, tmp_path):
    from lowlight_image_enhancement_amd import Validator

    def net(x):
        return 1.7 * x - 0.2

    g = torch.Generator().manual_seed(3)
    items = []
    for i in range(3):
        path = f"/data/Sony/short/1000{i}_00_0.1s.png"
        items.append({"lq": torch.rand(1, 3, 40, 56, generator=g), "gt": torch.rand(1, 3, 40, 56, generator=g),
                      "lq_path": path if i == 1 else [path]})
    val = Validator({"metrics": {"psnr": {"type": "linear_psnr"}, "ssim": {"type": "linear_ssim"},
                                 "de": {"type": "deltae2000_mean"}}}, device=dev)
    plain = val.run(net, items)
    test_mode = val.run(net, items, save_dir=str(tmp_path / "vis"), dataset_name="SID-test")
    train_mode = val.run(net, items, save_dir=str(tmp_path / "vis"), current_iter=5000, rgb2bgr=False)
    assert list(plain.items()) == list(test_mode.items()) == list(train_mode.items())
    for i, it in enumerate(items):
        name = f"1000{i}_00_0.1s"
        pred = quantize_ref(net(it["lq"])[0].numpy())
        gt = quantize_ref(it["gt"][0].numpy())
        d = tmp_path / "vis" / "SID-test"
        assert np.array_equal(pil_pixels((d / f"{name}.png").read_bytes()), pred)
        assert np.array_equal(pil_pixels((d / f"{name}_gt.png").read_bytes()), gt)
        d = tmp_path / "vis" / name
        assert np.array_equal(pil_pixels((d / f"{name}_5000.png").read_bytes()), pred[:, :, ::-1])
        assert np.array_equal(pil_pixels((d / f"{name}_5000_gt.png").read_bytes()), gt[:, :, ::-1])
    assert sorted(os.listdir(tmp_path / "vis")) == sorted(["SID-test"] + [f"1000{i}_00_0.1s" for i in range(3)])
    with pytest.raises(ValueError, match="lq_path"):
        val.run(net, [{"lq": items[0]["lq"], "gt": items[0]["gt"]}], save_dir=str(tmp_path / "vis"))
