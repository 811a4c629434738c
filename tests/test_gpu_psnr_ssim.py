"""GPU tests of the image-domain PSNR / SSIM (metrics/psnr_ssim.py, psnr_ssim.hip) against the reference's
calculate_psnr / calculate_ssim, whose outputs tests/golden/make_golden_psnr_ssim.py stored in psnr_ssim.npz for the
frame pairs of tests/psnr_ssim_fixtures.py.

The bounds come from the fixture, not from the device:
  * PSNR on uint8 / exact float32 data: 1e-12 dB (the squared-difference sum is exact in both; only sqrt and log10
    differ);
  * the float64 modes (valid SSIM, Y SSIM): tol_f64 = 16 x the largest difference between the reference and the
    generator's separable float64 evaluation of the same formula, floor 1e-13; PSNR-Y, a float32 value in the
    reference: tol_psnr_y = 4 x that difference for PSNR-Y;
  * the 3-D SSIM, per run: tol3d = 2 (|ref - F| + |F - S|), floor 1e-7, with F the float64 evaluation under the
    reference's float32-rounded 11 x 11 x 11 weights and S the separable float64 one; and the device agrees with S
    itself to 1e-11 relative.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from psnr_ssim_fixtures import MODES, RUNS, mode_kwargs, pair, run_inputs

pytestmark = pytest.mark.gpu

_RUNS = {}


@pytest.fixture(scope="module")
def gold():
    return golden("psnr_ssim.npz")


@pytest.fixture(scope="module")
def ps():
    from lowlight_image_enhancement_amd.metrics import psnr_ssim
    return psnr_ssim


def _bits(t):
    return t.view(torch.int64)


def _call(ps, mode, a, b, cb, order="HWC"):
    is_ssim, kw = mode_kwargs(mode)
    return (ps.calculate_ssim if is_ssim else ps.calculate_psnr)(a, b, cb, input_order=order, **kw)


def _run(ps, run, dev):
    """{mode: 0-d device tensor} of a run from numpy inputs, computed once"""
    if run not in _RUNS:
        a, b, checksum, cb, order = run_inputs(run)
        with torch.cuda.device(dev):
            res = {mode: _call(ps, mode, a, b, cb, order) for mode in MODES}
        for q in res.values():
            assert q.dtype == torch.float64 and q.dim() == 0 and q.is_cuda
        _RUNS[run] = (checksum, res)
    return _RUNS[run]


def _check(got, ref, tol, what):
    if np.isnan(ref):
        assert np.isnan(got), what
    elif np.isinf(ref):
        assert got == ref, what
    else:
        assert abs(got - ref) <= tol, (what, got, ref, abs(got - ref), tol)


# ------------------------------------------------------------------------------------------------ per run
@pytest.mark.parametrize("run", list(RUNS))
def test_against_reference(dev, ps, gold, run):
    checksum, res = _run(ps, run, dev)
    assert checksum == int(gold[f"{run}_checksum"])
    tol = {"psnr": float(gold["tol_psnr"]), "psnr_y": float(gold["tol_psnr_y"]),
           "ssim3d": float(gold[f"{run}_tol3d"]), "ssim_valid": float(gold["tol_f64"]), "ssim_y": float(gold["tol_f64"])}
    for mode in MODES:
        got, ref, s = float(res[mode].cpu()), float(gold[f"{run}_{mode}"]), float(gold[f"{run}_{mode}_S"])
        print(f"{run} {mode}: device {got!r}, reference {ref!r}, |d| {abs(got - ref):.3e} (bound {tol[mode]:.3e}); "
              f"separable float64 {s!r}, |d| {abs(got - s):.3e}")
        _check(got, ref, tol[mode], (run, mode))
        if mode == "ssim3d":
            _check(got, s, 1e-11 * abs(s), (run, mode, "separable float64"))


def test_left_variants(dev, ps, gold):
    a, b, checksum = pair("left23x80")
    assert checksum == int(gold["left23x80_checksum"])
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for mode in MODES:
        is_ssim, kw = mode_kwargs(mode)
        fn = ps.calculate_ssim_left if is_ssim else ps.calculate_psnr_left
        got = fn(a, b, 0, **kw)
        ref = float(gold[f"left23x80_{mode}"])
        tol = {"psnr": float(gold["tol_psnr"]), "psnr_y": float(gold["tol_psnr_y"]),
               "ssim3d": float(gold["left23x80_tol3d"])}.get(mode, float(gold["tol_f64"]))
        print(f"left23x80 {mode}: device {float(got.cpu())!r}, reference {ref!r} (bound {tol:.3e})")
        _check(float(got.cpu()), ref, tol, mode)
        # the same slice as a strided view of the whole 6-channel pair on the device
        is_y = kw.get("test_y_channel", False)
        view = (ps._ssim_view(ta[:, 64:, :3], tb[:, 64:, :3], ps.MODE_Y if is_y else
                              (ps.MODE_3D if kw.get("ssim3d", True) else ps.MODE_VALID))
                if is_ssim else ps._psnr_view(ta[:, 64:, :3], tb[:, 64:, :3], is_y))
        assert torch.equal(_bits(view), _bits(got)), mode


def test_nan_inf_and_exact_one(dev, ps):
    _, res = _run(ps, "n10x12", dev)
    assert torch.isnan(res["ssim_valid"]).item() and not torch.isnan(res["ssim3d"]).item()
    _, res = _run(ps, "same", dev)
    assert float(res["psnr"].cpu()) == float("inf") and float(res["psnr_y"].cpu()) == float("inf")
    for mode in ("ssim3d", "ssim_valid", "ssim_y"):
        assert float(res[mode].cpu()) == 1.0, mode
    # NaN propagates as in numpy: nan <= 1 is false, so max_value is 255, and the result is NaN
    a, b, _ = pair("f48x64")
    a = a.copy()
    a[3, 4, 1] = np.nan
    assert torch.isnan(ps.calculate_psnr(a, b, 0)).item()
    assert torch.isnan(ps.calculate_ssim(a, b, 0)).item()


def test_max_value_follows_the_data(dev, ps):
    """a [0, 1] frame takes max_value 1; one value above 1 anywhere in img1 (here outside the first tile) takes 255"""
    a, b, _ = pair("f48x64")
    p1, s1 = ps.calculate_psnr(a, b, 0), ps.calculate_ssim(a, b, 0, ssim3d=False)
    a2 = a.copy()
    a2[47, 63, 2] = np.float32(1.5)
    b2 = b.copy()
    b2[47, 63, 2] = np.float32(1.5) - (a[47, 63, 2] - b[47, 63, 2])  # the same difference at that pixel
    p255 = ps.calculate_psnr(a2, b2, 0)
    want = float(p1.cpu()) + 20.0 * np.log10(255.0)
    assert abs(float(p255.cpu()) - want) < 1e-5  # the squared difference at one pixel moved by float32 rounding only
    assert float(ps.calculate_ssim(a2, b2, 0, ssim3d=False).cpu()) > float(s1.cpu())  # C1, C2 65025 times larger


# ------------------------------------------------------------------------------------------------ layouts, determinism
def test_numpy_and_device_tensor_inputs_give_the_same_bits(dev, ps):
    _, res = _run(ps, "s96x80", dev)
    a, b, _, _, _ = run_inputs("s96x80")
    ta = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(dev)  # a tensor is CHW
    tb = torch.from_numpy(np.ascontiguousarray(b.transpose(2, 0, 1))).to(dev)
    for mode in MODES:
        assert torch.equal(_bits(_call(ps, mode, ta, tb, 0)), _bits(res[mode])), mode
        assert torch.equal(_bits(_call(ps, mode, ta.unsqueeze(0), tb.unsqueeze(0), 0)), _bits(res[mode])), mode
        assert torch.equal(_bits(_call(ps, mode, ta, tb.cpu(), 0)), _bits(res[mode])), mode  # a host tensor is uploaded


def test_chw_and_float_copies_are_bitwise_hwc(dev, ps):
    _, res = _run(ps, "s96x80", dev)
    _, chw = _run(ps, "s96x80_chw", dev)
    a, b, _, _, _ = run_inputs("s96x80")
    for mode in MODES:
        assert torch.equal(_bits(chw[mode]), _bits(res[mode])), mode
        # uint8 values are exact in float32 and in float64 (which is cast to float32): the same bits
        assert torch.equal(_bits(_call(ps, mode, a.astype(np.float32), b.astype(np.float32), 0)), _bits(res[mode]))
        assert torch.equal(_bits(_call(ps, mode, a.astype(np.float64), b, 0)), _bits(res[mode]))


@pytest.mark.parametrize("cb", [3, 4])
def test_strided_view_gives_the_bits_of_its_copy(dev, ps, cb):
    """a CHW device tensor (permuted inside) cropped by crop_border -- an odd and an even byte offset of the first
    pixel -- against the contiguous copy of the cropped frame, and a window of a larger buffer"""
    _, res = _run(ps, f"s96x80_cb{cb}", dev)
    a, b, _, _, _ = run_inputs("s96x80")
    ta = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(dev)
    tb = torch.from_numpy(np.ascontiguousarray(b.transpose(2, 0, 1))).to(dev)
    ca = np.ascontiguousarray(a[cb:-cb, cb:-cb])
    cbb = np.ascontiguousarray(b[cb:-cb, cb:-cb])
    big = torch.zeros(101, 87, 3, dtype=torch.uint8, device=dev)
    big[2:98, 5:85] = torch.from_numpy(a).to(dev)
    for mode in MODES:
        q = _call(ps, mode, ta, tb, cb)
        assert torch.equal(_bits(q), _bits(res[mode])), mode
        assert torch.equal(_bits(_call(ps, mode, ca, cbb, 0)), _bits(res[mode])), mode
        is_ssim, kw = mode_kwargs(mode)
        view = big[2:98, 5:85].permute(2, 0, 1)  # a CHW view of an HWC window
        assert torch.equal(_bits(_call(ps, mode, view, tb, cb)), _bits(res[mode])), mode


def test_two_runs_are_bitwise_equal(dev, ps):
    _, res = _run(ps, "s96x80", dev)
    a, b, _, cb, order = run_inputs("s96x80")
    for mode in MODES:
        assert torch.equal(_bits(_call(ps, mode, a, b, cb, order)), _bits(res[mode])), mode
    _, res = _run(ps, "st23x37", dev)
    a, b, _, cb, order = run_inputs("st23x37")
    for mode in MODES:
        assert torch.equal(_bits(_call(ps, mode, a, b, cb, order)), _bits(res[mode])), mode


# ------------------------------------------------------------------------------------------------ routes
def _restored(case, dev, scale=1.1, shift=-0.03):
    a, b, _ = pair(case)
    f = lambda x: (torch.from_numpy(x).to(dev).permute(2, 0, 1).float() / 255.0 * scale + shift).unsqueeze(0).contiguous()  # noqa: E731
    return f(a), f(b)


def test_tensor_route_is_the_metric_on_tensor2img_bytes(dev, ps):
    from lowlight_image_enhancement_amd.imgout import tensor2img
    pred, gt = _restored("s96x80", dev)
    assert tuple(pred.shape) == (1, 3, 96, 80)
    ia, ib = tensor2img(pred), tensor2img(gt)  # the same bytes through the host: uint8 HWC, BGR
    assert ia.dtype == np.uint8 and ia.shape == (96, 80, 3)
    for cb in (0, 3):
        for y in (False, True):
            q = ps.psnr_tensor(pred, gt, crop_border=cb, test_y_channel=y)
            assert q.dtype == torch.float64 and q.dim() == 0 and q.is_cuda
            assert torch.equal(_bits(q), _bits(ps.calculate_psnr(ia, ib, cb, test_y_channel=y)))
            for s3 in (True, False):
                q = ps.ssim_tensor(pred, gt, crop_border=cb, test_y_channel=y, ssim3d=s3)
                assert torch.equal(_bits(q), _bits(ps.calculate_ssim(ia, ib, cb, test_y_channel=y, ssim3d=s3)))
    # rgb2bgr matters to the Y channel only through the channel order
    q_rgb = ps.psnr_tensor(pred, gt, test_y_channel=True, rgb2bgr=False)
    assert torch.equal(_bits(q_rgb), _bits(ps.calculate_psnr(ia[..., ::-1].copy(), ib[..., ::-1].copy(), 0,
                                                             test_y_channel=True)))


def test_validator_with_registered_image_metrics(dev, ps):
    from lowlight_image_enhancement_amd import validation
    from lowlight_image_enhancement_amd.validation import Validator
    had = dict(validation._EXTRA)
    try:
        ps.register_image_metrics()
        v = Validator({"metrics": {"psnr": {"type": "calculate_psnr", "crop_border": 2, "test_y_channel": True},
                                   "ssim": {"type": "calculate_ssim", "crop_border": 2, "input_order": "HWC"},
                                   "ssim2d": {"type": "calculate_ssim", "crop_border": 0, "ssim3d": False}}}, device=dev)
        items = [_restored(c, dev) for c in ("s48x64", "s96x80", "n23x37")]  # a three-item loader
        want = {"psnr": 0.0, "ssim": 0.0, "ssim2d": 0.0}
        for pred, gt in items:
            want["psnr"] += float(ps.psnr_tensor(pred, gt, crop_border=2, test_y_channel=True).cpu()) / 3
            want["ssim"] += float(ps.ssim_tensor(pred, gt, crop_border=2).cpu()) / 3
            want["ssim2d"] += float(ps.ssim_tensor(pred, gt, ssim3d=False).cpu()) / 3
        probe = torch.ones(1, device=dev)
        torch.cuda.synchronize()
        raises = False
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                probe.sum().item()
            except RuntimeError:
                raises = True
            for pred, gt in items:  # no update() waits for the device; result() is the one read
                v.update(pred, gt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        r = v.result()
        print(f"sync debug mode raises on a device read: {raises}; result {r}")
        assert list(r) == ["psnr", "ssim", "ssim2d"]
        for k in want:
            assert r[k] == pytest.approx(want[k], rel=1e-12), k
        with pytest.raises(NotImplementedError):
            Validator({"use_image": True, "metrics": {"psnr": {"type": "calculate_psnr"}}}, device=dev)
    finally:
        validation._EXTRA.clear()
        validation._EXTRA.update(had)
