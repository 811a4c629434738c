"""CPU tests of the image-domain PSNR / SSIM (metrics/psnr_ssim.py, psnr_ssim.hip): argument handling and the
reference's exceptions, the opt-in registration, the alias, the C-ABI declarations, and the fixture's
self-consistency (a numpy re-evaluation of PSNR, the valid SSIM and the Y SSIM by the separable float64 formula
against the reference outputs tests/golden/make_golden_psnr_ssim.py stored, within the bounds it stored).
No kernel launches, no reference."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from conftest import golden
from psnr_ssim_fixtures import CASES, FLAT, MODES, RUNS, TEXTURED, pair, run_inputs


@pytest.fixture(scope="module")
def gold():
    return golden("psnr_ssim.npz")


@pytest.fixture()
def ps():
    from lowlight_image_enhancement_amd.metrics import psnr_ssim
    return psnr_ssim


# ------------------------------------------------------------------------------------------------ arguments
def test_exceptions_match_the_reference(ps):
    a = np.zeros((12, 13, 3), np.uint8)
    for fn in (ps.calculate_psnr, ps.calculate_ssim):
        with pytest.raises(AssertionError, match="Image shapes are differnet"):
            fn(a, np.zeros((12, 14, 3), np.uint8), 0)
        with pytest.raises(ValueError, match="Wrong input_order"):
            fn(a, a, 0, input_order="WHC")
        with pytest.raises(ValueError, match="transposes it twice"):
            fn(torch.zeros(3, 12, 13), torch.zeros(3, 12, 13), 0, input_order="CHW")
        with pytest.raises(ValueError):
            fn(np.zeros((12, 13, 4), np.uint8), np.zeros((12, 13, 4), np.uint8), 0)
        with pytest.raises(ValueError):
            fn(a, a, 6)  # nothing is left after the crop
        with pytest.raises(ValueError):
            fn(a, a, -1)
    for fn in (ps.calculate_psnr_left, ps.calculate_ssim_left):
        with pytest.raises(AssertionError):
            fn(a, a, 0, input_order="CHW")
        with pytest.raises(AssertionError):
            fn(a, a, 2)
    with pytest.raises(NotImplementedError):
        ps.calculate_skimage_ssim(a, a)
    with pytest.raises(NotImplementedError):
        ps.calculate_skimage_ssim_left(a, a)


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a machine without a GPU")
def test_no_gpu_is_an_error_not_a_fallback(ps):
    from lowlight_image_enhancement_amd._lib import NBPError
    a = np.zeros((12, 13, 3), np.uint8)
    for fn in (ps.calculate_psnr, ps.calculate_ssim):
        with pytest.raises(NBPError):
            fn(a, a, 0)
        with pytest.raises(NBPError):
            fn(torch.zeros(1, 3, 12, 13), torch.zeros(1, 3, 12, 13), 0)
    with pytest.raises(TypeError):
        ps.psnr_tensor(torch.zeros(1, 3, 12, 13), torch.zeros(1, 3, 12, 13))


def test_reorder_image_and_names(ps):
    x = np.arange(24).reshape(2, 3, 4)
    assert ps.reorder_image(x).shape == (2, 3, 4) and ps.reorder_image(x, "CHW").shape == (3, 4, 2)
    assert np.shares_memory(ps.reorder_image(x, "CHW"), x)
    assert ps.reorder_image(x[0]).shape == (3, 4, 1)
    with pytest.raises(ValueError):
        ps.reorder_image(x, "HW")
    import inspect
    assert list(inspect.signature(ps.calculate_psnr).parameters) == ["img1", "img2", "crop_border", "input_order",
                                                                     "test_y_channel"]
    assert list(inspect.signature(ps.calculate_ssim).parameters) == ["img1", "img2", "crop_border", "input_order",
                                                                     "test_y_channel", "ssim3d"]
    assert inspect.signature(ps.calculate_ssim).parameters["ssim3d"].default is True
    import lowlight_image_enhancement_amd.metrics as m
    assert m.psnr_ssim is ps and "psnr_ssim" in m.__all__
    assert not hasattr(m, "calculate_psnr") and not hasattr(m, "calculate_ssim")  # the module, not the bare names
    from lowlight_image_enhancement_amd.metrics.psnr import calculate_psnr
    assert calculate_psnr is not ps.calculate_psnr


def test_window_is_the_normalised_exponential(ps, gold):
    g = ps.gaussian_window()
    assert g.dtype == np.float64 and g.shape == (11,)
    assert np.array_equal(g, gold["window"])
    assert abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1])
    assert g[5] / g[4] == pytest.approx(np.exp(0.5 / 2.25), rel=1e-15)


# ------------------------------------------------------------------------------------------------ registration
def test_registration_is_opt_in_and_leaves_the_validator_as_it_was(ps):
    from lowlight_image_enhancement_amd import Validator, validation
    had = dict(validation._EXTRA)
    try:
        for name in ("calculate_psnr", "calculate_ssim", "psnr_img"):
            validation._EXTRA.pop(name, None)
        with pytest.raises(ValueError):
            Validator({"metrics": {"p": {"type": "calculate_psnr"}}}, device="cpu")
        ps.register_image_metrics(crop_border=2, test_y_channel=True)
        assert {"calculate_psnr", "calculate_ssim"} <= set(validation._EXTRA)
        assert len(validation.SUPPORTED_METRICS) == 6 and "calculate_psnr" not in validation.SUPPORTED_METRICS
        with pytest.raises(NotImplementedError):
            Validator({"use_image": True, "metrics": {"p": {"type": "calculate_psnr"}}}, device="cpu")
        v = Validator({"metrics": {"p": {"type": "calculate_psnr", "crop_border": 0, "test_y_channel": False},
                                   "s": {"type": "calculate_ssim", "crop_border": 0, "input_order": "HWC",
                                         "ssim3d": False}}}, device="cpu")
        assert v.names == ["p", "s"]
        ps.register_image_metrics(psnr="psnr_img", ssim=None)
        assert "psnr_img" in validation._EXTRA
        with pytest.raises(TypeError):
            ps.register_image_metrics(params=1)
        with pytest.raises(ValueError):
            ps.register_image_metrics(input_order="CHW")
        with pytest.raises(ValueError):
            validation._EXTRA["calculate_psnr"](None, None, input_order="CHW")
    finally:
        validation._EXTRA.clear()
        validation._EXTRA.update(had)


def test_install_aliases_exposes_the_module(ps):
    import lowlight_image_enhancement_amd as pkg
    had = sys.modules.get("basicsr.metrics.psnr_ssim")
    try:
        sys.modules.pop("basicsr.metrics.psnr_ssim", None)
        pkg.install_aliases()
        assert sys.modules["basicsr.metrics.psnr_ssim"] is ps
        sentinel = object()
        sys.modules["basicsr.metrics.psnr_ssim"] = sentinel  # setdefault: what exists stays
        pkg.install_aliases()
        assert sys.modules["basicsr.metrics.psnr_ssim"] is sentinel
    finally:
        sys.modules.pop("basicsr.metrics.psnr_ssim", None)
        if had is not None:
            sys.modules["basicsr.metrics.psnr_ssim"] = had


def test_symbols_are_declared_and_exported():
    from lowlight_image_enhancement_amd import _lib
    sigs = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nbp_bsr_psnr_workspace_bytes", "nbp_bsr_psnr", "nbp_bsr_ssim_workspace_bytes", "nbp_bsr_ssim"):
        assert name in sigs and hasattr(dll, name), name
    assert sigs["nbp_bsr_psnr"][1][-1] == "nbp_stream_t" and sigs["nbp_bsr_ssim"][1][-1] == "nbp_stream_t"
    assert sigs["nbp_bsr_ssim_workspace_bytes"] == ("size_t", ["int", "int", "int"])


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from lowlight_image_enhancement_amd import _lib
    L = _lib.lib().dll
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.nbp_bsr_psnr(None, p, 1, 8, 8, 3, 24, 3, 1, 24, 3, 1, 0, p, p, None) == -1
    assert b"nbp_bsr_psnr" in L.nbp_last_error_string()
    assert L.nbp_bsr_psnr(p, p, 1, 8, 8, 2, 16, 2, 1, 16, 2, 1, 0, p, p, None) == -1
    assert L.nbp_bsr_psnr(p, p, 1, 0, 8, 3, 24, 3, 1, 24, 3, 1, 0, p, p, None) == -1
    assert L.nbp_bsr_ssim(p, p, 1, 8, 8, 3, 24, 3, 1, 24, 3, 1, 3, p, p, p, None) == -1
    assert b"nbp_bsr_ssim" in L.nbp_last_error_string()
    assert L.nbp_bsr_ssim(p, p, 1, 8, 8, 6, 48, 6, 1, 48, 6, 1, 0, p, p, p, None) == -1
    assert L.nbp_bsr_ssim(p, p, 1, 8, 8, 3, 24, 3, 1, 24, 3, 1, 0, None, p, p, None) == -1
    # one (sum for max_value 1, sum for 255, flag) triple of float64 per 32 x 16 tile of the map, at least one
    assert L.nbp_bsr_ssim_workspace_bytes(96, 80, 0) == 6 * 3 * 3 * 8
    assert L.nbp_bsr_ssim_workspace_bytes(96, 80, 1) == 6 * 3 * 3 * 8   # 86 x 70
    assert L.nbp_bsr_ssim_workspace_bytes(26, 42, 1) == 1 * 1 * 3 * 8   # 16 x 32: one tile
    assert L.nbp_bsr_ssim_workspace_bytes(27, 43, 1) == 2 * 2 * 3 * 8
    assert L.nbp_bsr_ssim_workspace_bytes(10, 12, 1) == 3 * 8           # an empty map still has a workspace
    assert L.nbp_bsr_ssim_workspace_bytes(10, 12, 3) == 0
    assert L.nbp_bsr_psnr_workspace_bytes(7, 9) == 16
    assert L.nbp_bsr_psnr_workspace_bytes(4096, 4096) == 1024 * 16


# ------------------------------------------------------------------------------------------------ the fixture
def _along(x, g, axis):
    n = x.shape[axis] - 10
    out = np.zeros([n if a == axis else s for a, s in enumerate(x.shape)])
    for k in range(11):
        out = out + g[k] * np.take(x, range(k, k + n), axis=axis)
    return out


def _ssim_planes(a, b, g, max_value, replicate):
    """the separable float64 SSIM of float64 [H,W,C] planes: replicated border, or the valid region only"""
    if not replicate and (a.shape[0] <= 10 or a.shape[1] <= 10):
        return float("nan")
    q = [a, b, a * a, b * b, a * b]
    if replicate:
        q = [np.pad(x, ((5, 5), (5, 5), (0, 0)), mode="edge") for x in q]
    mu1, mu2, e11, e22, e12 = [_along(_along(x, g, 1), g, 0) for x in q]
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    m = ((2 * mu1 * mu2 + c1) * (2 * (e12 - mu1 * mu2) + c2)) / \
        ((mu1 ** 2 + mu2 ** 2 + c1) * ((e11 - mu1 ** 2) + (e22 - mu2 ** 2) + c2))
    return float(m.mean())


def _numpy_value(ps, a, b, mode):
    mv = lambda x: 1.0 if x.max() <= 1 else 255.0  # noqa: E731
    g = ps.gaussian_window()
    if a.shape[2] == 6:
        return (_numpy_value(ps, a[..., :3], b[..., :3], mode) + _numpy_value(ps, a[..., 3:], b[..., 3:], mode)) / 2
    if mode in ("psnr_y", "ssim_y"):
        a, b = ps.to_y_channel(a).astype(np.float64), ps.to_y_channel(b).astype(np.float64)
    if mode in ("psnr", "psnr_y"):
        mse = np.mean((a - b) ** 2)
        return float("inf") if mse == 0 else float(20.0 * np.log10(mv(a) / np.sqrt(mse)))
    if mode == "ssim_y":
        return _ssim_planes(a, b, g, 255.0, True)
    return _ssim_planes(a, b, g, mv(a), False)


def _close(got, ref, tol):
    if np.isnan(ref):
        return np.isnan(got)
    if np.isinf(ref):
        return got == ref
    return abs(got - ref) <= tol


@pytest.mark.parametrize("run", list(RUNS))
def test_fixture_is_self_consistent(ps, gold, run):
    a, b, checksum, cb, order = run_inputs(run)
    assert checksum == int(gold[f"{run}_checksum"])
    assert a.nbytes <= 40 * 1024  # small inputs only (the largest: 48 x 64 x 3 float32)
    ha, hb = ps.reorder_image(a, order).astype(np.float64), ps.reorder_image(b, order).astype(np.float64)
    if cb:
        ha, hb = ha[cb:-cb, cb:-cb], hb[cb:-cb, cb:-cb]
    tol = {"psnr": float(gold["tol_psnr"]), "psnr_y": float(gold["tol_psnr_y"]), "ssim_valid": float(gold["tol_f64"]),
           "ssim_y": float(gold["tol_f64"])}
    for mode in ("psnr", "psnr_y", "ssim_valid", "ssim_y"):
        got, ref = _numpy_value(ps, ha, hb, mode), float(gold[f"{run}_{mode}"])
        print(f"{run} {mode}: numpy {got!r}, reference {ref!r}, bound {tol[mode]:.3e}")
        assert _close(got, ref, tol[mode]), (run, mode, got, ref)
        assert _close(got, float(gold[f"{run}_{mode}_S"]), 1e-13)


def test_fixture_bounds_are_the_documented_ones(gold):
    assert float(gold["tol_psnr"]) == 1e-12
    assert float(gold["tol_f64"]) == max(16.0 * float(gold["diff_f64"]), 1e-13) and float(gold["tol_f64"]) < 1e-9
    assert float(gold["tol_psnr_y"]) == max(4.0 * float(gold["diff_psnr_y"]), 1e-13)
    assert float(gold["tol_psnr_y"]) < 1e-4  # the reference's own float32 rounding of a value near 38 dB
    for run, (case, _, _) in RUNS.items():
        ref, f, s = (float(gold[f"{run}_ssim3d{k}"]) for k in ("", "_F", "_S"))
        tol = float(gold[f"{run}_tol3d"])
        assert tol == max(2.0 * (abs(ref - f) + abs(f - s)), 1e-7)
        assert tol < (2e-3 if case in FLAT else 1e-5), (run, tol)
        assert case in FLAT or case in TEXTURED or case in ("n10x12", "same")
        assert abs(ref - s) <= tol
    assert float(gold["same_psnr"]) == float("inf") and float(gold["same_ssim3d"]) == 1.0
    assert np.isnan(float(gold["n10x12_ssim_valid"])) and np.isnan(float(gold["n7x9_ssim_valid"]))
    assert set(MODES) == {"psnr", "psnr_y", "ssim3d", "ssim_valid", "ssim_y"} and "left23x80" in CASES
    a, b, _ = pair("le1")
    assert a.max() == 1 and a.dtype == np.uint8
    a, b, _ = pair("f48x64")
    assert a.dtype == np.float32 and a.max() <= 1.0
