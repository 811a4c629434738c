"""Generate the PSNR / SSIM fixture (psnr_ssim.npz) by running the REFERENCE's calculate_psnr / calculate_ssim on the
frame pairs of tests/psnr_ssim_fixtures.py.

Test infrastructure only, as make_golden_niqe.py: the reference's basicsr/metrics/psnr_ssim.py, metric_util.py and
basicsr/utils/matlab_functions.py are loaded by path at run time behind stub packages; nothing of them is stored but
the numbers they produce.  cv2 and skimage are not needed; stand-ins supply what the metrics ask of them (derived from
cv2's documented behaviour, not observed):
  * getGaussianKernel(11, 1.5): exp(-x^2 / (2 sigma^2)) scaled by the reciprocal of its sum, float64, as cv2 computes a
    kernel larger than 7 taps (its fixed tables cover sizes up to 7 only);
  * filter2D(img, -1, window[, borderType]): a float64 correlation per channel, scipy.ndimage.correlate with
    mode='mirror' (cv2's default border, reflect-101) or mode='nearest' (BORDER_REPLICATE).  cv2 may use a DFT at this
    kernel size, so its rounding is not reproducible to the bit and no float64 mode is held to bits;
  * skimage.metrics.structural_similarity: never called.
_ssim_3d calls .cuda(); torch.Tensor.cuda and torch.nn.Module.cuda are made identities in this process, so the
reference's float32 conv3d runs on the CPU unchanged.

Per run and mode the file holds the reference's output, and the generator's float64 re-evaluations that set the
tolerances:
  * S: the same formula filtered separably in float64 (for the 3-D mode from the float32-rounded inputs and products);
  * F (3-D mode): the float64 evaluation with the reference's own float32-rounded 11 x 11 x 11 weights;
  * tol_f64 = max(16 x the largest |reference - S| over the valid and Y SSIM runs, 1e-13);
    tol_psnr_y = max(4 x the largest |reference - S| over the PSNR-Y runs, 1e-13);
    <run>_tol3d = max(2 (|reference - F| + |F - S|), 1e-7), asserted here to be < 1e-5 on the textured runs and < 2e-3
    on the flat one.

Usage:  python tests/golden/make_golden_psnr_ssim.py --ref <checkout of the reference>
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from psnr_ssim_fixtures import CASES, FLAT, MODES, RUNS, mode_kwargs, pair, run_inputs  # noqa: E402

BORDER_REPLICATE = 1


def _get_gaussian_kernel(ksize, sigma):
    assert ksize > 7, "cv2 takes smaller kernels from fixed tables"
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return (t * (1.0 / t.sum())).reshape(-1, 1)


def _filter2d(img, ddepth, kernel, borderType=None):
    from scipy.ndimage import correlate
    assert ddepth == -1 and img.dtype == np.float64
    mode = "nearest" if borderType == BORDER_REPLICATE else "mirror"
    if img.ndim == 2:
        return correlate(img, kernel, mode=mode)
    return np.stack([correlate(img[..., k], kernel, mode=mode) for k in range(img.shape[2])], axis=2)


def load_reference(ref: str):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def load(full, path):
        spec = importlib.util.spec_from_file_location(full, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[full] = m
        spec.loader.exec_module(m)
        return m

    def no_skimage(*a, **k):
        raise AssertionError("skimage is not used")

    base = os.path.join(ref, "NAFNet_base", "basicsr")
    stub("cv2", getGaussianKernel=_get_gaussian_kernel, filter2D=_filter2d, BORDER_REPLICATE=BORDER_REPLICATE,
         INTER_LINEAR=1, COLOR_BGR2GRAY=6)
    stub("skimage")
    stub("skimage.metrics", structural_similarity=no_skimage)
    stub("basicsr")
    stub("basicsr.utils")
    stub("basicsr.metrics")
    load("basicsr.utils.matlab_functions", os.path.join(base, "utils", "matlab_functions.py"))
    load("basicsr.metrics.metric_util", os.path.join(base, "metrics", "metric_util.py"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    return load("basicsr.metrics.psnr_ssim", os.path.join(base, "metrics", "psnr_ssim.py"))


# ------------------------------------------------------------------------------------------ float64 re-evaluations
G = _get_gaussian_kernel(11, 1.5).reshape(-1)


def _along(x, axis):
    """the 11-tap window along one axis of a float64 array, valid region (the caller pads)"""
    n = x.shape[axis] - 10
    out = np.zeros([n if a == axis else s for a, s in enumerate(x.shape)])
    for k in range(11):
        out = out + G[k] * np.take(x, range(k, k + n), axis=axis)
    return out


def _map_mean(mu1, mu2, e11, e22, e12, max_value):
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    mu1_sq, mu2_sq, mu1_mu2 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    m = ((2 * mu1_mu2 + c1) * (2 * (e12 - mu1_mu2) + c2)) / ((mu1_sq + mu2_sq + c1) * ((e11 - mu1_sq) + (e22 - mu2_sq) + c2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return float(m.mean()) if m.size else float("nan")


def sep2d(a, b, max_value, replicate):
    """float64 [H,W] or [H,W,C] planes -> the mean of the separable float64 map"""
    if a.ndim == 2:
        a, b = a[..., None], b[..., None]
    if not replicate and (a.shape[0] <= 10 or a.shape[1] <= 10):
        return float("nan")
    q = [a, b, a * a, b * b, a * b]
    if replicate:
        q = [np.pad(x, ((5, 5), (5, 5), (0, 0)), mode="edge") for x in q]
    return _map_mean(*[_along(_along(x, 1), 0) for x in q], max_value)


def vol3d(a, b, max_value, weights32):
    """the [H,W,C] volumes as the reference forms them (float32, float32 products) -> the float64 map mean, filtered
    separably (weights32 None) or with the given float32-rounded [11,11,11] weights (indexed [h][w][c])"""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    q = [x.astype(np.float64) for x in (a32, b32, a32 * a32, b32 * b32, a32 * b32)]
    q = [np.pad(x, 5, mode="edge") for x in q]
    if weights32 is None:
        f = [_along(_along(_along(x, 1), 0), 2) for x in q]
    else:
        H, W, C = a.shape
        w = weights32.astype(np.float64)
        f = []
        for x in q:
            acc = np.zeros((H, W, C))
            for i in range(11):
                for j in range(11):
                    for k in range(11):
                        acc += w[i, j, k] * x[i:i + H, j:j + W, k:k + C]
            f.append(acc)
    return _map_mean(*f, max_value)


def halves(fn, a, b):
    if a.ndim == 3 and a.shape[2] == 6:
        return (fn(a[..., :3], b[..., :3]) + fn(a[..., 3:], b[..., 3:])) / 2
    return fn(a, b)


def evaluate(ps, a, b, mode, weights32):
    """the generator's own float64 values of a mode on HWC float64 images after the crop: (S, F or None)"""
    mv = lambda x: 1.0 if x.max() <= 1 else 255.0  # noqa: E731
    if mode == "psnr":
        def f(x, y):
            mse = np.mean((x - y) ** 2)
            return float("inf") if mse == 0 else float(20.0 * np.log10(mv(x) / np.sqrt(mse)))
        return halves(f, a, b), None
    if mode == "psnr_y":
        def f(x, y):
            y1, y2 = ps.to_y_channel(x).astype(np.float64), ps.to_y_channel(y).astype(np.float64)
            mse = np.mean((y1 - y2) ** 2)
            return float("inf") if mse == 0 else float(20.0 * np.log10(mv(y1) / np.sqrt(mse)))
        return halves(f, a, b), None
    if mode == "ssim_valid":
        return halves(lambda x, y: sep2d(x, y, mv(x), False), a, b), None
    if mode == "ssim_y":
        def f(x, y):
            y1, y2 = ps.to_y_channel(x).astype(np.float64), ps.to_y_channel(y).astype(np.float64)
            return sep2d(y1[..., 0], y2[..., 0], 255.0, True)
        return halves(f, a, b), None
    s = halves(lambda x, y: vol3d(x, y, mv(x), None), a, b)
    fl = halves(lambda x, y: vol3d(x, y, mv(x), weights32), a, b)
    return s, fl


def explicit_y(x):
    """the rounding chain of the kernels (luma.h), elementwise in numpy"""
    v = x.astype(np.float32) / np.float32(255.0)
    if v.ndim == 3 and v.shape[2] == 3:
        d = ((v[..., 0].astype(np.float64) * 24.966 + v[..., 1].astype(np.float64) * 128.553)
             + v[..., 2].astype(np.float64) * 65.481) + 16.0
        v = (d / 255.0).astype(np.float32)[..., None]
    return v * np.float32(255.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference (the directory that holds NAFNet_base)")
    args = ap.parse_args()
    ps = load_reference(args.ref)
    warnings.filterwarnings("ignore")  # the reference takes the mean of an empty map on the 10 x 12 frame
    conv = ps._generate_3d_gaussian_kernel()
    # conv3d's weight [d][h][w] meets the volume [H][W][C] as (depth, height, width) = (H, W, C)
    weights32 = conv.weight.detach()[0, 0].numpy().astype(np.float32)

    out = {"window": G.copy()}
    d_f64, d_psnr_y, y_mismatch = 0.0, 0.0, 0
    for run, (case, cb, order) in RUNS.items():
        a, b, checksum, cb, order = run_inputs(run)
        out[f"{run}_checksum"] = np.asarray(checksum, dtype=np.int64)
        ha = ps.reorder_image(a, order).astype(np.float64)
        hb = ps.reorder_image(b, order).astype(np.float64)
        if cb:
            ha, hb = ha[cb:-cb, cb:-cb], hb[cb:-cb, cb:-cb]
        for x in (ha, hb):
            for h in ((x[..., :3], x[..., 3:]) if x.shape[2] == 6 else (x,)):
                y_mismatch += int((explicit_y(h).view(np.uint32) != ps.to_y_channel(h).view(np.uint32)).sum())
        for mode in MODES:
            is_ssim, kw = mode_kwargs(mode)
            fn = ps.calculate_ssim if is_ssim else ps.calculate_psnr
            ref = float(fn(a, b, cb, input_order=order, **kw))
            s, fl = evaluate(ps, ha, hb, mode, weights32)
            out[f"{run}_{mode}"] = np.asarray(ref, dtype=np.float64)
            out[f"{run}_{mode}_S"] = np.asarray(s, dtype=np.float64)
            line = f"{run:12s} {mode:10s} ref {ref!r:24} S {s!r:24}"
            if np.isnan(ref) or np.isinf(ref):
                assert (np.isnan(ref) and np.isnan(s)) or ref == s, (run, mode, ref, s)
            elif mode == "ssim3d":
                tol = max(2.0 * (abs(ref - fl) + abs(fl - s)), 1e-7)
                out[f"{run}_{mode}_F"] = np.asarray(fl, dtype=np.float64)
                out[f"{run}_tol3d"] = np.asarray(tol, dtype=np.float64)
                cap = 2e-3 if case in FLAT else 1e-5
                assert tol < cap, f"{run}: tol3d {tol:.3e} breaks the cap {cap:.0e}: replace the fixture"
                line += f" F {fl!r:24} |ref-F| {abs(ref - fl):.2e} |F-S| {abs(fl - s):.2e} tol {tol:.2e}"
            elif mode in ("ssim_valid", "ssim_y"):
                d_f64 = max(d_f64, abs(ref - s))
                line += f" |ref-S| {abs(ref - s):.2e}"
            elif mode == "psnr_y":
                d_psnr_y = max(d_psnr_y, abs(ref - s))
                line += f" |ref-S| {abs(ref - s):.2e}"
            else:
                assert abs(ref - s) <= 1e-12, (run, ref, s)
            print(line)
    # the _left variants: HWC, no crop
    a, b, checksum = pair("left23x80")
    out["left23x80_checksum"] = np.asarray(checksum, dtype=np.int64)
    la, lb = a[:, 64:, :3].astype(np.float64), b[:, 64:, :3].astype(np.float64)
    for mode in MODES:
        is_ssim, kw = mode_kwargs(mode)
        fn = ps.calculate_ssim_left if is_ssim else ps.calculate_psnr_left
        ref = float(fn(a, b, 0, **kw))
        s, fl = evaluate(ps, la, lb, mode, weights32)
        out[f"left23x80_{mode}"] = np.asarray(ref, dtype=np.float64)
        out[f"left23x80_{mode}_S"] = np.asarray(s, dtype=np.float64)
        if mode == "ssim3d":
            tol = max(2.0 * (abs(ref - fl) + abs(fl - s)), 1e-7)
            assert tol < 1e-5, tol
            out["left23x80_ssim3d_F"] = np.asarray(fl, dtype=np.float64)
            out["left23x80_tol3d"] = np.asarray(tol, dtype=np.float64)
        elif mode in ("ssim_valid", "ssim_y"):
            d_f64 = max(d_f64, abs(ref - s))
        elif mode == "psnr_y":
            d_psnr_y = max(d_psnr_y, abs(ref - s))
        print(f"{'left23x80':12s} {mode:10s} ref {ref!r:24} S {s!r:24}")
    assert y_mismatch == 0, f"{y_mismatch} Y values of the explicit chain differ from the reference's to_y_channel"
    out["diff_f64"] = np.asarray(d_f64, dtype=np.float64)
    out["diff_psnr_y"] = np.asarray(d_psnr_y, dtype=np.float64)
    out["tol_f64"] = np.asarray(max(16.0 * d_f64, 1e-13), dtype=np.float64)
    out["tol_psnr_y"] = np.asarray(max(4.0 * d_psnr_y, 1e-13), dtype=np.float64)
    out["tol_psnr"] = np.asarray(1e-12, dtype=np.float64)
    print(f"largest |ref - S|: float64 SSIM modes {d_f64:.3e} -> tol_f64 {float(out['tol_f64']):.3e}; "
          f"PSNR-Y {d_psnr_y:.3e} -> tol_psnr_y {float(out['tol_psnr_y']):.3e}; Y chain mismatches {y_mismatch}")
    path = os.path.join(HERE, "psnr_ssim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
