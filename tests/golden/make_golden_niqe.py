"""Generate the NIQE fixture (niqe.npz) by running the REFERENCE's calculate_niqe on the frames of tests/niqe_fixtures.py.

Test infrastructure only, as make_golden_tlsc.py: the reference's basicsr/metrics/niqe.py, metric_util.py and
basicsr/utils/matlab_functions.py are loaded by path at run time behind stub packages; nothing of them is stored but the
numbers they produce.  cv2 is not needed: a stand-in supplies `resize`, which asserts the exact 2:1 ratio the metric
always asks for and applies the pair means that INTER_LINEAR reduces to at that ratio (source coordinate 2 dx + 0.5:
weights 1/2, 1/2), each rounded to float32.

Per case the file holds the frame's shape, seed, checksum and crop_border, the reference's feature matrix
[blocks][36] (compute_feature is wrapped to capture it) and score, and the TWIN DEVIATION: the same reference code with
every block cast to float64 before compute_feature -- the number of alpha entries that moved, the largest relative move
of the other features over the rows whose alpha entries agree (denominator max(|ref|, 1e-3)) and the relative move of
the score.  It also holds the Y plane of case A, scipy's r_gam table and the reference's CPU seconds for the largest
case, labelled with the CPU it ran on.

Usage:  python tests/golden/make_golden_niqe.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import platform
import shutil
import sys
import time
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from niqe_fixtures import CASES, GOLDEN_CASES, frame  # noqa: E402

ALPHA_COLS = [s * 18 + c for s in (0, 1) for c in (0, 2, 6, 10, 14)]
OTHER_COLS = [c for c in range(36) if c not in ALPHA_COLS]


def _resize(img, dsize, interpolation=None):
    w, h = dsize
    H, W = img.shape
    assert H == 2 * h and W == 2 * w, "the metric halves an even-sized frame: an exact 2:1 ratio"
    x = img.astype(np.float32)
    half = np.float32(0.5)
    hx = x[:, 0::2] * half + x[:, 1::2] * half
    return (hx[0::2] * half + hx[1::2] * half).astype(img.dtype)


def load_reference_niqe(ref: str):
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

    base = os.path.join(ref, "NAFNet_base", "basicsr")
    stub("cv2", resize=_resize, INTER_LINEAR=1, COLOR_BGR2GRAY=6)
    stub("basicsr")
    stub("basicsr.utils")
    stub("basicsr.metrics")
    load("basicsr.utils.matlab_functions", os.path.join(base, "utils", "matlab_functions.py"))
    load("basicsr.metrics.metric_util", os.path.join(base, "metrics", "metric_util.py"))
    return load("basicsr.metrics.niqe", os.path.join(base, "metrics", "niqe.py"))


def run(nq, img, crop_border, order, f64_blocks=False):
    """(score, features [blocks][36], seconds) of the reference's calculate_niqe"""
    feats = []
    orig = nq.compute_feature

    def capture(block):
        f = orig(block.astype(np.float64) if f64_blocks else block)
        feats.append(f)
        return f

    nq.compute_feature = capture
    try:
        t0 = time.process_time()
        q = float(nq.calculate_niqe(img, crop_border, input_order=order))
        dt = time.process_time() - t0
    finally:
        nq.compute_feature = orig
    f = np.asarray(feats, dtype=np.float64)
    n = f.shape[0] // 2
    return q, np.concatenate([f[:n], f[n:]], axis=1), dt


def cpu_label():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    warnings.filterwarnings("ignore")  # the reference takes the mean of empty slices on flat blocks
    nq = load_reference_niqe(args.ref)
    pris = os.path.join(args.ref, "NAFNet_base", "basicsr", "metrics", "niqe_pris_params.npz")
    shutil.copyfile(pris, os.path.join(HERE, "niqe_pris_params.npz"))
    os.chdir(os.path.join(args.ref, "NAFNet_base"))  # calculate_niqe loads its parameters by a relative path

    out = {}
    for name in GOLDEN_CASES:
        kind, h, w, seed, cb, order = CASES[name]
        img, checksum, cb, order = frame(name)
        q, feat, dt = run(nq, img, cb, order)
        q64, feat64, _ = run(nq, img, cb, order, f64_blocks=True)
        assert np.array_equal(np.isnan(feat), np.isnan(feat64)), name
        steps = np.rint(np.nan_to_num(np.abs(feat[:, ALPHA_COLS] - feat64[:, ALPHA_COLS])) / 0.001)
        rows = (steps == 0).all(axis=1)
        a, b = feat[rows][:, OTHER_COLS], feat64[rows][:, OTHER_COLS]
        with np.errstate(invalid="ignore"):
            rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-3)
        rel = rel[~np.isnan(rel)]
        out[f"{name}_shape"] = np.asarray(img.shape, dtype=np.int64)
        out[f"{name}_seed"] = np.asarray(seed, dtype=np.int64)
        out[f"{name}_checksum"] = np.asarray(checksum, dtype=np.int64)
        out[f"{name}_crop_border"] = np.asarray(cb, dtype=np.int64)
        out[f"{name}_feat"] = feat
        out[f"{name}_score"] = np.asarray(q, dtype=np.float64)
        out[f"{name}_twin_alpha_moved"] = np.asarray(int((steps != 0).sum()), dtype=np.int64)
        out[f"{name}_twin_feat_rel"] = np.asarray(rel.max() if rel.size else 0.0, dtype=np.float64)
        out[f"{name}_twin_score_rel"] = np.asarray(abs(q64 - q) / abs(q), dtype=np.float64)
        print(f"{name}: {img.shape} {img.dtype} blocks {feat.shape[0]} score {q:.9f} nan rows "
              f"{int(np.isnan(feat).any(axis=1).sum())} twin: alpha moved {int((steps != 0).sum())}, "
              f"features {out[f'{name}_twin_feat_rel']:.3e}, score {out[f'{name}_twin_score_rel']:.3e}  ({dt:.2f} s)")
        if name == "F":
            out["ref_cpu_seconds"] = np.asarray(dt, dtype=np.float64)
            out["ref_cpu_case"] = np.asarray(f"case F, {h} x {w}, {feat.shape[0]} blocks")
            out["ref_cpu_label"] = np.asarray(cpu_label())
    img_a = frame("A")[0]
    out["A_y"] = nq.to_y_channel(nq.reorder_image(img_a.astype(np.float32), input_order="HWC")).squeeze().astype(np.float32)
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    from scipy.special import gamma
    out["r_gam"] = np.square(gamma(rec * 2)) / (gamma(rec) * gamma(rec * 3))
    path = os.path.join(HERE, "niqe.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
