"""GPU tests of the device NIQE (metrics/niqe.py, niqe.hip) against the reference's calculate_niqe, whose feature
matrices and scores tests/golden/make_golden_niqe.py stored in niqe.npz for the frames of tests/niqe_fixtures.py.

The bounds come from the fixture, not from the device: B_f = 4 x the largest move of a non-alpha feature, and
B_q = 4 x the largest move of the score, when the reference itself is run with its blocks cast to float64 (the
"twin").  The device differs from the reference in what the twin varies -- the precision and order of the block
moments -- plus last-place differences of the MSCN map of the same order; hence the margin of 4.  An alpha entry is a
table index: at most 1 % of a case's finite alpha entries may sit one table step (0.001) away, none further.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from niqe_fixtures import GOLDEN_CASES, frame

pytestmark = pytest.mark.gpu

PARAMS = os.path.join(GOLDEN, "niqe_pris_params.npz")
ALPHA_COLS = [s * 18 + c for s in (0, 1) for c in (0, 2, 6, 10, 14)]
OTHER_COLS = [c for c in range(36) if c not in ALPHA_COLS]
ALPHA_CAP = 0.01

_RUNS = {}


@pytest.fixture(scope="module")
def gold():
    return golden("niqe.npz")


def _bounds(gold):
    b_f = 4.0 * max(float(gold[f"{c}_twin_feat_rel"]) for c in GOLDEN_CASES)
    b_q = 4.0 * max(float(gold[f"{c}_twin_score_rel"]) for c in GOLDEN_CASES)
    return b_f, b_q


def _run(case, dev):
    """(frame checksum, features [blocks, 36], score) of a case on the device, computed once"""
    if case not in _RUNS:
        from lowlight_image_enhancement_amd.metrics import calculate_niqe, niqe_features
        img, checksum, cb, order = frame(case)
        t = torch.from_numpy(img).to(dev)
        feat = niqe_features(t, cb, order, params=PARAMS)
        q = calculate_niqe(t, cb, order, params=PARAMS)
        assert q.dtype == torch.float64 and q.dim() == 0 and q.is_cuda
        assert feat.dtype == torch.float64 and feat.is_cuda
        _RUNS[case] = (checksum, feat.cpu().numpy(), float(q.cpu()), q)
    return _RUNS[case]


def _alpha_steps(got, ref):
    """table steps between the finite alpha entries of two feature matrices (NaN patterns already equal)"""
    a, b = got[:, ALPHA_COLS], ref[:, ALPHA_COLS]
    fin = ~np.isnan(b)
    steps = np.zeros(a.shape)
    steps[fin] = np.abs(a[fin] - b[fin]) / 0.001
    return steps, fin


def _score_numpy(feat):
    p = np.load(PARAMS)
    mu = np.nanmean(feat, axis=0)
    clean = feat[~np.isnan(feat).any(axis=1)]
    cov = np.cov(clean, rowvar=False)
    d = p["mu_pris_param"].reshape(-1) - mu
    return float(np.sqrt(d @ np.linalg.pinv((p["cov_pris_param"] + cov) / 2) @ d))


# ------------------------------------------------------------------------------------------------ per case
@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_niqe_against_reference(dev, gold, case):
    b_f, b_q = _bounds(gold)
    checksum, feat, q, _ = _run(case, dev)
    ref, q_ref = gold[f"{case}_feat"], float(gold[f"{case}_score"])
    # (1) the regenerated frame is the generator's
    assert checksum == int(gold[f"{case}_checksum"])
    assert feat.shape == ref.shape
    # (3) NaN pattern
    assert np.array_equal(np.isnan(feat), np.isnan(ref))
    if case == "D":
        zero_row = np.isnan(ref).any(axis=1)
        assert zero_row.sum() == 1 and zero_row[0]
        assert np.all(feat[0, ALPHA_COLS] == 0.2)  # np.argmin of NaNs: index 0, at both scales
        assert np.all(np.isnan(feat[0, OTHER_COLS]))
    # (4) alpha entries
    steps, fin = _alpha_steps(feat, ref)
    n_fin = int(fin.sum())
    moved = steps > 1e-6
    print(f"{case}: blocks {feat.shape[0]}, finite alpha entries {n_fin}, moved {int(moved.sum())}, "
          f"largest move {steps.max():.3g} steps; twin moved {int(gold[f'{case}_twin_alpha_moved'])}")
    assert int(gold[f"{case}_twin_alpha_moved"]) <= ALPHA_CAP * n_fin, "the inputs, not the device, are at fault"
    assert np.all(np.abs(steps[moved] - 1.0) < 1e-6), steps[moved]
    assert moved.sum() <= ALPHA_CAP * n_fin
    # (5) the other features, over the rows whose alpha entries all agree
    rows = ~moved.any(axis=1)
    a, b = feat[rows][:, OTHER_COLS], ref[rows][:, OTHER_COLS]
    rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-3)
    rel = rel[~np.isnan(rel)]
    print(f"{case}: other features, largest relative difference {rel.max():.3e} (B_f {b_f:.3e})")
    assert rel.max() <= b_f
    # (6) the score stage alone: numpy on the device's own features
    q_np = _score_numpy(feat)
    print(f"{case}: score {q!r}, numpy on the device's features {q_np!r}, reference {q_ref!r}, "
          f"relative {abs(q - q_ref) / abs(q_ref):.3e} (B_q {b_q:.3e})")
    assert abs(q - q_np) <= 1e-8 * abs(q_np)
    # (7) end to end, where no alpha entry moved
    if not moved.any():
        assert abs(q - q_ref) <= b_q * abs(q_ref)


def test_luma_within_one_ulp(dev, gold):
    from lowlight_image_enhancement_amd._lib import call
    img = frame("A")[0]
    t = torch.from_numpy(img).to(dev)
    H, W, _ = img.shape
    y = torch.empty(H, W, dtype=torch.float32, device=dev)
    call("niqe_luma", t, 1, H, W, 3, t.stride(0), t.stride(1), t.stride(2), y)
    got, ref = y.cpu().numpy(), gold["A_y"]
    assert ref.dtype == np.float32 and got.shape == ref.shape
    ulp = np.spacing(np.abs(ref))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(f"luma: {int((got != ref).sum())} of {ref.size} pixels differ, largest difference {float((err / ulp).max()):.2f} ulp")
    assert np.all(err <= ulp)


# ------------------------------------------------------------------------------------------------ layouts, determinism
def test_chw_is_bitwise_hwc(dev):
    _, feat_a, _, q_a = _run("A", dev)
    _, feat_c, _, q_c = _run("G_chw", dev)
    assert np.array_equal(feat_a, feat_c, equal_nan=True)
    assert torch.equal(q_a.view(torch.int64), q_c.view(torch.int64))


def test_strided_view_needs_no_copy(dev):
    """a CHW device tensor permuted to HWC (a view) and a cropped window of a larger buffer give A's bits"""
    from lowlight_image_enhancement_amd.metrics import calculate_niqe
    _, _, _, q_a = _run("A", dev)
    img = frame("A")[0]
    big = torch.zeros(200, 210, 3, dtype=torch.uint8, device=dev)
    big[3:195, 5:197] = torch.from_numpy(img).to(dev)
    q = calculate_niqe(big[3:195, 5:197], 0, params=PARAMS)
    assert torch.equal(q.view(torch.int64), q_a.view(torch.int64))
    q = calculate_niqe(frame("A")[0], 0, params=PARAMS)  # a numpy array is uploaded
    assert torch.equal(q.view(torch.int64), q_a.view(torch.int64))


def test_two_runs_are_bitwise_equal(dev):
    from lowlight_image_enhancement_amd.metrics import calculate_niqe, niqe_features
    _, feat, _, q = _run("F", dev)
    img, _, cb, order = frame("F")
    t = torch.from_numpy(img).to(dev)
    feat2 = niqe_features(t, cb, order, params=PARAMS).cpu().numpy()
    q2 = calculate_niqe(t, cb, order, params=PARAMS)
    assert np.array_equal(feat.view(np.int64), feat2.view(np.int64))
    assert torch.equal(q.view(torch.int64), q2.view(torch.int64))


def test_fewer_than_two_clean_rows_is_nan(dev):
    from lowlight_image_enhancement_amd.metrics import calculate_niqe
    one_block = torch.from_numpy(frame("A")[0][:100, :100].copy()).to(dev)
    assert torch.isnan(calculate_niqe(one_block, 0, params=PARAMS)).item()


# ------------------------------------------------------------------------------------------------ routes
def test_niqe_tensor_is_calculate_niqe_of_tensor2img(dev):
    from lowlight_image_enhancement_amd.imgout import _quantize
    from lowlight_image_enhancement_amd.metrics import calculate_niqe, niqe_tensor
    img = frame("B")[0]
    t = (torch.from_numpy(img).to(dev).permute(2, 0, 1).float() / 255.0 * 1.1 - 0.03).unsqueeze(0).contiguous()
    assert tuple(t.shape) == (1, 3, 200, 301)
    q = niqe_tensor(t, params=PARAMS)
    hwc = _quantize(t[0], 0.0, 1.0, True)  # tensor2img's device bytes (BGR)
    q_ref = calculate_niqe(hwc, 0, params=PARAMS)
    assert q.dtype == torch.float64 and q.dim() == 0
    assert torch.equal(q.view(torch.int64), q_ref.view(torch.int64))
    from lowlight_image_enhancement_amd.imgout import tensor2img
    q_host = calculate_niqe(tensor2img(t), 0, params=PARAMS)  # the same bytes through the host
    assert torch.equal(q.view(torch.int64), q_host.view(torch.int64))


def test_validator_with_registered_niqe(dev):
    from lowlight_image_enhancement_amd.metrics import niqe_tensor, register_niqe_metric
    from lowlight_image_enhancement_amd.validation import Validator
    register_niqe_metric("niqe_y", params=PARAMS)
    v = Validator({"metrics": {"n": {"type": "niqe_y"}}}, device=dev)
    items = []
    for case in ("A", "B"):
        img = frame(case)[0]
        items.append((torch.from_numpy(img).to(dev).permute(2, 0, 1).float() / 255.0).unsqueeze(0).contiguous())
    for t in items:
        v.update(t, torch.zeros_like(t))
    want = sum(float(niqe_tensor(t, params=PARAMS).cpu()) for t in items) / 2
    assert v.result()["n"] == pytest.approx(want, rel=1e-12)
    with pytest.raises(ValueError):
        Validator({"metrics": {"niqe": {"type": "calculate_niqe"}}}, device=dev)
