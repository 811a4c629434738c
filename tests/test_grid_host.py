"""Tiled inference (val.grids) without a GPU: the Python plan (tiling.grid_plan) and the C-ABI plan (nbp_grid_plan)
against every plan the reference's grids() produced (tests/golden/grid_plans.npz, made by make_golden_grids.py), their
error cases, and a numpy restatement of grids_inverse() against the reference's outputs (grid_blend.npz), which pins
what the fixture means: per pixel the covering tiles are added in tile order onto +0, one fp32 add at a time, and the sum
is divided by their number."""
import ctypes

import numpy as np
import pytest

from conftest import golden

W8_CFG = dict(img_channel=3, width=8, enc_blk_nums=[1, 1], middle_blk_num=1, dec_blk_nums=[1, 1])  # grid_nets.npz


def plan_cases(g):
    """[(h, w, val_opt, crop_h, crop_w, i origins, j origins)] of the hand-picked plans"""
    out = []
    for k in range(int(g["n_cases"])):
        h, w = (int(v) for v in g[f"hw_{k}"])
        size, ratio = g[f"size_{k}"], g[f"ratio_{k}"]
        opt = {}
        for a, name in enumerate(("h", "w")):
            if size[a] >= 0:
                opt[f"crop_size_{name}"] = int(size[a])
            else:
                opt[f"crop_size_{name}_ratio"] = float(ratio[a])
        ch, cw = (int(v) for v in g[f"crop_{k}"])
        out.append((h, w, opt, ch, cw, [int(v) for v in g[f"i_{k}"]], [int(v) for v in g[f"j_{k}"]]))
    return out


def c_plan(h, w, ch, cw):
    """nbp_grid_plan through ctypes: (return code, n_rows, step_i, n_cols, step_j)"""
    from lowlight_image_enhancement_amd._lib import lib
    out = (ctypes.c_int * 4)(-7, -7, -7, -7)
    base = ctypes.addressof(out)
    rc = lib().dll.nbp_grid_plan(h, w, ch, cw, base, base + 4, base + 8, base + 12)
    return (rc,) + tuple(out)


def origins(h, c, n, step):
    """tile origins of one axis from the C-ABI plan: k * step, and h - c for the last"""
    return [k * step for k in range(n - 1)] + [h - c]


def blend_restated(outs, h, w, ii, jj):
    """grids_inverse() (image_restoration_model.py:221-245) per tile in tile order.  The adds are formed in float64 and
    rounded to float32 after each one: the float64 sum of two float32 values rounded once is the correctly rounded
    float32 sum (53 >= 2 * 24 + 2 bits), so every step is the reference's fp32 `+=`.  The division by 1, 2 or 4 is exact."""
    T, C, ch, cw = outs.shape
    acc = np.zeros((C, h, w), dtype=np.float32)
    cnt = np.zeros((h, w), dtype=np.float64)
    for t in range(T):
        i, j = ii[t], jj[t]
        win = acc[:, i:i + ch, j:j + cw]
        win[...] = (win.astype(np.float64) + outs[t].astype(np.float64)).astype(np.float32)
        cnt[i:i + ch, j:j + cw] += 1.0
    return (acc.astype(np.float64) / cnt).astype(np.float32), cnt


def test_grid_plan_matches_the_reference():
    from lowlight_image_enhancement_amd.tiling import grid_plan
    g = golden("grid_plans.npz")
    cases = plan_cases(g)
    assert len(cases) == 7
    for h, w, opt, ch, cw, ii, jj in cases:
        got = grid_plan(h, w, opt)
        assert got[:2] == (ch, cw), (h, w, opt)
        assert got[2] == [{"i": i, "j": j} for i, j in zip(ii, jj)], (h, w, opt)
    assert sorted(set(cases[5][5])) == [0, 19, 38, 57, 73]  # the clamped last row of 97 / 24
    assert cases[3][3:5] == (25, 26)  # int(0.5 * 50), int(0.34 * 77)


def test_c_plan_matches_the_reference():
    g = golden("grid_plans.npz")
    for h, w, _, ch, cw, ii, jj in plan_cases(g):
        rc, nr, si, nc, sj = c_plan(h, w, ch, cw)
        assert rc == 0
        ri, cj = origins(h, ch, nr, si), origins(w, cw, nc, sj)
        assert [i for i in ri for _ in cj] == ii and cj * nr == jj, (h, w, ch, cw)  # row-major tile order


def test_both_plans_match_the_reference_sweep():
    from lowlight_image_enhancement_amd.tiling import grid_plan
    g = golden("grid_plans.npz")
    oh, oc = (int(v) for v in g["sweep_other"])
    hc, off = g["sweep_hc"], g["sweep_off"]
    assert len(hc) == 64 * 65 // 2
    for k, (h, c) in enumerate(hc):
        h, c = int(h), int(c)
        rows = [int(v) for v in g["sweep_rows"][off[k]:off[k + 1]]]
        cols = [int(v) for v in g["sweep_cols"][off[k]:off[k + 1]]]
        assert rows == cols and len(rows) == (h - 1) // c + 1
        # the swept axis as rows ...
        idx = grid_plan(h, oh, {"crop_size_h": c, "crop_size_w": oc})[2]
        assert idx == [{"i": i, "j": j} for i in rows for j in (0, 2)], (h, c)
        rc, nr, si, nc, sj = c_plan(h, oh, c, oc)
        assert rc == 0 and origins(h, c, nr, si) == rows and origins(oh, oc, nc, sj) == [0, 2], (h, c)
        # ... and as columns
        idx = grid_plan(oh, h, {"crop_size_h": oc, "crop_size_w": c})[2]
        assert idx == [{"i": i, "j": j} for i in (0, 2) for j in cols], (h, c)
        rc, nr, si, nc, sj = c_plan(oh, h, oc, c)
        assert rc == 0 and origins(h, c, nc, sj) == cols and origins(oh, oc, nr, si) == [0, 2], (h, c)


def test_plans_agree_at_frame_sizes():
    """the integer step against the reference's float expression where the fixtures do not reach: SID frames and extents
    near 2^31"""
    from lowlight_image_enhancement_amd.tiling import grid_plan
    for h, w, ch, cw in [(2848, 4256, 256, 256), (1424, 2128, 256, 256), (2848, 4256, 255, 257), (1001, 999, 100, 37)]:
        idx = grid_plan(h, w, {"crop_size_h": ch, "crop_size_w": cw})[2]
        rc, nr, si, nc, sj = c_plan(h, w, ch, cw)
        assert rc == 0 and nr * nc == len(idx)
        assert idx == [{"i": i, "j": j} for i in origins(h, ch, nr, si) for j in origins(w, cw, nc, sj)]
    import math
    for h, c in [(2 ** 31 - 1, 2 ** 30), (2 ** 31 - 1, 65536), (2 ** 31 - 1, 46341), (2 ** 31 - 2, 3), (2 ** 31 - 1, 3), (2 ** 31 - 1, 1),
                 (2 ** 31 - 1, 2 ** 31 - 2)]:
        n = (h - 1) // c + 1
        step = c if n == 1 else math.ceil((h - c) / (n - 1) - 1e-8)
        assert c_plan(h, 8, c, 8)[:3] == (0, n, step) and c_plan(8, h, 8, c)[3:] == (n, step), (h, c)


def test_error_cases():
    from lowlight_image_enhancement_amd._lib import lib
    from lowlight_image_enhancement_amd.tiling import grid_plan
    opt = {"crop_size_h": 32, "crop_size_w": 32}
    with pytest.raises(ValueError):
        grid_plan(64, 64, opt, scale=2)
    with pytest.raises(ValueError):
        grid_plan(31, 64, opt)  # crop_h > h
    with pytest.raises(ValueError):
        grid_plan(64, 31, opt)  # crop_w > w
    with pytest.raises(ValueError):
        grid_plan(64, 64, {"crop_size_h_ratio": 1.5, "crop_size_w": 32})
    with pytest.raises(KeyError):
        grid_plan(64, 64, {"crop_size_w": 32})
    with pytest.raises(KeyError):
        grid_plan(64, 64, {"crop_size_h": 32, "crop_size_h_ratio": 0.5})  # neither key of the w axis
    assert grid_plan(64, 64, {"crop_size_h": 32, "crop_size_h_ratio": 0.25, "crop_size_w": 64})[0] == 32  # size wins
    err = -1  # NBP_ERR_ARG
    for h, w, ch, cw in [(64, 64, 0, 32), (64, 64, 32, 0), (64, 64, -3, 32), (31, 64, 32, 32), (64, 31, 32, 32)]:
        assert c_plan(h, w, ch, cw) == (err, -7, -7, -7, -7), (h, w, ch, cw)  # refused, outputs untouched
    assert b"crop" in lib().dll.nbp_last_error_string()


def test_package_exports():
    import lowlight_image_enhancement_amd as pkg
    from lowlight_image_enhancement_amd import tiling
    assert pkg.grid_plan is tiling.grid_plan and pkg.tiled_forward is tiling.tiled_forward
    assert pkg.val_forward is tiling.val_forward


def test_restated_blend_reproduces_the_reference():
    g, plans = golden("grid_blend.npz"), plan_cases(golden("grid_plans.npz"))
    cases = [int(k) for k in g["cases"]]
    assert [plans[k][:2] + plans[k][3:5] for k in cases] == [(97, 61, 24, 40), (33, 32, 32, 32), (64, 96, 32, 32),
                                                              (65, 100, 32, 33)]
    for k in cases:
        h, w, _, ch, cw, ii, jj = plans[k]
        outs, ref = g[f"outs_{k}"], g[f"out_{k}"]
        assert outs.shape == (len(ii), 3, ch, cw) and ref.shape == (1, 3, h, w)
        got, cnt = blend_restated(outs, h, w, ii, jj)
        assert set(np.unique(cnt)) <= {1.0, 2.0, 4.0} and cnt.min() >= 1.0
        assert np.array_equal(got.view(np.int32), ref[0].view(np.int32)), k  # bit for bit, signed zeros included
        neg = np.signbit(outs) & (outs == 0)
        assert neg.sum() > 100 and not (np.signbit(ref) & (ref == 0)).any()  # -0.0 went in, only +0.0 comes out
