"""GPU: the validation-pass statistics kernels (valstats.hip) through metrics.valstats.

  * nbp_quantile_select against torch.sort on the device (equality by value; no -0.0 in the inputs), quantile_rows
    against CPU torch.quantile of the downloaded row within 2 fp32 ulp (one lerp of the same two floats and weight on
    either side; the two may contract differently), and above torch.quantile's 2^24-element cap;
  * nbp_val_color_maps against the float64 oracle (oracle/losses.py): the ΔE00 map with the unfused kernel's bound, the
    Sobel magnitude within 2x the error of the existing rgb_to_lab -> sobel_mag kernels (the factor allows for a
    different FMA contraction of the same expressions), de_mean and nbp_masked_mean against float64 sums of the
    kernel's own downloaded maps;
  * color_stats against the oracle with the bounds of tests/test_gpu_color_metrics.py.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- select
def _check_select(x, q):
    """both order statistics of every row against the sorted row; returns (k_lo, k_hi, weight, sorted rows)"""
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rank, quantile_select
    k_lo, k_hi, w = quantile_rank(x.shape[1], q)
    out = quantile_select(x, k_lo, k_hi)
    s = torch.sort(x, dim=1).values
    assert out.shape == (x.shape[0], 2)
    assert torch.equal(out[:, 0], s[:, k_lo]), (out[:, 0], s[:, k_lo])
    assert torch.equal(out[:, 1], s[:, k_hi]), (out[:, 1], s[:, k_hi])
    return k_lo, k_hi, w, s


def _check_rows_vs_cpu_quantile(x, q):
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rows
    got = quantile_rows(x, q).cpu().numpy()
    ref = torch.quantile(x.cpu(), q, dim=1).numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2 * np.spacing(np.abs(ref))).all(), (got, ref)


def _rand(dev, shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def test_select_uniform_rows_both_signs(dev):
    x = _rand(dev, (3, 1517), 1) * 2.0 - 1.0
    assert (x < 0).any() and (x > 0).any()
    k_lo, k_hi, w, _ = _check_select(x, 0.85)
    assert (k_lo, k_hi) == (1288, 1289) and w == 0.5999755859375
    _check_rows_vs_cpu_quantile(x, 0.85)
    for q in (0.0, 1.0, 0.5):  # the ends: minimum and maximum
        _check_select(x, q)


def test_select_tiny_rows(dev):
    _check_select(_rand(dev, (2, 1), 2) - 0.5, 0.85)
    k_lo, k_hi, w, _ = _check_select(_rand(dev, (2, 2), 3) - 0.5, 0.5)
    assert (k_lo, k_hi, w) == (0, 1, 0.5)
    _check_rows_vs_cpu_quantile(_rand(dev, (2, 2), 3) - 0.5, 0.5)
    _check_rows_vs_cpu_quantile(_rand(dev, (1, 1), 4), 0.85)


def test_select_all_equal_row(dev):
    x = torch.full((1, 4099), 0.3125, device=dev)
    _check_select(x, 0.85)
    _check_rows_vs_cpu_quantile(x, 0.85)


def test_select_ties_over_several_blocks(dev):
    vals = torch.tensor([-2.5, -1e-3, 0.25, 0.2500001, 7e8])
    idx = torch.randint(0, 5, (2, 70001), generator=torch.Generator().manual_seed(5))
    x = vals[idx].to(dev)
    for q in (0.85, 0.2, 0.5):
        _check_select(x, q)
    _check_rows_vs_cpu_quantile(x, 0.85)


def test_select_values_differing_in_the_last_pass_bits_only(dev):
    base = 1.0 + torch.arange(1024, dtype=torch.float64) * 2.0 ** -23
    x = base.to(torch.float32).repeat(3)
    assert torch.unique(x).numel() == 1024
    x = x[torch.randperm(x.numel(), generator=torch.Generator().manual_seed(6))].view(1, -1).to(dev)
    for q in (0.85, 0.5, 0.001):
        _check_select(x, q)
    _check_rows_vs_cpu_quantile(x, 0.85)


def test_select_ranks_in_different_top_level_bins(dev):
    n = 1000
    x = torch.cat([torch.full((n // 2,), 0.5), torch.full((n // 2,), 2.0)])
    x = x[torch.randperm(n, generator=torch.Generator().manual_seed(7))].view(1, -1).to(dev)
    k_lo, k_hi, w, s = _check_select(x, 0.5)
    assert (k_lo, k_hi) == (499, 500) and s[0, k_lo] == 0.5 and s[0, k_hi] == 2.0
    _check_rows_vs_cpu_quantile(x, 0.5)


def test_select_integral_rank(dev):
    x = _rand(dev, (2, 101), 8) * 10.0 - 5.0
    k_lo, k_hi, w, _ = _check_select(x, 0.85)
    assert k_lo == k_hi == 85 and w == 0.0
    _check_rows_vs_cpu_quantile(x, 0.85)


def test_select_nan_row_yields_nan_and_neighbours_are_exact(dev):
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rank, quantile_rows, quantile_select
    x = _rand(dev, (3, 1517), 9) * 2.0 - 1.0
    x[1, 700] = float("nan")
    k_lo, k_hi, _ = quantile_rank(1517, 0.85)
    out = quantile_select(x, k_lo, k_hi)
    assert torch.isnan(out[1]).all()
    s = torch.sort(x[[0, 2]], dim=1).values
    assert torch.equal(out[[0, 2], 0], s[:, k_lo]) and torch.equal(out[[0, 2], 1], s[:, k_hi])
    r = quantile_rows(x, 0.85)
    assert torch.isnan(r[1]) and not torch.isnan(r[[0, 2]]).any()


def test_select_above_the_torch_quantile_cap(dev):
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rows
    n = 2 ** 24 + 5
    x = torch.randn(1, n, device=dev, generator=torch.Generator(device=dev).manual_seed(10))
    with pytest.raises(RuntimeError):
        torch.quantile(x, 0.85, dim=1)
    k_lo, k_hi, w, s = _check_select(x, 0.85)
    assert k_hi > 2 ** 23
    assert torch.equal(quantile_rows(x, 0.85), torch.lerp(s[:, k_lo], s[:, k_hi], w))


def test_select_and_rows_refuse_bad_arguments(dev):
    from lowlight_image_enhancement_amd._lib import NBPError
    from lowlight_image_enhancement_amd.metrics.valstats import quantile_rows, quantile_select
    x = _rand(dev, (2, 10), 11)
    for k in ((-1, 3), (4, 3), (3, 10)):
        with pytest.raises(ValueError):
            quantile_select(x, *k)
    for q in (-0.01, 1.01):
        with pytest.raises(ValueError):
            quantile_rows(x, q)
    with pytest.raises(ValueError):
        quantile_rows(x[0], 0.5)
    with pytest.raises(NBPError):
        quantile_rows(x.cpu(), 0.5)


# ---------------------------------------------------------------------------------------------- colour maps
def _rgb_pair(shape, seed, spill=True):
    """the recipe of tests/test_gpu_color_metrics.py"""
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(*shape, generator=gen) * (1.2 if spill else 1.0) - (0.1 if spill else 0.0)  # some outside [0,1]
    b = torch.rand(*shape, generator=gen)
    a[0, :, 0, 0] = 0.0   # exact clamp boundaries
    a[0, :, 0, 1 % shape[3]] = 1.0
    return a, b


@functools.lru_cache(maxsize=None)
def _oracle(shape, seed, spill=False):
    """(pred, tgt, float64 ΔE00 map [N,H,W], float64 Sobel magnitude [N,H,W], float64 L [N,1,H,W]) — computed once"""
    from oracle.losses import deltae00_metric_map, rgb_to_lab
    a, b = _rgb_pair(shape, seed, spill)
    if spill:
        b = b * 1.2 - 0.1
    lab = rgb_to_lab(a.double().clamp(0.0, 1.0))
    de = deltae00_metric_map(lab, rgb_to_lab(b.double().clamp(0.0, 1.0)))
    kx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=torch.float64).view(1, 1, 3, 3)
    ky = kx.transpose(2, 3).contiguous()
    L = lab[:, 0:1]
    grad = torch.sqrt(Fn.conv2d(L, kx, padding=1) ** 2 + Fn.conv2d(L, ky, padding=1) ** 2 + 1e-12)
    return a, b, de, grad[:, 0], L


def _unfused_grad(pred_dev):
    """today's kernels: nbp_rgb_to_lab -> nbp_sobel_mag"""
    from lowlight_image_enhancement_amd._lib import call
    N, _, H, W = pred_dev.shape
    lab = torch.empty_like(pred_dev)
    call("rgb_to_lab", pred_dev, N, H, W, lab)
    grad = torch.empty(N, H, W, device=pred_dev.device)
    call("sobel_mag", lab, N, H, W, grad)
    return grad


def _check_maps(dev, shape, seed, spill):
    from lowlight_image_enhancement_amd.metrics.valstats import color_maps, masked_mean, quantile_rows
    a, b, de_ref, grad_ref, _ = _oracle(shape, seed, spill)
    pa, pb = a.to(dev), b.to(dev)
    de, grad, de_mean = color_maps(pa, pb, clamp=True)
    N, _, H, W = shape
    assert de.shape == grad.shape == (N, H, W) and de_mean.shape == (N,) and de_mean.dtype == torch.float64
    np.testing.assert_allclose(de.double().cpu().numpy(), de_ref.numpy(), atol=5e-4, rtol=1e-4)
    # the Sobel magnitude: the existing two-kernel path sets the error scale
    err_old = (_unfused_grad(pa.clamp(0.0, 1.0).contiguous()).double().cpu() - grad_ref).abs().max().item()
    err_new = (grad.double().cpu() - grad_ref).abs().max().item()
    print(f"sobel {shape} spill={spill}: unfused max-abs error {err_old:.3e}, fused {err_new:.3e}")
    assert err_old > 0.0 or err_new == 0.0
    assert err_new <= 2.0 * err_old, (err_new, err_old)
    # float64 reductions against float64 sums of the kernel's own maps
    de_h, grad_h = de.double().cpu().view(N, -1), grad.cpu().view(N, -1)
    np.testing.assert_allclose(de_mean.cpu().numpy(), de_h.mean(dim=1).numpy(), rtol=1e-10, atol=0.0)
    thr = quantile_rows(grad.view(N, -1), 0.85)
    m = masked_mean(de.view(N, -1), grad.view(N, -1), thr)
    mask = grad_h >= thr.cpu().view(N, 1)
    assert m["count"].dtype == torch.int64 and m["sum"].dtype == torch.float64
    assert torch.equal(m["count"].cpu(), mask.sum(dim=1))
    assert int(m["pooled_count"].item()) == int(mask.sum())
    np.testing.assert_allclose(m["sum"].cpu().numpy(), (de_h * mask).sum(dim=1).numpy(), rtol=1e-10, atol=0.0)
    np.testing.assert_allclose(m["pooled_sum"].item(), de_h[mask].sum().item(), rtol=1e-10, atol=0.0)
    return de, grad


@pytest.mark.parametrize("shape,seed", [((2, 3, 17, 23), 11), ((1, 3, 31, 29), 12)])
def test_color_maps_and_stats_against_oracle(dev, shape, seed):
    from lowlight_image_enhancement_amd.metrics.valstats import color_stats, quantile_rank
    a, b, de_ref, grad_ref, _ = _oracle(shape, seed, False)
    N = shape[0]
    # the mask must not hinge on an fp32 rounding: the two sorted Sobel values around the threshold lie well apart
    k_lo, k_hi, _ = quantile_rank(shape[2] * shape[3], 0.85)
    s = torch.sort(grad_ref.view(N, -1), dim=1).values
    gap = (s[:, k_hi] - s[:, k_lo]).min().item()
    assert k_hi == k_lo + 1 and gap > 0.1, gap
    _check_maps(dev, shape, seed, False)
    st = color_stats(a.to(dev), b.to(dev), q=0.85, want_p95=True)
    for v in st.values():
        assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
    flat = de_ref.view(N, -1)
    assert abs(st["mean"].item() - flat.mean(1).mean().item()) < 1e-4
    assert abs(st["p95"].item() - torch.quantile(flat.reshape(-1), 0.95).item()) < 1e-3
    thr = torch.quantile(grad_ref.view(N, -1), 0.85, dim=1, keepdim=True)
    edge = flat[grad_ref.view(N, -1) >= thr].mean().item()
    assert abs(st["edge_mean"].item() - edge) < 2e-3 * edge
    assert "p95" not in color_stats(a.to(dev), b.to(dev))


@pytest.mark.parametrize("shape", [(1, 3, 1, 40), (1, 3, 40, 1), (1, 3, 3, 3), (2, 3, 33, 65)])
def test_color_maps_degenerate_geometry(dev, shape):
    _check_maps(dev, shape, 20 + sum(shape), False)


def test_color_maps_clamp_values_outside_unit_range(dev):
    from lowlight_image_enhancement_amd.metrics.valstats import color_maps
    shape = (2, 3, 33, 65)
    a, b, _, _, _ = _oracle(shape, 31, True)
    assert (a < 0).any() and (a > 1).any() and (b < 0).any() and (b > 1).any()
    de, grad = _check_maps(dev, shape, 31, True)
    # clamp=True on raw inputs is the unclamped kernel on clamped inputs, bit for bit
    de2, grad2, _ = color_maps(a.to(dev).clamp(0.0, 1.0), b.to(dev).clamp(0.0, 1.0), clamp=False)
    assert torch.equal(de, de2) and torch.equal(grad, grad2)


def test_color_stats_validates_inputs(dev):
    from lowlight_image_enhancement_amd.metrics.valstats import color_stats
    a, b = _rgb_pair((1, 3, 8, 8), 1, spill=False)
    with pytest.raises(ValueError):
        color_stats(a[:, :2].to(dev), b[:, :2].to(dev))
    with pytest.raises(ValueError):
        color_stats(a.to(dev), b[..., :4].to(dev))
    with pytest.raises(TypeError):
        color_stats(a.numpy(), b)
    with pytest.raises(ValueError):
        color_stats(a.to(dev), b.to(dev), q=1.0)
    st = color_stats(a[0].to(dev), b[0].to(dev))  # [C,H,W] accepted
    assert torch.isfinite(st["mean"]) and torch.isfinite(st["edge_mean"])
