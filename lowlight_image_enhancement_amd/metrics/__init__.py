"""metrics API subset on the hot path (reference: metrics/)."""

_NIQE = ("calculate_niqe", "niqe_features", "niqe_tensor", "register_niqe_metric")
_CHANNELWISE = ("rgb_psnr", "cpsnr_rgb", "rgb_ssim", "channel_stats", "register_channelwise_metrics")
__all__ = list(_NIQE + _CHANNELWISE + ("lpips_srgb", "psnr_ssim"))


def __getattr__(name):  # imported on first use
    if name == "psnr_ssim":  # reference: basicsr/metrics/psnr_ssim.py; the module, since its calculate_psnr and
        import importlib     # calculate_ssim are not those of metrics.psnr / metrics.ssim
        return importlib.import_module(".psnr_ssim", __name__)
    if name in _NIQE:  # NIQE (reference: basicsr/metrics/niqe.py)
        from . import niqe
        return getattr(niqe, name)
    if name in _CHANNELWISE:  # reference: metrics/channelwise.py
        from . import channelwise
        return getattr(channelwise, name)
    if name == "lpips_srgb":  # reference: metrics/perceptual.py
        from . import perceptual
        return perceptual.lpips_srgb
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
