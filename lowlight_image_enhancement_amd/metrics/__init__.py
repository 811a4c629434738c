"""metrics API subset on the hot path (reference: metrics/)."""

__all__ = ["calculate_niqe", "niqe_features", "niqe_tensor", "register_niqe_metric"]


def __getattr__(name):  # NIQE (reference: basicsr/metrics/niqe.py), imported on first use
    if name in __all__:
        from . import niqe
        return getattr(niqe, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
