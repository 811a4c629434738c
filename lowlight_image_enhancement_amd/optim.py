"""train.optim_g on the fused step: hyper-parameter specs of the optimizers the reference's setup_optimizers builds
(NAFNet_base/basicsr/models/image_restoration_model.py:112-142, lowlight_model.py:92-107): Adam, AdamW and SGD with
torch's keyword names.  A spec holds numbers only; the step itself is nbp_optim_prepare followed by nbp_adamw_apply,
nbp_adam_apply or nbp_sgd_apply over NBPTrainer's flat buffers (csrc/optim.hip, csrc/optim_apply.hip).

The defaults are read from the signatures of the installed torch.optim classes and the arguments are validated by
constructing that class once over a throw-away parameter, so the ValueErrors are torch's own.  `maximize=True` is not
implemented; `foreach` / `fused` / `capturable` / `differentiable` choose between torch implementations of one formula
and are accepted and ignored.
"""
from __future__ import annotations

import inspect
from typing import Any, Dict

import torch

_IGNORED = ("foreach", "fused", "capturable", "differentiable")


def _defaults(cls) -> Dict[str, Any]:
    sig = inspect.signature(cls.__init__)
    return {k: p.default for k, p in sig.parameters.items()
            if k not in ("self", "params") and p.default is not inspect.Parameter.empty}


class _Spec:
    """Keyword arguments of one torch.optim class, validated by it, kept as plain attributes."""
    torch_cls = None
    kind = ""

    def __init__(self, **kw):
        defaults = _defaults(self.torch_cls)
        unknown = [k for k in kw if k not in defaults]
        if unknown:  # what torch.optim.X(params, **kw) raises for them
            raise TypeError(f"{self.torch_cls.__name__}.__init__() got an unexpected keyword argument {unknown[0]!r}")
        args = dict(defaults)
        args.update(kw)
        for k in ("lr", "weight_decay"):
            if isinstance(args.get(k), torch.Tensor):
                raise TypeError(f"{k}: a Python number is required (the lr travels to the device once per step)")
        if args.get("maximize"):
            raise NotImplementedError(f"{self.torch_cls.__name__}(maximize=True) is not implemented on the fused step")
        check = {k: v for k, v in args.items() if k not in _IGNORED}
        self.torch_cls([torch.zeros(1, requires_grad=True)], **check)  # torch's own argument checks
        self.kwargs = args
        for k, v in args.items():
            setattr(self, k, v)

    def torch_kwargs(self) -> Dict[str, Any]:
        """The keyword arguments that give the same update in torch.optim (the ignored ones left at their defaults)."""
        return {k: v for k, v in self.kwargs.items() if k not in _IGNORED}

    def param_group(self) -> Dict[str, Any]:
        """param_groups[0] of this torch's optimizer.state_dict() for these arguments (without 'params')."""
        opt = self.torch_cls([torch.zeros(1, requires_grad=True)], **self.torch_kwargs())
        g = dict(opt.state_dict()["param_groups"][0])
        for k in _IGNORED:
            if k in g and k in self.kwargs:
                g[k] = self.kwargs[k]
        g.pop("params")
        return g

    def __repr__(self):
        shown = ", ".join(f"{k}={v!r}" for k, v in self.kwargs.items() if k not in _IGNORED and k != "maximize")
        return f"{type(self).__name__}({shown})"


class _AdamBase(_Spec):
    @property
    def plain_adamw(self) -> bool:
        """True for the update nbp_adamw_apply computes: decoupled decay, no amsgrad."""
        return self.decoupled and not self.amsgrad


class Adam(_AdamBase):
    """torch.optim.Adam: L2 weight decay (decoupled_weight_decay=True gives AdamW's), optional amsgrad."""
    torch_cls = torch.optim.Adam
    kind = "adam"

    @property
    def decoupled(self) -> bool:
        return bool(self.kwargs.get("decoupled_weight_decay", False))


class AdamW(_AdamBase):
    """torch.optim.AdamW: decoupled weight decay, optional amsgrad."""
    torch_cls = torch.optim.AdamW
    kind = "adam"
    decoupled = True


class SGD(_Spec):
    """torch.optim.SGD: momentum, dampening, nesterov, L2 weight decay."""
    torch_cls = torch.optim.SGD
    kind = "sgd"


def build_optimizer(optim_g: dict) -> _Spec:
    """setup_optimizers' dispatch (image_restoration_model.py:128-141): pops 'type' from the dict, as the reference
    does, and passes the rest to the class as keywords."""
    optim_type = optim_g.pop("type")
    if optim_type == "Adam":
        return Adam(**optim_g)
    if optim_type == "SGD":
        return SGD(**optim_g)
    if optim_type == "AdamW":
        return AdamW(**optim_g)
    raise NotImplementedError(f"optimizer {optim_type} is not supperted yet.")


__all__ = ["Adam", "AdamW", "SGD", "build_optimizer"]
