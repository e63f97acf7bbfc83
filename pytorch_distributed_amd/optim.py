"""Parameter groups and the pure-torch counterpart of the segmented native optimizer.

The native engine runs grouped SGD (per-group learning rate, momentum, weight decay, Nesterov and a
LARS trust ratio) as one segmented HIP kernel over its flat buffers (``csrc/optim.hip``,
:class:`~pytorch_distributed_amd.models.native.NativeSGD`). This module holds what both engines
share and what needs no GPU:

* :func:`build_param_groups` -- the usual ImageNet split: no weight decay on 1-D parameters (BatchNorm
  weight and bias, the fc bias), a trust ratio only on tensors with ``dim() >= 2``;
* :func:`normalize_param_groups` -- validation of torch-style group dicts (the refusals of NativeSGD);
* :class:`LARS` -- the same update in plain torch ops, used by the torch engine and on the CPU.

The update, per parameter tensor with gradient ``g`` (already unscaled)::

    q    = trust * |p| / (|g| + wd * |p| + eps)   if trust > 0 and |p| > 0 and |g| > 0, else 1
    d    = q * (g + wd * p)
    b    = momentum * b + d                       (first step: b = d)
    p   -= lr * (d + momentum * b  if nesterov else  b)

With ``trust == 0`` this is ``torch.optim.SGD`` (dampening 0).
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

__all__ = ["build_param_groups", "normalize_param_groups", "LARS", "GROUP_KEYS"]

# keys a group may set; the rest of torch.optim.SGD's group keys are carried but must keep their
# defaults (they select other implementations of the same update, or updates not implemented here)
GROUP_KEYS = ("lr", "momentum", "weight_decay", "nesterov", "lars", "lars_eps")
_CARRIED = ("dampening", "maximize", "foreach", "differentiable", "fused", "initial_lr")


def build_param_groups(model: torch.nn.Module, weight_decay: float, no_bn_decay: bool = False,
                       lars: float = 0.0) -> List[dict]:
    """torch-style parameter groups of ``model``: tensors with ``dim() >= 2`` (conv and fc weights)
    keep ``weight_decay`` and get the trust coefficient ``lars``; 1-D tensors (BatchNorm weight and
    bias, the fc bias) never get a trust ratio and, with ``no_bn_decay``, no weight decay. With
    neither option the result is one group of every parameter."""
    if lars < 0:
        raise ValueError(f"lars must be >= 0, got {lars}")
    params = [p for p in model.parameters() if p.requires_grad]
    if not no_bn_decay and not lars > 0:
        return [{"params": params, "weight_decay": weight_decay}]
    mats = [p for p in params if p.dim() >= 2]
    vecs = [p for p in params if p.dim() < 2]
    g_m = {"params": mats, "weight_decay": weight_decay}
    g_v = {"params": vecs, "weight_decay": 0.0 if no_bn_decay else weight_decay}
    if lars > 0:
        g_m["lars"] = float(lars)
        g_v["lars"] = 0.0
    return [g for g in (g_m, g_v) if g["params"]]


def check_hyper(h: dict, where: str = "") -> None:
    """The value rules shared by every implementation of the update."""
    for k in ("lr", "momentum", "weight_decay", "lars", "lars_eps"):
        v = h.get(k, 0.0)
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not v >= 0 or v == float("inf"):
            raise ValueError(f"{where}{k} must be a finite number >= 0, got {v!r}")
    if h.get("nesterov", False) and not h.get("momentum", 0.0) > 0:
        raise ValueError(f"{where}nesterov needs momentum > 0 (torch.optim.SGD's rule)")
    if h.get("dampening", 0.0) != 0:
        raise ValueError(f"{where}dampening must be 0, got {h['dampening']!r}")


def normalize_param_groups(model_params: Iterable[torch.nn.Parameter],
                           param_groups: Optional[list], defaults: dict) -> List[dict]:
    """Validate torch-style ``param_groups`` against the parameters of one model and fill in
    ``defaults``. ``None`` means one group of every parameter. Parameters in no group are frozen
    (as with torch, where they are simply not handed to the optimizer). ValueError for: a
    parameter that is not the model's or that appears twice, an unknown key, a negative value,
    Nesterov without momentum, a dampening other than 0."""
    own = {id(p) for p in model_params}
    check_hyper(defaults, "NativeSGD: ")
    if param_groups is None:
        param_groups = [{"params": [p for p in model_params]}]
    if isinstance(param_groups, dict) or not isinstance(param_groups, (list, tuple)):
        raise ValueError("param_groups must be a list of dicts with a 'params' entry")
    seen, out = set(), []
    for gi, g in enumerate(param_groups):
        where = f"param_groups[{gi}]: "
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(where + "a group is a dict with a 'params' entry")
        unknown = set(g) - {"params"} - set(GROUP_KEYS) - set(_CARRIED)
        if unknown:
            raise ValueError(where + f"unknown key(s) {sorted(unknown)}; known: {list(GROUP_KEYS)}")
        ps = g["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        for p in ps:
            if id(p) not in own:
                raise ValueError(where + "holds a parameter that is not the model's")
            if id(p) in seen:
                raise ValueError(where + "holds a parameter that another group (or this one) "
                                 "already holds")
            seen.add(id(p))
        for k in ("maximize", "differentiable"):
            if g.get(k):
                raise ValueError(where + f"{k} is not implemented")
        ng = {k: v for k, v in g.items() if k != "params"}
        for k in GROUP_KEYS:
            ng.setdefault(k, defaults[k])
        ng["nesterov"] = bool(ng["nesterov"])
        check_hyper(ng, where)
        ng["params"] = ps
        out.append(ng)
    return out


class LARS(torch.optim.Optimizer):
    """SGD with momentum, optional Nesterov momentum and an optional layer-wise trust ratio (LARS),
    per parameter group, in plain torch ops (see the module docstring for the update). ``lars`` is
    the trust coefficient; 0 turns the ratio off, and the update is then ``torch.optim.SGD``'s.
    Norms are accumulated in float64 and the ratio is rounded to the parameter's dtype once, like
    the native kernel's."""

    def __init__(self, params, lr=0.1, momentum=0.0, weight_decay=0.0, nesterov=False, lars=0.0,
                 lars_eps=1e-8, dampening=0.0) -> None:
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=bool(nesterov),
                        lars=lars, lars_eps=lars_eps, dampening=dampening)
        check_hyper(defaults, "LARS: ")
        super().__init__(params, defaults)
        for i, g in enumerate(self.param_groups):
            check_hyper(g, f"LARS: param_groups[{i}]: ")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for g in self.param_groups:
            lr, mom, wd = g["lr"], g["momentum"], g["weight_decay"]
            trust, eps, nesterov = g["lars"], g["lars_eps"], g["nesterov"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                d = grad.add(p, alpha=wd) if wd != 0 else grad.clone()
                if trust > 0:
                    wn = p.double().pow(2).sum().sqrt()
                    gn = grad.double().pow(2).sum().sqrt()
                    q = torch.where((wn > 0) & (gn > 0), trust * wn / (gn + wd * wn + eps),
                                    torch.ones_like(wn))
                    d.mul_(q.to(d.dtype))
                if mom != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = d.clone()
                    else:
                        buf.mul_(mom).add_(d)
                    d = d.add(buf, alpha=mom) if nesterov else buf
                p.add_(d, alpha=-lr)
        return loss
