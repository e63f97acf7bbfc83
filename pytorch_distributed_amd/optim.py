"""Parameter groups and the pure-torch counterpart of the segmented native optimizer.

The native engine runs grouped SGD (per-group learning rate, momentum, weight decay, Nesterov and a
LARS trust ratio) as one segmented HIP kernel over its flat buffers (``csrc/optim.hip``,
:class:`~pytorch_distributed_amd.models.native.NativeSGD`). This module holds what both engines
share and what needs no GPU:

* :func:`build_param_groups` -- the usual ImageNet split: no weight decay on 1-D parameters (BatchNorm
  weight and bias, the fc bias), a trust ratio only on tensors with ``dim() >= 2``;
* :func:`normalize_param_groups` -- validation of torch-style group dicts (the refusals of NativeSGD);
* :class:`LARS` -- the same update in plain torch ops, used by the torch engine and on the CPU;
* :class:`LAMB` -- the plain-torch counterpart of the native AdamW / LAMB kernels
  (``csrc/adam.hip``, :class:`~pytorch_distributed_amd.models.native_train.NativeAdamW`); with
  ``lamb`` off its update is ``torch.optim.AdamW``'s, which the torch engine uses for ``adamw``.

The update, per parameter tensor with gradient ``g`` (already unscaled)::

    q    = trust * |p| / (|g| + wd * |p| + eps)   if trust > 0 and |p| > 0 and |g| > 0, else 1
    d    = q * (g + wd * p)
    b    = momentum * b + d                       (first step: b = d)
    p   -= lr * (d + momentum * b  if nesterov else  b)

With ``trust == 0`` this is ``torch.optim.SGD`` (dampening 0).

The adaptive update, per parameter tensor, with t the number of steps applied so far + 1::

    m  = b1 m + (1 - b1) g          v = b2 v + (1 - b2) g^2
    c1 = 1 / (1 - b1^t)             c2 = 1 / sqrt(1 - b2^t)
    a  = (m c1) / (sqrt(v) c2 + eps)
    AdamW:  p = p (1 - lr wd) - lr a
    LAMB :  u = a + wd p;  r = |p| / |u| if |p| > 0 and |u| > 0 else 1;  p = p - lr r u
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import torch

__all__ = ["build_param_groups", "normalize_param_groups", "LARS", "GROUP_KEYS", "LAMB",
           "ADAM_GROUP_KEYS", "check_adam_hyper"]

# keys a group may set; the rest of torch.optim.SGD's group keys are carried but must keep their
# defaults (they select other implementations of the same update, or updates not implemented here)
GROUP_KEYS = ("lr", "momentum", "weight_decay", "nesterov", "lars", "lars_eps")
_CARRIED = ("dampening", "maximize", "foreach", "differentiable", "fused", "initial_lr")
# the same for the adaptive optimizers (torch.optim.AdamW's group keys)
ADAM_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "lamb")
_ADAM_CARRIED = ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
                 "decoupled_weight_decay", "initial_lr")


def build_param_groups(model: torch.nn.Module, weight_decay: float, no_bn_decay: bool = False,
                       lars: float = 0.0, lamb: bool = False) -> List[dict]:
    """torch-style parameter groups of ``model``: tensors with ``dim() >= 2`` (conv and fc weights)
    keep ``weight_decay`` and get the trust coefficient ``lars`` (or, with ``lamb``, the LAMB trust
    ratio: ``lamb=True``); 1-D tensors (BatchNorm weight and bias, the fc bias) never get a trust
    ratio and, with ``no_bn_decay``, no weight decay. With none of the options the result is one
    group of every parameter."""
    if lars < 0:
        raise ValueError(f"lars must be >= 0, got {lars}")
    params = [p for p in model.parameters() if p.requires_grad]
    if lamb:
        if lars > 0:
            raise ValueError("lars and lamb are two trust ratios: pick one")
        g_m = {"params": [p for p in params if p.dim() >= 2], "weight_decay": weight_decay,
               "lamb": True}
        g_v = {"params": [p for p in params if p.dim() < 2],
               "weight_decay": 0.0 if no_bn_decay else weight_decay, "lamb": False}
        return [g for g in (g_m, g_v) if g["params"]]
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


def check_adam_hyper(h: dict, where: str = "") -> None:
    """The value rules of the adaptive optimizers (those of the launchers of ``csrc/adam.hip``)."""
    for k in ("lr", "eps", "weight_decay"):
        v = h[k]
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not v >= 0 or v == float("inf"):
            raise ValueError(f"{where}{k} must be a finite number >= 0, got {v!r}")
    betas = h["betas"]
    if (not isinstance(betas, (tuple, list)) or len(betas) != 2
            or not all(isinstance(b, (int, float)) and not isinstance(b, bool) and 0 <= b < 1
                       for b in betas)):
        raise ValueError(f"{where}betas must be two numbers in [0, 1), got {betas!r}")
    if h.get("amsgrad"):
        raise ValueError(f"{where}amsgrad is not implemented")


def normalize_param_groups(model_params: Iterable[torch.nn.Parameter],
                           param_groups: Optional[list], defaults: dict, keys=GROUP_KEYS,
                           carried=_CARRIED, check=check_hyper, who: str = "NativeSGD") -> List[dict]:
    """Validate torch-style ``param_groups`` against the parameters of one model and fill in
    ``defaults``. ``None`` means one group of every parameter. Parameters in no group are frozen
    (as with torch, where they are simply not handed to the optimizer). ValueError for: a
    parameter that is not the model's or that appears twice, an unknown key, a negative value,
    Nesterov without momentum, a dampening other than 0."""
    own = {id(p) for p in model_params}
    check(defaults, f"{who}: ")
    if param_groups is None:
        param_groups = [{"params": [p for p in model_params]}]
    if isinstance(param_groups, dict) or not isinstance(param_groups, (list, tuple)):
        raise ValueError("param_groups must be a list of dicts with a 'params' entry")
    seen, out = set(), []
    for gi, g in enumerate(param_groups):
        where = f"param_groups[{gi}]: "
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(where + "a group is a dict with a 'params' entry")
        unknown = set(g) - {"params"} - set(keys) - set(carried)
        if unknown:
            raise ValueError(where + f"unknown key(s) {sorted(unknown)}; known: {list(keys)}")
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
        for k in keys:
            ng.setdefault(k, defaults[k])
        for k in ("nesterov", "lamb"):
            if k in keys:
                ng[k] = bool(ng[k])
        check(ng, where)
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


class LAMB(torch.optim.Optimizer):
    """Adam moments with decoupled weight decay and, per parameter group, the LAMB layer-wise trust
    ratio, in plain torch ops (see the module docstring for the update). With ``lamb=False`` a
    group's update is ``torch.optim.AdamW``'s (amsgrad off). The norms are accumulated in float64
    and the ratio is rounded to the parameter's dtype once, like the native kernel's. The state has
    ``torch.optim.AdamW``'s format (``step``, ``exp_avg``, ``exp_avg_sq``)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 lamb=True) -> None:
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, lamb=bool(lamb))
        check_adam_hyper(defaults, "LAMB: ")
        super().__init__(params, defaults)
        for i, g in enumerate(self.param_groups):
            check_adam_hyper(g, f"LAMB: param_groups[{i}]: ")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for g in self.param_groups:
            lr, (b1, b2), eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                st["step"] += 1
                t = int(st["step"])
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.lerp_(p.grad, 1 - b1)
                v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
                c1, c2 = 1 / (1 - b1 ** t), 1 / (1 - b2 ** t) ** 0.5
                a = (m * c1).div_(v.sqrt().mul_(c2).add_(eps))
                if not g["lamb"]:
                    p.mul_(1 - lr * wd).add_(a, alpha=-lr)
                    continue
                u = a.add_(p, alpha=wd)
                wn, un = p.double().pow(2).sum().sqrt(), u.double().pow(2).sum().sqrt()
                r = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn)).to(p.dtype)
                p.add_(u * r, alpha=-lr)
        return loss
