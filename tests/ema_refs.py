"""Float64 references for the weight EMA (pytorch_distributed_amd/ema.py, csrc/ema.hip).

The kernel and the torch fallback compute ``e <- e + w (p - e)`` in float32 with a float32 ``w``;
the references take that same ``w`` (a Python float holding a float32 value) and evaluate the
recurrence in float64 without intermediate rounding.

Error bound of one float32 update against the float64 value from the same float32 inputs: the
difference ``p - e`` is rounded once (<= u |p - e| <= u (|p| + |e|), u = 2^-24), and the fused
multiply-add rounds once more (<= u |e'| <= u max(|p|, |e|) as e' lies between e and p for w in
[0, 1]); an unfused evaluation adds the product's rounding (<= u w |p - e|). All three together stay
within ``3 u (|p| + |e|)``. Over several updates the errors add up: an error already in e is carried
with the factor (1 - w) <= 1.
"""
import numpy as np
import torch

F64 = torch.float64
U24 = 2.0 ** -24


def weight(decay: float, t: int, warmup: bool) -> float:
    """float32(1 - d), d = min(decay, (1 + t) / (10 + t)) with warmup (t updates applied so far)."""
    d = decay
    if warmup:
        d = min(decay, (1.0 + t) / (10.0 + t))
    return float(np.float32(1.0 - d))


def lerp64(e: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    e64, p64 = e.to(F64), p.to(F64)
    return e64 + w * (p64 - e64)


def lerp_bound(e_old: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """Per-element bound of one float32 update (see the module docstring)."""
    return 3 * U24 * (p.to(F64).abs() + e_old.to(F64).abs())


def run(e0: torch.Tensor, snapshots, decay: float, every: int = 1, warmup: bool = True):
    """The recurrence over per-step snapshots of p (one per optimizer step): an update on every
    ``every``-th step. Returns (e64, accumulated bound, updates applied, index of the last snapshot
    that was averaged or None)."""
    e = e0.to(F64).clone()
    bound = torch.zeros_like(e)
    n, last = 0, None
    for step, p in enumerate(snapshots, 1):
        if step % every:
            continue
        # the float32 e differs from this e by at most `bound`: its size enters the next bound
        bound = bound + 3 * U24 * (p.to(F64).abs() + e.abs() + bound)
        e = e + weight(decay, n, warmup) * (p.to(F64) - e)
        n, last = n + 1, step - 1
    return e, bound, n, last


def closed_form(e0: torch.Tensor, p: torch.Tensor, ws) -> torch.Tensor:
    """Constant p: e_n = p + (e_0 - p) prod_k (1 - w_k)."""
    keep = 1.0
    for w in ws:
        keep *= 1.0 - w
    return p.to(F64) + (e0.to(F64) - p.to(F64)) * keep


def copy(e: torch.Tensor, p: torch.Tensor):
    """EMA_COPY: (e, p) afterwards."""
    return p.clone(), p.clone()


def swap(e: torch.Tensor, p: torch.Tensor):
    """EMA_SWAP: (e, p) afterwards; the shadow is torch's cast of the new p."""
    return p.clone(), e.clone()
