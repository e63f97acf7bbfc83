"""float64 reference of global-norm gradient clipping (csrc/clip.hip, NativeSGD(clip_grad_norm=...)).

    norm  = inv * sqrt(sum over the ranges of g^2)            float64, rounded to float32 once
    coef  = min(1, max_norm / (norm + 1e-6))                  IEEE single precision, NaN kept
    scale = inv * coef                                        single precision: what the SGD multiplies g by

as ``torch.nn.utils.clip_grad_norm_`` computes them (its ``clamp(max=1)`` propagates a NaN; an infinite
norm gives 0), then the update of tests/optim_refs.py with ``scale`` in the place of ``inv``. Nothing
here imports the package. Checked against torch in tests/test_clip_refs_cpu.py.
"""
import numpy as np
import torch

import optim_refs as R

F64 = torch.float64
f32 = np.float32


def norm64(g, ranges) -> float:
    """sqrt of the float64 sum of squares of ``g`` (flat, any float dtype) over [(offset, numel)]."""
    g64 = g.to(F64)
    total = torch.zeros((), dtype=F64)
    for off, n in ranges:
        total = total + g64[off:off + n].pow(2).sum()
    return float(total.sqrt())


def norm32(g, ranges, inv=1.0) -> np.float32:
    """The unscaled norm as published: float32(float32(inv) * norm64)."""
    return f32(np.float64(f32(inv)) * np.float64(norm64(g, ranges)))


def coef32(norm, max_norm) -> np.float32:
    """min(1, max_norm / (norm + 1e-6)) in float32 arithmetic; NaN stays NaN."""
    with np.errstate(all="ignore"):
        c = f32(max_norm) / (f32(norm) + f32(1e-6))
    return c if np.isnan(c) or c <= f32(1.0) else f32(1.0)


def scale32(g, ranges, max_norm, inv=1.0, found_inf=False) -> np.float32:
    """float32(inv) * coef, or float32(inv) alone on a skipped step: out[1] of the kernel."""
    if found_inf:
        return f32(inv)
    with np.errstate(all="ignore"):
        return f32(inv) * coef32(norm32(g, ranges, inv), max_norm)


def clipped_sgd_ref(p, g, segments, hyper, steps: int, max_norm, inv=1.0, shadow_dtype=None):
    """:func:`optim_refs.seg_sgd_ref` on the clipped gradient: the norm runs over ``segments`` (the
    optimizer's tensors), and the float32 ``scale`` multiplies g where the unclipped update has
    ``inv`` -- in the LARS gradient norm as well, the order torch applies (unscale, clip, trust)."""
    return R.seg_sgd_ref(p, g, segments, hyper, steps, float(scale32(g, segments, max_norm, inv)),
                         shadow_dtype)
