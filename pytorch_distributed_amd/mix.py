"""Label smoothing, mixup and CutMix: the loss and data half of the large-batch ResNet-50 recipe
(He et al., "Bag of Tricks"; torchvision's reference training script).

* :func:`draw_mix` -- one (mode, lam, box) per batch, a pure function of (seed, rank, epoch, step).
* :class:`BatchMixer` -- mixes a finished batch with itself rolled by one sample: the HIP kernel
  (``csrc/mix.hip`` ``batch_mix``) on a GPU batch of the native engine's layouts, plain torch
  elsewhere.
* :class:`SoftCrossEntropy` -- the criterion of the torch engine and the CPU; the native engine's
  is :class:`~pytorch_distributed_amd.models.native.NativeCrossEntropy` (``xent_soft``).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import nn
import torch.nn.functional as F

__all__ = ["MIXUP", "CUTMIX", "draw_mix", "BatchMixer", "SoftCrossEntropy", "soft_cross_entropy",
           "mix_torch", "MIX_REFUSAL"]

MIXUP, CUTMIX = 0, 1          # ops.native_ops MIX_MIXUP / MIX_CUTMIX
_STREAM = 0x4D4958            # "MIX": keeps these draws apart from every other (seed, ...) stream

MIX_REFUSAL = ("{what} cannot run label smoothing, mixup or CutMix: captured steps (MX_GRAPH=1, the "
               "DataParallel replica graphs) bake their loss arguments in at capture and would train "
               "on hard labels. Run without MX_GRAPH / on one device (the single-GPU and DDP scripts "
               "work), or drop MX_LABEL_SMOOTHING / MX_MIXUP / MX_CUTMIX")


def draw_mix(seed: int, rank: int, epoch: int, step: int, S: int, mixup_alpha: float,
             cutmix_alpha: float) -> Tuple[Optional[int], float, Optional[Tuple[int, int, int, int]]]:
    """The batch's mixing draw: ``(mode, lam, box)``. A pure function of its arguments, so a
    resumed run and every rank reproduce their own draws. With both alphas > 0 the mode is picked
    with probability 1/2, then lam ~ Beta(alpha, alpha) of that mode. CutMix follows torchvision:
    centre uniform over the image, half sizes ``int(0.5 * sqrt(1-lam) * S)``, corners clamped to
    [0, S], and lam replaced by ``1 - area / S^2``. ``box`` = (y1, y2, x1, x2), rows and columns
    half-open. Both alphas 0: ``(None, 1.0, None)``."""
    if not (mixup_alpha >= 0 and cutmix_alpha >= 0):
        raise ValueError(f"mixup / cutmix alphas must be >= 0, got {mixup_alpha!r}, {cutmix_alpha!r}")
    if mixup_alpha == 0 and cutmix_alpha == 0:
        return None, 1.0, None
    rng = np.random.default_rng((int(seed), int(rank), int(epoch), int(step), _STREAM))
    if mixup_alpha > 0 and cutmix_alpha > 0:
        mode = CUTMIX if rng.random() < 0.5 else MIXUP
    else:
        mode = MIXUP if mixup_alpha > 0 else CUTMIX
    if mode == MIXUP:
        lam = float(rng.beta(mixup_alpha, mixup_alpha))
        return MIXUP, min(max(lam, 0.0), 1.0), None
    lam = min(max(float(rng.beta(cutmix_alpha, cutmix_alpha)), 0.0), 1.0)
    rx, ry = int(rng.integers(S)), int(rng.integers(S))
    r = 0.5 * math.sqrt(1.0 - lam)
    rw, rh = int(r * S), int(r * S)
    x1, y1 = max(rx - rw, 0), max(ry - rh, 0)
    x2, y2 = min(rx + rw, S), min(ry + rh, S)
    lam = 1.0 - (x2 - x1) * (y2 - y1) / (S * S)
    return CUTMIX, lam, (y1, y2, x1, x2)


def mix_torch(x: torch.Tensor, out: torch.Tensor, layout: int, mode: int, lam: float, box) -> None:
    """``batch_mix`` in plain torch (CPU, torch engine): roll by one sample, then the kernel's
    ``lam*x + (1-lam)*partner`` in f32 with the same float32 weights, rounded once (mixup), or a
    slice assignment of the box (CutMix)."""
    part = x.roll(1, 0)
    if mode == MIXUP:
        from .ops.native_ops import mix_weights
        lam32, oml32 = mix_weights(lam)
        out.copy_(x.float() * lam32 + part.float() * oml32)
        return
    out.copy_(x)
    y1, y2, x1, x2 = box
    if layout == 1:
        out[:, :, y1:y2, x1:x2] = part[:, :, y1:y2, x1:x2]
        return
    B, S2 = x.shape[0], x.shape[1]
    # [B, i, j, 16] -> pixels [B, i, p, j, q, c] = image [B, 2i+p, 2j+q, c] (slots 12..15: padding)
    def img(t):
        return t[..., :12].reshape(B, S2, S2, 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * S2, 2 * S2, 3)
    a, p = img(out).clone(), img(part)
    a[:, y1:y2, x1:x2] = p[:, y1:y2, x1:x2]
    out[..., :12] = a.reshape(B, S2, 2, S2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, S2, S2, 12)


class BatchMixer:
    """``mixer(samples, labels, epoch, step) -> (samples, labels, labels_b, lam)``: one
    :func:`draw_mix` per batch, applied to the whole batch against itself rolled by one sample
    (``labels_b = labels.roll(1, 0)``). Owns one output buffer, reallocated only when the batch's
    shape, dtype or device changes; the returned samples are that buffer until the next call."""

    def __init__(self, cfg, ctx, layout: Optional[int] = None) -> None:
        self.seed, self.rank = int(cfg.seed), int(getattr(ctx, "rank", 0))
        self.mixup, self.cutmix, self.S = float(cfg.mixup), float(cfg.cutmix), int(cfg.image_size)
        self.native = getattr(ctx, "engine", "torch") == "native"
        self.layout = layout
        self.out: Optional[torch.Tensor] = None

    def _buffer(self, x: torch.Tensor) -> torch.Tensor:
        o = self.out
        if o is None or o.shape != x.shape or o.dtype != x.dtype or o.device != x.device:
            self.out = o = torch.empty_like(x, memory_format=torch.contiguous_format)
        return o

    def __call__(self, samples: torch.Tensor, labels: torch.Tensor, epoch: int, step: int):
        mode, lam, box = draw_mix(self.seed, self.rank, epoch, step, self.S, self.mixup, self.cutmix)
        if mode is None:
            return samples, labels, None, 1.0
        from .ops import native_ops as K
        found = K.batch_layout(samples)
        if found is None or self.layout not in (None, found[0]):
            raise ValueError(f"BatchMixer: batch {tuple(samples.shape)} is neither s2d "
                             f"[B, S/2, S/2, 16] nor NCHW [B, 3, S, S]")
        layout, S = found
        if S != self.S:
            raise ValueError(f"BatchMixer: batch of {S}x{S} images, draws made for {self.S}x{self.S}")
        samples = samples.contiguous()
        out = self._buffer(samples)
        if samples.is_cuda and self.native and (layout == 0 or samples.dtype == torch.float32):
            K.batch_mix(samples, out, layout, mode, lam, box)
        else:
            mix_torch(samples, out, layout, mode, lam, box)
        return out, labels, labels.roll(1, 0), lam


def soft_cross_entropy(logits, labels, labels_b=None, lam: float = 1.0, eps: float = 0.0):
    loss = F.cross_entropy(logits, labels, label_smoothing=eps)
    if labels_b is None:
        return loss
    return lam * loss + (1.0 - lam) * F.cross_entropy(logits, labels_b, label_smoothing=eps)


class SoftCrossEntropy(nn.Module):
    """``lam * CE(x, a) + (1-lam) * CE(x, b)``, both with label smoothing (mean over the batch):
    the criterion of the torch engine and the CPU."""

    soft_targets = True      # forward takes (logits, labels, labels_b, lam): trainer.build_criterion

    def __init__(self, label_smoothing: float = 0.0) -> None:
        super().__init__()
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}")
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits, labels, labels_b=None, lam: float = 1.0):
        return soft_cross_entropy(logits, labels, labels_b, lam, self.label_smoothing)
