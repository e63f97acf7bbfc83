"""Random erasing (Zhong et al.; ``torchvision.transforms.RandomErasing(p, scale, ratio, value=0)``):
per sample, with probability p, one random rectangle of the normalised image is set to 0, which in
normalised space is the mean colour. It runs on the finished batch right after it reaches the
device and before mixup / CutMix, torchvision's order (per-sample transforms, then the mixing).

* :func:`batch_key`, :func:`draw_erase` -- the boxes of a batch, a pure function of (seed, rank,
  epoch, step, position in the batch), in Python float64: the host mirror of the device draw
  (``csrc/erase.hip`` ``erase_draw_kernel``).
* :func:`erase_torch` -- the erase by slice assignment, both model-ready layouts.
* :class:`BatchEraser` -- two launches (draw, erase) into a persistent box table on a GPU batch of
  the native engine's layouts, ``draw_erase`` + ``erase_torch`` elsewhere; the same boxes either way.

The draw follows torchvision with the arithmetic in float64, as the crop draw of the packed data
path does (its float32 ``uniform_`` / ``exp`` are deliberately not reproduced). ``value="random"``
(per-pixel normal noise) is not offered.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

__all__ = ["batch_key", "draw_erase", "erase_torch", "BatchEraser", "SCALE", "RATIO", "ATTEMPTS"]

SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)     # torchvision's defaults (ops.native_ops ERASE_SCALE / ERASE_RATIO)
ATTEMPTS = 10
_STREAM = 0x455241            # "ERA": keeps these draws apart from every other (seed, ...) stream
_M32 = 0xFFFFFFFF


def _hash32(x: int) -> int:
    """lowbias32 (csrc/common.h hash32, data/synthetic.py) on a Python int."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def batch_key(seed: int, rank: int, epoch: int, step: int) -> int:
    """The uint32 key of one batch's draws: four nested hashes, so changing any one of the four
    arguments changes every box. Computed on the host and handed to the kernel."""
    k = _hash32(int(seed) * 97 + _STREAM)
    for v in (rank, epoch, step):
        k = _hash32(k ^ (int(v) & _M32))
    return k


def _uniform(skey: int, k: int) -> float:
    return _hash32(skey ^ (((k + 1) * 0x27D4EB2F) & _M32)) / 4294967296.0       # exact in float64


def draw_erase(seed: int, rank: int, epoch: int, step: int, B: int, S: int, p: float,
               scale=SCALE, ratio=RATIO) -> np.ndarray:
    """The erase boxes of one batch: int32 ``[B, 4]`` rows ``(y1, y2, x1, x2)``, rows and columns
    half-open, all zeros where the sample is left alone.

    Sample b draws from ``skey = hash32(batch_key ^ (b*0x9E3779B9 + 0x85EBCA6B))`` with
    ``u(k) = hash32(skey ^ (k+1)*0x27D4EB2F) / 2^32``: it is erased if ``u(0) < p``; attempt a of
    ten takes ``area = S*S*(s0 + (s1-s0)*u(1+4a))``, ``ar = exp(l0 + (l1-l0)*u(2+4a))`` with the
    logarithms of the ratio bounds, ``h = round(sqrt(area*ar))``, ``w = round(sqrt(area/ar))``
    (half to even) and is accepted when ``h < S and w < S`` (strict, as torchvision; h or w of 0
    gives an empty box), at ``i = int(u(3+4a)*(S-h+1))``, ``j = int(u(4+4a)*(S-w+1))``. Ten
    refusals leave the image alone, as torchvision does.

    The key of a sample is its POSITION IN THE BATCH, not its dataset id: the trainer does not see
    sample ids on every data path. The draw is still a pure function of (seed, rank, epoch, step,
    b), so a resumed run reproduces its boxes and DDP ranks draw different ones; DataParallel
    erases the global batch once, before the scatter."""
    from .ops.native_ops import erase_bounds
    p, s0, s1, l0, l1 = erase_bounds(p, scale, ratio)
    B, S = int(B), int(S)
    if B < 1 or S < 1:
        raise ValueError(f"draw_erase: batch {B} and image side {S} must be >= 1")
    bkey = batch_key(seed, rank, epoch, step)
    boxes = np.zeros((B, 4), dtype=np.int32)
    full = float(S) * float(S)
    for b in range(B):
        skey = _hash32(bkey ^ ((b * 0x9E3779B9 + 0x85EBCA6B) & _M32))
        if not _uniform(skey, 0) < p:
            continue
        for a in range(ATTEMPTS):
            area = full * (s0 + (s1 - s0) * _uniform(skey, 1 + 4 * a))
            ar = math.exp(l0 + (l1 - l0) * _uniform(skey, 2 + 4 * a))
            # area / ar overflows to inf for absurd bounds (the device's IEEE division): a refusal
            fh, fw = math.sqrt(area * ar), math.sqrt(area / ar) if ar > 0 else math.inf
            if not (math.isfinite(fh) and math.isfinite(fw)):
                continue
            h, w = round(fh), round(fw)
            if h < S and w < S:
                i = int(_uniform(skey, 3 + 4 * a) * (S - h + 1))
                j = int(_uniform(skey, 4 + 4 * a) * (S - w + 1))
                boxes[b] = (i, i + h, j, j + w)
                break
    return boxes


def erase_torch(x: torch.Tensor, boxes, layout: int) -> None:
    """``batch_erase`` in plain torch (CPU, torch engine), in place: slice assignment of +0.0 to
    the box of every sample, clamped to the image as the kernel clamps it. ``layout`` 1: NCHW
    ``[B, 3, S, S]``; 0: s2d ``[B, S/2, S/2, 16]`` through the view ``[B, i, j, p, q, c]`` = pixel
    ``(2i+p, 2j+q, c)`` of slots 0..11 (the view arithmetic of ``mix.mix_torch``; slots 12..15 are
    not touched), one assignment per row / column parity."""
    boxes = np.asarray(boxes.cpu() if isinstance(boxes, torch.Tensor) else boxes)
    B = x.shape[0]
    if boxes.shape != (B, 4):
        raise ValueError(f"erase_torch: boxes {boxes.shape} for a batch of {B}")
    S = x.shape[2] * (2 if layout == 0 else 1)
    v = x[..., :12].unflatten(-1, (2, 2, 3)) if layout == 0 else None
    for b, (y1, y2, x1, x2) in enumerate(boxes.tolist()):
        y1, y2, x1, x2 = max(y1, 0), min(y2, S), max(x1, 0), min(x2, S)
        if y1 >= y2 or x1 >= x2:
            continue
        if layout == 1:
            x[b, :, y1:y2, x1:x2] = 0.0
            continue
        for pp in range(2):          # rows 2i+pp in [y1, y2): i in [ceil((y1-pp)/2), ceil((y2-pp)/2))
            for q in range(2):
                v[b, (y1 - pp + 1) // 2:(y2 - pp + 1) // 2, (x1 - q + 1) // 2:(x2 - q + 1) // 2, pp, q] = 0.0


class BatchEraser:
    """``eraser(samples, epoch, step) -> samples``: random erasing of a finished batch, in place
    (every loader hands out a freshly made batch per step), with one :func:`draw_erase` box per
    sample keyed by its position in the batch. On a GPU batch of the native engine's layouts (s2d
    of any model dtype, NCHW f32) it is two launches, the draw into a persistent ``[B, 4]`` int32
    table (reallocated only when B or the device changes) and the erase: no host sync, no other
    allocation. Elsewhere :func:`draw_erase` + :func:`erase_torch`. Both produce the same boxes."""

    def __init__(self, cfg, ctx, scale=SCALE, ratio=RATIO) -> None:
        self.seed, self.rank = int(cfg.seed), int(getattr(ctx, "rank", 0))
        self.p, self.S = float(cfg.random_erase), int(cfg.image_size)
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.native = getattr(ctx, "engine", "torch") == "native"
        self.table: Optional[torch.Tensor] = None

    def _table(self, x: torch.Tensor) -> torch.Tensor:
        t = self.table
        if t is None or t.shape[0] != x.shape[0] or t.device != x.device:
            self.table = t = torch.empty(x.shape[0], 4, dtype=torch.int32, device=x.device)
        return t

    def __call__(self, samples: torch.Tensor, epoch: int, step: int) -> torch.Tensor:
        from .ops import native_ops as K
        found = K.batch_layout(samples)
        if found is None:
            raise ValueError(f"BatchEraser: batch {tuple(samples.shape)} is neither s2d "
                             f"[B, S/2, S/2, 16] nor NCHW [B, 3, S, S]")
        layout, S = found
        if S != self.S:
            raise ValueError(f"BatchEraser: batch of {S}x{S} images, draws made for {self.S}x{self.S}")
        samples = samples.contiguous()      # (a no-op on every loader's batch: erased in place)
        B = samples.shape[0]
        if samples.is_cuda and self.native and (layout == 0 or samples.dtype == torch.float32):
            table = self._table(samples)
            K.erase_draw(table, S, batch_key(self.seed, self.rank, epoch, step), self.p, self.scale,
                         self.ratio)
            K.batch_erase(samples, table, layout)
        else:
            erase_torch(samples, draw_erase(self.seed, self.rank, epoch, step, B, S, self.p, self.scale,
                                            self.ratio), layout)
        return samples
