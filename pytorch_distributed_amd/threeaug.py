"""3-Augment (DeiT-III, Touvron et al.; timm's ``three_augment``) of a finished, normalised batch, per
training sample: after RandAugment, before the colour jitter, the random erasing and mixup / CutMix.
Each sample takes ONE of three ops, drawn uniformly:

== ========= ==========================================================================================
op what      on ``x01_c = clamp(x_c * STD_c + MEAN_c, 0, 1)`` (the jitter's un-normalisation)
== ========= ==========================================================================================
0  grayscale all three channels become ``0.2989 r + 0.587 g + 0.114 b`` (``Grayscale(3)``)
1  solarize  ``x >= 128 / 255 ? 1 - x : x`` (``RandomSolarize(p=1)`` at PIL's default threshold)
2  blur      ``GaussianBlur(kernel_size=2R+1, sigma)``, sigma uniform in [0.1, 2]: separable, ``reflect``
             padding (index ``-k`` reads ``k``, ``S-1+k`` reads ``S-1-k``), ``out(y, x) = sum_dy w[|dy|]
             sum_dx w[|dx|] x01(refl(y+dy), refl(x+dx))`` over ``-R..R``, the horizontal pass first,
             ``w[d] = exp(-0.5 (d / sigma)^2) / sum``; a run uses R = 11 (kernel size 23)
== ========= ==========================================================================================

and is re-normalised, ``(y_c - MEAN_c) / STD_c``, with one rounding to the batch dtype. The s2d padding
slots keep their bits, validation is never augmented.

* :func:`draw_three_aug` -- the table of a batch, a pure function of (seed, rank, epoch, step, position
  in the batch), in numpy float64: the host mirror of ``csrc/threeaug.hip`` ``three_aug_draw_kernel``.
* :func:`three_aug_table` / :func:`table_parts` -- the packing: int32 ``[B, 16]`` rows ``(op,
  bits(sigma), R, 0, bits(w[0]) .. bits(w[11]))``, the weights float32 and 0 beyond R. The apply reads
  op, R and the weights only.
* :func:`three_aug_torch` -- the definition in plain torch, both model-ready layouts.
* :class:`BatchThreeAugment` -- the draw and the apply launch into a persistent table and second
  buffer on a GPU batch of the native engine's layouts, ``draw_three_aug`` + ``three_aug_torch``
  elsewhere; the same ops and weights either way.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .erase import _subkey, _uniform, batch_key as _batch_key

__all__ = ["batch_key", "blur_weights", "draw_three_aug", "three_aug_table", "table_parts", "three_aug_torch",
           "BatchThreeAugment", "GRAYSCALE", "SOLARIZE", "BLUR", "RMAX", "RADIUS"]

GRAYSCALE, SOLARIZE, BLUR = 0, 1, 2
RMAX = 11                     # csrc/threeaug.hip RMAX
RADIUS = 11                   # a training run's: GaussianBlur(kernel_size=23)
_STREAM = 0x334155            # "3AU": keeps these draws apart from every other (seed, ...) stream


def batch_key(seed: int, rank: int, epoch: int, step: int) -> int:
    """``erase.batch_key`` on the 3-Augment's own stream."""
    return _batch_key(seed, rank, epoch, step, _STREAM)


def blur_weights(sigma, R: int) -> np.ndarray:
    """float32 ``[12]``: ``w[d] = e[d] / (e[0] + 2 e[1] + .. + 2 e[R])``, ``e[d] = exp(-0.5 (d / s)^2)``
    with s the float32 ``sigma`` widened to double, all in double (the sum in ascending d), rounded
    once; 0 beyond R."""
    if not 1 <= int(R) <= RMAX:
        raise ValueError(f"blur_weights: radius {R!r} outside 1..{RMAX}")
    s = np.float64(np.float32(sigma))
    q = np.arange(RMAX + 1, dtype=np.float64) / s
    e = np.where(np.arange(RMAX + 1) <= R, np.exp(-0.5 * (q * q)), 0.0)
    total = e[0]
    for d in range(1, RMAX + 1):
        total = total + 2.0 * e[d]
    return (e / total).astype(np.float32)


def three_aug_table(ops, sigmas, R: int) -> np.ndarray:
    """The int32 ``[B, 16]`` table of ``ops`` ``[B]`` (0..2) and ``sigmas`` ``[B]`` (rounded to float32;
    read by the blur rows' weights only) at radius ``R``."""
    ops = np.asarray(ops, dtype=np.int64)
    sig = np.ascontiguousarray(np.asarray(sigmas, dtype=np.float32))
    if ops.ndim != 1 or sig.shape != ops.shape or ((ops < 0) | (ops > 2)).any():
        raise ValueError(f"three_aug_table: ops {ops.shape} (0..2) and sigmas {sig.shape} must both be [B]")
    if not (sig > 0).all():
        raise ValueError("three_aug_table: sigma must be > 0")
    table = np.zeros((ops.shape[0], 16), dtype=np.int32)
    table[:, 0], table[:, 1], table[:, 2] = ops, sig.view(np.int32), int(R)
    for b in range(ops.shape[0]):
        table[b, 4:] = blur_weights(sig[b], R).view(np.int32)
    return table


def table_parts(table):
    """``(ops int [B], R int [B], weights float32 [B, 12])`` of a table."""
    t = np.ascontiguousarray(np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table,
                                        dtype=np.int32))
    if t.ndim != 2 or t.shape[1] != 16:
        raise ValueError(f"3-Augment table {t.shape} must be [B, 16]")
    return t[:, 0].astype(np.int64), t[:, 2].astype(np.int64), t[:, 4:].copy().view(np.float32)


def draw_three_aug(seed: int, rank: int, epoch: int, step: int, B: int, R: int = RADIUS) -> np.ndarray:
    """The 3-Augment table of one batch (:func:`three_aug_table`'s packing). Sample n draws from
    ``skey = counter_subkey(batch_key, n)`` with ``u(k)`` as ``erase.draw_erase``: ``op = int(u(0) * 3)``,
    ``sigma = float32(0.1 + 1.9 * u(1))``. As the erase's, the key of a sample is its position in the
    batch."""
    B = int(B)
    if B < 1:
        raise ValueError(f"draw_three_aug: batch {B} must be >= 1")
    bkey = batch_key(seed, rank, epoch, step)
    ops, sigmas = np.empty(B, dtype=np.int64), np.empty(B, dtype=np.float64)
    for n in range(B):
        skey = _subkey(bkey, n)
        ops[n] = int(_uniform(skey, 0) * 3.0)
        sigmas[n] = 0.1 + 1.9 * _uniform(skey, 1)
    return three_aug_table(ops, sigmas, R)


def _reflect(n: int, R: int, device) -> torch.Tensor:
    """Source indices of positions ``-R .. n-1+R`` under torch's ``reflect`` padding."""
    i = torch.arange(-R, n + R, device=device)
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))


def three_aug_torch(x: torch.Tensor, table, layout: int) -> torch.Tensor:
    """``three_aug`` in plain torch (CPU, torch engine), in place, in the dtype of ``x`` and in float32
    at least; returns ``x``. ``layout`` 1: NCHW ``[B, 3, S, S]``; 0: s2d ``[B, S/2, S/2, 16]`` (slots
    12..15 are not touched)."""
    from .data.synthetic import MEAN, STD
    ops, radii, weights = table_parts(table)
    B = x.shape[0]
    if ops.shape[0] != B:
        raise ValueError(f"three_aug_torch: a table of {ops.shape[0]} rows for a batch of {B}")
    wt = x.dtype if x.dtype == torch.float64 else torch.float32
    mean, std = torch.tensor(MEAN, dtype=wt, device=x.device), torch.tensor(STD, dtype=wt, device=x.device)
    for b in range(B):
        if layout == 0:
            h = x.shape[1]
            img = x[b, ..., :12].reshape(h, h, 2, 2, 3).permute(0, 2, 1, 3, 4).reshape(2 * h, 2 * h, 3)
        else:
            img = x[b].movedim(0, -1)
        S, R = img.shape[0], int(radii[b])
        img = (img.to(wt) * std + mean).clamp(0.0, 1.0)
        if ops[b] == GRAYSCALE:
            gray = 0.2989 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]
            img = gray.unsqueeze(-1).expand(S, S, 3)
        elif ops[b] == SOLARIZE:
            img = torch.where(img >= 128.0 / 255.0, 1.0 - img, img)
        else:
            if not 1 <= R <= RMAX or R >= S:
                raise ValueError(f"three_aug_torch: sample {b}: radius {R} outside 1..{RMAX} or not below {S}")
            w = torch.tensor(weights[b], dtype=wt, device=x.device)
            idx = _reflect(S, R, x.device)
            hor = torch.zeros_like(img)
            for k in range(2 * R + 1):
                hor = hor + w[abs(k - R)] * img[:, idx[k:k + S]]
            img = torch.zeros_like(hor)
            for k in range(2 * R + 1):
                img = img + w[abs(k - R)] * hor[idx[k:k + S]]
        out = ((img - mean) / std).to(x.dtype)
        if layout == 0:
            h = x.shape[1]
            x[b, ..., :12] = out.reshape(h, 2, h, 2, 3).permute(0, 2, 1, 3, 4).reshape(h, h, 12)
        else:
            x[b] = out.movedim(-1, 0)
    return x


class BatchThreeAugment:
    """``aug(samples, epoch, step) -> samples``: 3-Augment of a finished batch with one
    :func:`draw_three_aug` row per sample, keyed by its position in the batch. On a GPU batch of the
    native engine's layouts (s2d of any model dtype, NCHW f32) it is two launches and no host sync:
    the draw into a persistent int32 ``[B, 16]`` table and the apply from the loader's batch into a
    persistent second buffer, which is returned (the blur reads a neighbourhood, so nothing runs in
    place); both are reallocated only when B, the dtype or the device changes. Elsewhere
    :func:`draw_three_aug` + :func:`three_aug_torch` on the batch itself. Both draw the same table."""

    def __init__(self, cfg, ctx) -> None:
        self.seed, self.rank = int(cfg.seed), int(getattr(ctx, "rank", 0))
        self.S, self.R = int(cfg.image_size), RADIUS
        if self.S < self.R + 1:
            raise ValueError(f"BatchThreeAugment: the {2 * self.R + 1}-tap blur reflects {self.R} pixels: "
                             f"image_size must be at least {self.R + 1}, got {self.S}")
        self.native = getattr(ctx, "engine", "torch") == "native"
        self.table: Optional[torch.Tensor] = None
        self.buf: Optional[torch.Tensor] = None

    def __call__(self, samples: torch.Tensor, epoch: int, step: int) -> torch.Tensor:
        from .ops import native_ops as K
        found = K.batch_layout(samples)
        if found is None:
            raise ValueError(f"BatchThreeAugment: batch {tuple(samples.shape)} is neither s2d "
                             f"[B, S/2, S/2, 16] nor NCHW [B, 3, S, S]")
        layout, S = found
        if S != self.S:
            raise ValueError(f"BatchThreeAugment: batch of {S}x{S} images, the run's are {self.S}x{self.S}")
        samples = samples.contiguous()      # (a no-op on every loader's batch)
        if samples.is_cuda and self.native and (layout == 0 or samples.dtype == torch.float32):
            b = self.buf
            if b is None or b.shape != samples.shape or b.dtype != samples.dtype or b.device != samples.device:
                self.table = torch.empty(samples.shape[0], 16, dtype=torch.int32, device=samples.device)
                self.buf = torch.empty_like(samples)
            K.three_aug_draw(self.table, batch_key(self.seed, self.rank, epoch, step), self.R)
            K.three_aug(samples, self.buf, self.table, layout, max_r=self.R)
            return self.buf
        return three_aug_torch(samples, draw_three_aug(self.seed, self.rank, epoch, step, samples.shape[0],
                                                       self.R), layout)
