"""Colour jitter (``torchvision.transforms.ColorJitter(brightness, contrast, saturation, hue)``) of a
finished, normalised batch, per training sample: right after the batch reaches the device, before
random erasing and before mixup / CutMix (per-sample transforms, then the mixing).

For each sample, with its four factors and its op order from the draw, every pixel is

1. un-normalised: ``x01_c = clamp(x_c * STD_c + MEAN_c, 0, 1)`` (``data/synthetic.py``; the clamp is
   part of the definition: 16-bit rounding and the synthetic data leave values outside [0, 1]),
2. taken through the enabled ops in the sample's order, each the torchvision float-image formula
   with ``gray = 0.2989 r + 0.587 g + 0.114 b``: brightness ``clamp(f x)``, contrast
   ``clamp(f x + (1 - f) m)`` with m the mean of gray over the image as it stands when contrast is
   reached, saturation ``clamp(f x + (1 - f) gray)``, hue ``_rgb2hsv``, ``h = (h + f) mod 1``,
   ``_hsv2rgb``,
3. re-normalised, ``(y_c - MEAN_c) / STD_c``, and rounded once to the batch dtype.

An op of strength 0 is skipped, the s2d padding slots keep their bits, validation is never jittered.

* :func:`draw_jitter` -- the table of a batch, a pure function of (seed, rank, epoch, step, position
  in the batch), in Python float64: the host mirror of ``csrc/jitter.hip`` ``jitter_draw_kernel``.
* :func:`jitter_table` / :func:`table_parts` -- the table's packing: int32 ``[B, 5]`` rows = the bits
  of the float32 factors (brightness, contrast, saturation, hue) and the op order in nibbles.
* :func:`jitter_torch` -- the definition in plain torch, both model-ready layouts.
* :class:`BatchJitter` -- draw, mean (when contrast is on) and apply launches into a persistent table
  and slab on a GPU batch of the native engine's layouts, ``draw_jitter`` + ``jitter_torch``
  elsewhere; the same factors and orders either way.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .erase import _subkey, _uniform, batch_key as _batch_key

__all__ = ["batch_key", "draw_jitter", "jitter_table", "table_parts", "jitter_torch", "BatchJitter",
           "BRIGHTNESS", "CONTRAST", "SATURATION", "HUE", "SKIP"]

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
SKIP = 15                     # the nibble of an op that is not applied; -1 in an unpacked order
_STREAM = 0x4A4954            # "JIT": keeps these draws apart from every other (seed, ...) stream


def batch_key(seed: int, rank: int, epoch: int, step: int) -> int:
    """``erase.batch_key`` on the jitter's own stream."""
    return _batch_key(seed, rank, epoch, step, _STREAM)


def jitter_table(factors, orders) -> np.ndarray:
    """The int32 ``[B, 5]`` table of float ``factors`` ``[B, 4]`` (brightness, contrast, saturation,
    hue; rounded to float32) and ``orders`` ``[B, 4]``: the op at each position, -1 = none."""
    f = np.ascontiguousarray(np.asarray(factors, dtype=np.float32))
    o = np.asarray(orders, dtype=np.int64)
    if f.ndim != 2 or f.shape[1] != 4 or o.shape != f.shape:
        raise ValueError(f"jitter_table: factors {f.shape} and orders {o.shape} must both be [B, 4]")
    if ((o < -1) | (o > 3)).any():
        raise ValueError("jitter_table: an order holds ops 0..3 or -1 (none)")
    nib = np.where(o < 0, SKIP, o)
    table = np.empty((f.shape[0], 5), dtype=np.int32)
    table[:, :4] = f.view(np.int32)
    table[:, 4] = nib[:, 0] | nib[:, 1] << 4 | nib[:, 2] << 8 | nib[:, 3] << 12
    return table


def table_parts(table):
    """``(factors float32 [B, 4], orders int [B, 4])`` of a table; nibbles above 3 read -1."""
    t = np.ascontiguousarray(np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table,
                                        dtype=np.int32))
    if t.ndim != 2 or t.shape[1] != 5:
        raise ValueError(f"jitter table {t.shape} must be [B, 5]")
    nib = (t[:, 4:5].astype(np.int64) >> (4 * np.arange(4))) & 15
    return t[:, :4].copy().view(np.float32), np.where(nib > 3, -1, nib)


def draw_jitter(seed: int, rank: int, epoch: int, step: int, B: int, strengths) -> np.ndarray:
    """The jitter table of one batch (:func:`jitter_table`'s packing). Every sample draws:
    ``ColorJitter`` has no probability of applying.

    Sample n draws from ``skey = counter_subkey(batch_key, n)`` with ``u(k)`` as ``erase.draw_erase``:
    the order is a Fisher-Yates permutation of (brightness, contrast, saturation, hue), for
    ``i = 3, 2, 1``: ``j = int(u(3 - i) * (i + 1))``, swap positions i and j; ``fb = lo + (hi - lo) *
    u(3)`` with ``[lo, hi] = [max(0, 1 - b), 1 + b]``, fc from ``u(4)`` and fs from ``u(5)`` alike,
    ``fh = -h + 2h * u(6)``, in float64 and rounded once to float32. An op of strength 0 keeps its
    place in the permutation and is marked skipped. As the erase's, the key of a sample is its
    position in the batch."""
    from .ops.native_ops import jitter_strengths
    strengths = jitter_strengths(strengths)
    B = int(B)
    if B < 1:
        raise ValueError(f"draw_jitter: batch {B} must be >= 1")
    bkey = batch_key(seed, rank, epoch, step)
    factors, orders = np.empty((B, 4), dtype=np.float64), np.empty((B, 4), dtype=np.int64)
    h = strengths[3]
    for n in range(B):
        skey = _subkey(bkey, n)
        perm = [0, 1, 2, 3]
        for i in (3, 2, 1):
            j = int(_uniform(skey, 3 - i) * (i + 1))
            perm[i], perm[j] = perm[j], perm[i]
        orders[n] = [-1 if strengths[op] == 0 else op for op in perm]
        for k in range(3):
            lo, hi = max(0.0, 1.0 - strengths[k]), 1.0 + strengths[k]
            factors[n, k] = lo + (hi - lo) * _uniform(skey, 3 + k)
        factors[n, 3] = -h + 2.0 * h * _uniform(skey, 6)
    return jitter_table(factors, orders)


def _clamp(v):
    return v.clamp(0.0, 1.0)


def _gray(img):
    return 0.2989 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]


def _hue(img, fh):
    """torchvision's ``_rgb2hsv``, ``h = (h + fh) mod 1``, ``_hsv2rgb`` on ``[..., 3]`` values in [0, 1]."""
    r, g, b = img.unbind(-1)
    maxc, minc = img.amax(-1), img.amin(-1)
    cr = maxc - minc
    eq = cr == 0
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    crd = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    h6 = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.fmod(h6 / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + fh, 1.0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.long() % 6
    v = maxc
    p, q, t = _clamp(v * (1.0 - s)), _clamp(v * (1.0 - f * s)), _clamp(v * (1.0 - (1.0 - f) * s))
    pick = lambda *six: torch.stack(six, -1).gather(-1, i.unsqueeze(-1)).squeeze(-1)
    return torch.stack((pick(v, q, p, p, t, v), pick(t, v, v, q, p, p), pick(p, p, t, v, v, q)), -1)


def jitter_torch(x: torch.Tensor, table, layout: int) -> None:
    """``batch_jitter`` in plain torch (CPU, torch engine), in place, in the dtype of ``x`` and in
    float32 at least. ``layout`` 1: NCHW ``[B, 3, S, S]``; 0: s2d ``[B, S/2, S/2, 16]`` through the
    view ``[B, i, j, p, q, c]`` of slots 0..11 (slots 12..15 are not touched). As the kernel, a sample
    with every op skipped keeps the stored value of each element the clamp leaves alone."""
    from .data.synthetic import MEAN, STD
    factors, orders = table_parts(table)
    B = x.shape[0]
    if factors.shape[0] != B:
        raise ValueError(f"jitter_torch: a table of {factors.shape[0]} rows for a batch of {B}")
    wt = x.dtype if x.dtype == torch.float64 else torch.float32
    mean, std = torch.tensor(MEAN, dtype=wt, device=x.device), torch.tensor(STD, dtype=wt, device=x.device)
    view = x[..., :12].unflatten(-1, (2, 2, 3)) if layout == 0 else x.movedim(1, -1)    # [B, ..., 3]
    for b in range(B):
        stored = view[b].to(wt)
        raw = stored * std + mean
        img = _clamp(raw)
        fb, fc, fs, fh = torch.tensor(factors[b], dtype=wt, device=x.device).unbind()
        ops = [int(op) for op in orders[b] if op >= 0]
        for op in ops:
            if op == BRIGHTNESS:
                img = _clamp(fb * img)
            elif op == CONTRAST:
                m = _gray(img).double().mean().to(wt)       # the kernel's: summed in double
                img = _clamp(fc * img + (1.0 - fc) * m)
            elif op == SATURATION:
                img = _clamp(fs * img + (1.0 - fs) * _gray(img).unsqueeze(-1))
            else:
                img = _hue(img, fh)
        out = (img - mean) / std
        if not ops:
            out = torch.where(img == raw, stored, out)
        view[b] = out.to(x.dtype)


class BatchJitter:
    """``jitter(samples, epoch, step) -> samples``: colour jitter of a finished batch, in place (every
    loader hands out a freshly made batch per step), with one :func:`draw_jitter` row per sample keyed
    by its position in the batch. On a GPU batch of the native engine's layouts (s2d of any model
    dtype, NCHW f32) it is the draw into a persistent int32 ``[B, 5]`` table, the mean pass into a
    persistent slab of doubles (only when contrast is on) and the apply: no host sync, no other
    allocation; table and slab are reallocated only when B or the device changes. Elsewhere
    :func:`draw_jitter` + :func:`jitter_torch`. Both draw the same factors and orders."""

    def __init__(self, cfg, ctx) -> None:
        from .ops.native_ops import jitter_strengths
        self.seed, self.rank = int(cfg.seed), int(getattr(ctx, "rank", 0))
        self.strengths, self.S = jitter_strengths(cfg.color_jitter), int(cfg.image_size)
        self.native = getattr(ctx, "engine", "torch") == "native"
        self.table: Optional[torch.Tensor] = None
        self.slab: Optional[torch.Tensor] = None

    def _buffers(self, x: torch.Tensor, layout: int, S: int):
        from .ops import native_ops as K
        t = self.table
        if t is None or t.shape[0] != x.shape[0] or t.device != x.device:
            B = x.shape[0]
            self.table = torch.empty(B, 5, dtype=torch.int32, device=x.device)
            self.slab = None
            if self.strengths[CONTRAST] > 0:
                self.slab = torch.empty(B * K.jitter_bps(B, S, x.dtype, layout), dtype=torch.float64,
                                        device=x.device)
        return self.table, self.slab

    def __call__(self, samples: torch.Tensor, epoch: int, step: int) -> torch.Tensor:
        from .ops import native_ops as K
        found = K.batch_layout(samples)
        if found is None:
            raise ValueError(f"BatchJitter: batch {tuple(samples.shape)} is neither s2d "
                             f"[B, S/2, S/2, 16] nor NCHW [B, 3, S, S]")
        layout, S = found
        if S != self.S:
            raise ValueError(f"BatchJitter: batch of {S}x{S} images, the run's are {self.S}x{self.S}")
        samples = samples.contiguous()      # (a no-op on every loader's batch: jittered in place)
        if samples.is_cuda and self.native and (layout == 0 or samples.dtype == torch.float32):
            table, slab = self._buffers(samples, layout, S)
            K.jitter_draw(table, batch_key(self.seed, self.rank, epoch, step), self.strengths)
            K.batch_jitter(samples, table, layout, slab)
        else:
            jitter_torch(samples, draw_jitter(self.seed, self.rank, epoch, step, samples.shape[0],
                                              self.strengths), layout)
        return samples
