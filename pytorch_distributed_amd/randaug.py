"""RandAugment (Cubuk et al.; ``torchvision.transforms.RandAugment(num_ops=n, magnitude=m,
num_magnitude_bins=31, interpolation=NEAREST)``) of a finished, normalised batch, per training
sample: right after the batch reaches the device, before the colour jitter, the random erasing and
mixup / CutMix.

A slot is one of a sample's n successive ops. It reads the whole sample, un-normalises each pixel as
the jitter does (``x01_c = clamp(x_c * STD_c + MEAN_c, 0, 1)``), applies its op, re-normalises and
rounds ONCE TO THE BATCH DTYPE into another buffer. With ``k = m`` and ``sgn = -1`` when the slot's
sign draw is below 0.5, else 1:

== ============ =====================================================================================
id op           what it does
== ============ =====================================================================================
0  Identity     nothing
1  ShearX       coefficients ``(1, s, 0, 0, 1, 0)``, ``s = sgn * (0.3 k / 30)`` (about the corner)
2  ShearY       ``(1, 0, 0, s, 1, 0)``
3  TranslateX   ``(1, 0, -t, 0, 1, 0)``, ``t = sgn * trunc(150 / 331 * S * k / 30)`` pixels
4  TranslateY   ``(1, 0, 0, 0, 1, -t)``
5  Rotate       ``a = sgn * radians(30 k / 30)``, ``c = cos a``, ``s = sin a``, ``h = S / 2``:
                ``(c, -s, h - c h + s h, s, c, h - s h - c h)``
6  Brightness   ``clamp(f x)``, ``f = 1 + sgn * (0.9 k / 30)`` (ops 6..9)
7  Color        ``clamp(f x + (1 - f) gray)``, ``gray = 0.2989 r + 0.587 g + 0.114 b``
8  Contrast     ``clamp(f x + (1 - f) m)``, m the mean of gray over the sample, summed in double
9  Sharpness    ``clamp(f x + (1 - f) blur)``; blur = the 3x3 sum with weights
                ``[[1, 1, 1], [1, 5, 1], [1, 1, 1]] / 13`` inside, x itself on the border; S <= 2: nothing
10 Posterize    ``q = floor(255 x + 0.5) & mask``, ``x = q / 255``; ``bits = 8 - round(k / 7.5)`` (half
                to even), ``mask = 0xFF & ~((1 << (8 - bits)) - 1)``
11 Solarize     ``x >= thr ? 1 - x : x``, ``thr = (255 - 255 k / 30) / 255``
12 AutoContrast per channel, lo / hi its min / max over the sample: unchanged when ``hi == lo``, else
                ``clamp((x - lo) * (1 / (hi - lo)))``
13 Equalize     per channel, hist of ``q = floor(255 x + 0.5)``: ``step = (S*S - hist[last non-empty
                bin]) // 255``; unchanged when 0, else ``x = min(255, (sum_{j<q} hist[j] + step // 2)
                // step) / 255``
== ============ =====================================================================================

A geometric op (1..5) copies STORED values and does not un-normalise: output pixel (y, x) with centre
``cx = x + 0.5, cy = y + 0.5`` takes source pixel ``(floor(a3 cx + a4 cy + a5), floor(a0 cx + a1 cy +
a2))``, evaluated in float32 as ``(a*cx + b*cy) + c``; a source outside the image gives the stored
value 0 (the mean colour) in all three channels. A slot of Identity, or a channel an op leaves
unchanged, keeps the bits of every element the clamp leaves alone (the jitter's rule).

* :func:`draw_randaug` -- the table of a batch, a pure function of (seed, rank, epoch, step, position
  in the batch), in Python float64: the host mirror of ``csrc/randaug.hip`` ``randaug_draw_kernel``.
* :func:`pack_table` / :func:`table_parts` -- the table's packing: int32 ``[B, n, 8]``, word 0 the op
  id, word 1 the bits of the float32 f / thr (the posterize mask as an integer), words 2..7 the bits
  of the float32 affine coefficients (0 for the other ops).
* :func:`randaug_torch` -- the definition in plain torch, both model-ready layouts.
* :class:`BatchRandAugment` -- the draw and a statistics and an apply launch per slot on a GPU batch
  of the native engine's layouts, ``draw_randaug`` + ``randaug_torch`` elsewhere.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .erase import _subkey, _uniform, batch_key as _batch_key

__all__ = ["batch_key", "draw_randaug", "pack_table", "table_parts", "randaug_torch", "BatchRandAugment",
           "OPS", "NUM_OPS", "rand_augment_args"]

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color",
       "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
NUM_OPS = len(OPS)
_STREAM = 0x524E44            # "RND": keeps these draws apart from every other (seed, ...) stream


def batch_key(seed: int, rank: int, epoch: int, step: int) -> int:
    """``erase.batch_key`` on RandAugment's own stream."""
    return _batch_key(seed, rank, epoch, step, _STREAM)


def rand_augment_args(nm) -> tuple:
    """``(n, m)`` validated: n in 0..4 (0 = off), m in 0..30."""
    if len(nm) != 2 or any(int(v) != v for v in nm) or not (0 <= nm[0] <= 4 and 0 <= nm[1] <= 30):
        raise ValueError(f"RandAugment takes (n, m), n ops in 0..4 (0 = off) of magnitude bin m in 0..30, "
                         f"got {nm!r}")
    return int(nm[0]), int(nm[1])


def pack_table(ops, params, coeffs) -> np.ndarray:
    """The int32 ``[B, n, 8]`` table of ``ops`` ``[B, n]``, ``params`` ``[B, n]`` (f or thr, rounded to
    float32; for Posterize rows the integer mask) and ``coeffs`` ``[B, n, 6]`` (rounded to float32;
    kept for the geometric rows only)."""
    ops = np.asarray(ops, dtype=np.int64)
    par, co = np.asarray(params, dtype=np.float64), np.asarray(coeffs, dtype=np.float64)
    if ops.ndim != 2 or par.shape != ops.shape or co.shape != ops.shape + (6,):
        raise ValueError(f"pack_table: ops {ops.shape}, params {par.shape} and coeffs {co.shape} must be "
                         f"[B, n], [B, n] and [B, n, 6]")
    table = np.zeros(ops.shape + (8,), dtype=np.int32)
    table[..., 0] = ops
    table[..., 1] = np.where(ops == 10, par.astype(np.int32), par.astype(np.float32).view(np.int32))
    geo = (ops >= 1) & (ops <= 5)
    table[..., 2:] = np.where(geo[..., None], co.astype(np.float32).view(np.int32), 0)
    return table


def table_parts(table):
    """``(ops int [B, n], params float32 [B, n] (the mask of a Posterize row as a number), coeffs
    float32 [B, n, 6])`` of a table."""
    t = np.ascontiguousarray(np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table,
                                        dtype=np.int32))
    if t.ndim != 3 or t.shape[2] != 8:
        raise ValueError(f"RandAugment table {t.shape} must be [B, n, 8]")
    ops = t[..., 0].astype(np.int64)
    par = np.where(ops == 10, t[..., 1].astype(np.float32), t[..., 1].copy().view(np.float32))
    return ops, par, t[..., 2:].copy().view(np.float32)


def draw_randaug(seed: int, rank: int, epoch: int, step: int, B: int, S: int, n: int, m: int) -> np.ndarray:
    """The RandAugment table of one batch (:func:`pack_table`'s packing). Sample b draws from ``skey =
    counter_subkey(batch_key, b)`` with ``u(k)`` as ``erase.draw_erase``; slot j takes ``op = int(u(2j) *
    14)`` and ``sgn = -1 if u(2j + 1) < 0.5 else 1``, so a slot's draw does not depend on n. The
    parameters are the module docstring's expressions, evaluated left to right in float64 and rounded
    once to float32; ``sin`` / ``cos`` are taken of the positive angle and the sine negated. As the
    erase's, the key of a sample is its position in the batch."""
    n, m = rand_augment_args((n, m))
    B, S = int(B), int(S)
    if B < 1 or S < 1 or n < 1:
        raise ValueError(f"draw_randaug: batch {B}, image side {S} and n {n} must be >= 1")
    bkey = batch_key(seed, rank, epoch, step)
    k, fS = float(m), float(S)
    a = (30.0 * k / 30.0) * (math.pi / 180.0)
    ca, sa = math.cos(a), math.sin(a)
    ops = np.zeros((B, n), dtype=np.int64)
    par, co = np.zeros((B, n)), np.zeros((B, n, 6))
    for b in range(B):
        skey = _subkey(bkey, b)
        for j in range(n):
            op = int(_uniform(skey, 2 * j) * float(NUM_OPS))
            sgn = -1.0 if _uniform(skey, 2 * j + 1) < 0.5 else 1.0
            c = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            if op == 1:
                c[1] = sgn * (0.3 * k / 30.0)
            elif op == 2:
                c[3] = sgn * (0.3 * k / 30.0)
            elif op == 3:
                c[2] = -(sgn * float(math.trunc(150.0 / 331.0 * fS * k / 30.0)))
            elif op == 4:
                c[5] = -(sgn * float(math.trunc(150.0 / 331.0 * fS * k / 30.0)))
            elif op == 5:
                cs, sn, h = ca, sgn * sa, 0.5 * fS
                c = [cs, -sn, h - cs * h + sn * h, sn, cs, h - sn * h - cs * h]
            elif 6 <= op <= 9:
                par[b, j] = 1.0 + sgn * (0.9 * k / 30.0)
            elif op == 10:
                par[b, j] = 0xFF & ~((1 << round(k / 7.5)) - 1)
            elif op == 11:
                par[b, j] = (255.0 - 255.0 * k / 30.0) / 255.0
            ops[b, j], co[b, j] = op, c
    return pack_table(ops, par, co)


def _clamp(v):
    return v.clamp(0.0, 1.0)


def _levels(img):
    return torch.floor(255.0 * img + 0.5).long()


def _slot_torch(stored, op, par, co, mean, std):
    """One slot on a sample's stored values ``[S, S, 3]`` (float32 or float64): the new stored values,
    not yet rounded to the batch dtype."""
    S, wt = stored.shape[0], stored.dtype
    if 1 <= op <= 5:
        a = [torch.tensor(float(v), dtype=torch.float32) for v in co]
        ctr = torch.arange(S, dtype=torch.float32) + 0.5
        cy, cx = ctr[:, None], ctr[None, :]
        u, v = torch.floor((a[0] * cx + a[1] * cy) + a[2]), torch.floor((a[3] * cx + a[4] * cy) + a[5])
        inside = (u >= 0) & (u < S) & (v >= 0) & (v < S)
        src = stored[v.clamp(0, S - 1).long(), u.clamp(0, S - 1).long()]
        return torch.where(inside[..., None], src, torch.zeros((), dtype=wt))
    raw = stored * std + mean
    img = _clamp(raw)
    f = torch.tensor(float(par), dtype=wt)
    keep = torch.zeros(3, dtype=torch.bool)          # channels the op leaves unchanged
    if op == 6:
        new = _clamp(f * img)
    elif op == 7:
        gray = 0.2989 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]
        new = _clamp(f * img + ((1.0 - f) * gray)[..., None])
    elif op == 8:
        gray = 0.2989 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]
        new = _clamp(f * img + (1.0 - f) * gray.double().mean().to(wt))     # the kernel's: summed in double
    elif op == 9 and S > 2:
        blur = img.clone()
        win = sum(img[1 + dy:S - 1 + dy, 1 + dx:S - 1 + dx] * (5.0 if dy == dx == 0 else 1.0)
                  for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        blur[1:-1, 1:-1] = win / 13.0
        new = _clamp(f * img + (1.0 - f) * blur)
    elif op == 10:
        new = (_levels(img) & int(par)).to(wt) / 255.0
    elif op == 11:
        new = torch.where(img >= f, 1.0 - img, img)
    elif op == 12:
        lo, hi = img.amin((0, 1)), img.amax((0, 1))
        keep = hi == lo
        new = _clamp((img - lo) * (1.0 / torch.where(keep, torch.ones_like(hi), hi - lo)))
    elif op == 13:
        q, new = _levels(img), img.clone()
        for c in range(3):
            hist = torch.bincount(q[..., c].flatten(), minlength=256)
            step = int(S * S - hist[hist.nonzero().max()]) // 255
            keep[c] = step == 0
            if step:
                lut = ((hist.cumsum(0) - hist + step // 2) // step).clamp(max=255)
                new[..., c] = lut[q[..., c]].to(wt) / 255.0
    else:
        keep[:] = True
        new = img
    out = (new - mean) / std
    same = torch.where(img == raw, stored, (img - mean) / std)   # an element off the clamp keeps its bits
    return torch.where(keep, same, out)


def randaug_torch(x: torch.Tensor, table, layout: int) -> torch.Tensor:
    """The chain of every sample's table rows in plain torch (CPU, torch engine), in float32 at least,
    each slot rounded to the dtype of ``x``; the result is written back into ``x``, which is returned.
    ``layout`` 1: NCHW ``[B, 3, S, S]``; 0: s2d ``[B, S/2, S/2, 16]`` (slots 12..15 are not touched)."""
    from .data.synthetic import MEAN, STD
    ops, par, co = table_parts(table)
    B = x.shape[0]
    if ops.shape[0] != B:
        raise ValueError(f"randaug_torch: a table of {ops.shape[0]} rows for a batch of {B}")
    wt = x.dtype if x.dtype == torch.float64 else torch.float32
    dev = x.device
    mean, std = torch.tensor(MEAN, dtype=wt), torch.tensor(STD, dtype=wt)
    h = x.shape[2]
    for b in range(B):
        if layout == 0:      # [i, j, p, q, c] -> [i, p, j, q, c] = pixel (2i+p, 2j+q)
            img = x[b, ..., :12].unflatten(-1, (2, 2, 3)).permute(0, 2, 1, 3, 4).reshape(2 * h, 2 * h, 3)
        else:
            img = x[b].permute(1, 2, 0)
        img = img.cpu()
        for j in range(ops.shape[1]):
            img = _slot_torch(img.to(wt), int(ops[b, j]), par[b, j], co[b, j], mean, std).to(x.dtype)
        if layout == 0:
            x[b, ..., :12] = img.reshape(h, 2, h, 2, 3).permute(0, 2, 1, 3, 4).reshape(h, h, 12).to(dev)
        else:
            x[b] = img.permute(2, 0, 1).to(dev)
    return x


class BatchRandAugment:
    """``aug(samples, epoch, step) -> samples``: RandAugment of a finished batch with one
    :func:`draw_randaug` row of n slots per sample, keyed by its position in the batch. On a GPU
    batch of the native engine's layouts (s2d of any model dtype, NCHW f32) it is ``2 n + 1``
    launches: the draw into a persistent int32 ``[B, n, 8]`` table, then per slot the statistics
    (histograms, min / max, gray sums into persistent tables and a slab) and the apply, slot 0 from
    the loader's batch into a persistent second buffer, slot 1 back, and so on; the tensor that
    holds the result is returned, the second buffer when n is odd. No host sync; the buffers are
    reallocated only when B, the dtype or the device changes. Elsewhere :func:`draw_randaug` +
    :func:`randaug_torch` on the batch itself. Both draw the same table."""

    def __init__(self, cfg, ctx) -> None:
        self.seed, self.rank = int(cfg.seed), int(getattr(ctx, "rank", 0))
        self.n, self.m = rand_augment_args(cfg.rand_augment)
        if self.n < 1:
            raise ValueError("BatchRandAugment: n = 0 is off: build none")
        self.S = int(cfg.image_size)
        self.native = getattr(ctx, "engine", "torch") == "native"
        self.table: Optional[torch.Tensor] = None
        self.stats: Optional[torch.Tensor] = None
        self.slab: Optional[torch.Tensor] = None
        self.buf: Optional[torch.Tensor] = None

    def _buffers(self, x: torch.Tensor, layout: int, S: int) -> None:
        from .ops import native_ops as K
        b = self.buf
        if b is None or b.shape != x.shape or b.dtype != x.dtype or b.device != x.device:
            B = x.shape[0]
            self.table = torch.empty(B, self.n, 8, dtype=torch.int32, device=x.device)
            self.stats = torch.empty(self.n * B * K.randaug_stat_row(), dtype=torch.int32, device=x.device)
            self.slab = torch.empty(B * K.randaug_bps(B, S, x.dtype, layout), dtype=torch.float64,
                                    device=x.device)
            self.buf = torch.empty_like(x)

    def __call__(self, samples: torch.Tensor, epoch: int, step: int) -> torch.Tensor:
        from .ops import native_ops as K
        found = K.batch_layout(samples)
        if found is None:
            raise ValueError(f"BatchRandAugment: batch {tuple(samples.shape)} is neither s2d "
                             f"[B, S/2, S/2, 16] nor NCHW [B, 3, S, S]")
        layout, S = found
        if S != self.S:
            raise ValueError(f"BatchRandAugment: batch of {S}x{S} images, the run's are {self.S}x{self.S}")
        samples = samples.contiguous()      # (a no-op on every loader's batch)
        if samples.is_cuda and self.native and (layout == 0 or samples.dtype == torch.float32):
            self._buffers(samples, layout, S)
            K.randaug_draw(self.table, self.stats, S, batch_key(self.seed, self.rank, epoch, step), self.m)
            src, dst = samples, self.buf
            for j in range(self.n):
                K.randaug_stats(src, self.table, j, self.stats, self.slab, layout)
                K.randaug_apply(src, dst, self.table, j, self.stats, self.slab, layout)
                src, dst = dst, src
            return src
        return randaug_torch(samples, draw_randaug(self.seed, self.rank, epoch, step, samples.shape[0], S,
                                                   self.n, self.m), layout)
