"""Float64 Python reference of random erasing (csrc/erase.hip, pytorch_distributed_amd/erase.py):
the key chain, the box draw and the erase itself.

Nothing here uses a kernel of this project or imports ``pytorch_distributed_amd.erase``.
tests/test_erase_refs_cpu.py checks the package's host mirror against it, tests/test_erase_gpu.py
the kernels.

The draw of the sample at batch position ``b`` (all uint32 arithmetic):

    bkey = hash32(hash32(hash32(hash32(seed*97 + 0x455241) ^ rank) ^ epoch) ^ step)
    skey = hash32(bkey ^ (b*0x9E3779B9 + 0x85EBCA6B))
    u(k) = hash32(skey ^ ((k+1)*0x27D4EB2F)) / 2^32          (exact in float64)

The sample is erased if u(0) < p. Attempt a = 0..9 is ``torchvision.transforms.RandomErasing``'s
with ``uniform(a, b) = a + (b-a)*u`` and ``randint(0, n) = int(u*n)`` on fixed counters: u(1+4a) for
the area, u(2+4a) for the log-ratio, u(3+4a) for the row, u(4+4a) for the column; the first attempt
with h < S and w < S (strict) is taken, and ten refusals leave the image alone.

As in tests/packed_refs.py, the only step where a device ``exp`` (or ``math.exp`` here) can
legitimately change an integer is the rounding of ``sqrt(area*ar)`` / ``sqrt(area/ar)``: a sample is
FRAGILE when one of these values, in any attempt evaluated, lies within ``FRAGILE_EPS`` of k + 0.5.
Relative errors of a few ulp (1e-16) in exp move the roots by < 1e-11 at sides <= 32768, so 1e-6 is
generous; the tests assert that their grids hold NO fragile sample.
"""
import functools
import math

import numpy as np
import torch

from packed_refs import hash32

M32 = 0xFFFFFFFF
FRAGILE_EPS = 1e-6
SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)
S2D, NCHW = 0, 1


def batch_key(seed: int, rank: int, epoch: int, step: int) -> int:
    return hash32(hash32(hash32(hash32((seed * 97 + 0x455241) & M32) ^ (rank & M32)) ^ (epoch & M32))
                  ^ (step & M32))


def sample_key(bkey: int, b: int) -> int:
    return hash32(bkey ^ ((b * 0x9E3779B9 + 0x85EBCA6B) & M32))


def uniform(skey: int, k: int) -> float:
    return hash32(skey ^ (((k + 1) * 0x27D4EB2F) & M32)) / 4294967296.0


def _near_half(v: float) -> bool:
    return abs((v - math.floor(v)) - 0.5) <= FRAGILE_EPS


def draw(seed: int, rank: int, epoch: int, step: int, B: int, S: int, p: float, scale=SCALE,
         ratio=RATIO):
    """``(boxes int32 [B, 4] = (y1, y2, x1, x2) half-open, accepted [B], fragile [B])``: accepted is
    the attempt taken (0..9), -1 for a sample that failed the gate or all ten attempts (its row is
    all zeros)."""
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    bkey = batch_key(seed, rank, epoch, step)
    boxes = np.zeros((B, 4), dtype=np.int32)
    accepted, fragile = [-1] * B, [False] * B
    for b in range(B):
        skey = sample_key(bkey, b)
        if not uniform(skey, 0) < p:
            continue
        for a in range(10):
            area = S * S * (scale[0] + (scale[1] - scale[0]) * uniform(skey, 1 + 4 * a))
            ar = math.exp(l0 + (l1 - l0) * uniform(skey, 2 + 4 * a))
            fh, fw = math.sqrt(area * ar), math.sqrt(area / ar)
            fragile[b] = fragile[b] or _near_half(fh) or _near_half(fw)
            h, w = int(round(fh)), int(round(fw))
            if h < S and w < S:
                i = int(uniform(skey, 3 + 4 * a) * (S - h + 1))
                j = int(uniform(skey, 4 + 4 * a) * (S - w + 1))
                boxes[b] = (i, i + h, j, j + w)
                accepted[b] = a
                break
    return boxes, accepted, fragile


_INT = {2: torch.int16, 4: torch.int32}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns as integers (so +0.0 != -0.0 and NaN payloads compare)."""
    t = t.detach().contiguous().cpu()
    return t.view(_INT[t.element_size()])


def erased(x: torch.Tensor, boxes, layout: int) -> torch.Tensor:
    """``x`` with the pixels y1 <= y < y2, x1 <= x < x2 (box of sample b, clamped to [0, S]) set to
    +0.0 in all three channels, by index arithmetic on the integer bit patterns: NCHW element
    [b][c][y][x]; s2d element [b][y // 2][x // 2][6*(y % 2) + 3*(x % 2) + c]. Every other element,
    the s2d slots 12..15 included, keeps its bits. Returns a new tensor of x's dtype."""
    out = bits(x).clone()
    B = x.shape[0]
    S = x.shape[2] * (2 if layout == S2D else 1)
    rows = np.asarray(boxes).reshape(B, 4).tolist()
    for b, (y1, y2, x1, x2) in enumerate(rows):
        y1, y2, x1, x2 = max(y1, 0), min(y2, S), max(x1, 0), min(x2, S)
        if y1 >= y2 or x1 >= x2:
            continue
        ys = torch.arange(y1, y2)[:, None]
        xs = torch.arange(x1, x2)[None, :]
        for c in range(3):
            if layout == NCHW:
                out[b, c, ys, xs] = 0
            else:
                out[b, ys // 2, xs // 2, 6 * (ys % 2) + 3 * (xs % 2) + c] = 0
    return out.view(x.dtype)


# ------------------------------------------------------------------ shared fixtures
SEEDS, RANKS, EPOCHS, STEPS, SIDES, BATCH = (0, 5), (0, 1), (0, 1, 2), (0, 1, 7), (4, 10, 32, 224), 64
PROBS = (0.0, 0.25, 1.0)
# scale (1, 1), ratio (1, 1): h = w = S in every attempt, all ten refused (h < S is strict)
REFUSED = ((1.0, 1.0), (1.0, 1.0))


def almost(S: int):
    """Bounds that give h = w = S - 1 in every attempt: accepted, at offsets in {0, 1}."""
    s = (S - 1) ** 2 / (S * S)
    return ((s, s), (1.0, 1.0))


def grid():
    return [(seed, rank, epoch, step, S) for seed in SEEDS for rank in RANKS for epoch in EPOCHS
            for step in STEPS for S in SIDES]


@functools.lru_cache(maxsize=None)
def grid_draw(seed, rank, epoch, step, S, p, B=BATCH, scale=SCALE, ratio=RATIO):
    """:func:`draw`, computed once per argument set and shared by the tests. Treat as read-only."""
    return draw(seed, rank, epoch, step, B, S, p, scale, ratio)


def box_kinds(S: int):
    """Eight hand-written boxes, one per sample of a batch of 8 (S >= 4)."""
    return {"empty": (1, 1, 0, S), "whole": (0, S, 0, S), "odd pixel": (1, 2, 3, 4),
            "flush with 0": (0, 2, 0, 3), "flush with S": (S - 3, S, S - 2, S),
            "one row": (2, 3, 0, S), "one column": (1, S - 1, 1, 2),
            "outside": (-3, S + 5, 1, S + 2)}


_NAN = {torch.float32: 0x7FC01234, torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}


@functools.lru_cache(maxsize=None)
def planted_input(layout: int, dtype, S: int, B: int = 8):
    """Random images with, in EVERY sample, -0, a NaN with a payload and the largest finite value of
    both signs at pixels of every row / column parity (the boxes of :func:`box_kinds` catch some of
    them and miss others); an s2d batch has its slots 12..15 filled with 3.0. Treat as read-only."""
    from mix_refs import s2d_from_nchw
    g = torch.Generator().manual_seed(1000 * S + 10 * B + layout)
    img = torch.randn(B, 3, S, S, generator=g).to(dtype)
    fmax = torch.finfo(dtype).max
    img[:, 0, 0, 0] = -0.0
    img[:, 2, 1, 3] = -fmax
    img[:, 0, S - 1, S - 1] = fmax
    img[:, 2, S - 2, 0] = -0.0
    img[:, 1, 2, S - 1] = fmax
    iv = img.view(_INT[img.element_size()])
    iv[:, 1, 1, 1] = _NAN[dtype]
    iv[:, 1, 2, 1] = _NAN[dtype]
    iv[:, 0, 0, S - 2] = _NAN[dtype]
    if layout == NCHW:
        return img
    x = s2d_from_nchw(img)
    x[..., 12:] = 3.0
    return x
