"""Float64 Python reference of the packed data path's crop draw (csrc/augment.hip aug_draw_kernel,
ops.native_ops.aug_draw), and the fixtures the packed tests share.

Nothing here uses a kernel of this project. tests/test_packed_refs_cpu.py checks the reference
against ``data.folder.train_crop_params`` / ``val_crop_params``; tests/test_packed_gpu.py compares
the kernel with it.

The draw of sample ``id`` in epoch ``e`` of ``split`` under ``seed`` (all uint32 arithmetic):

    salt = (seed*97 + SPLIT_ID[split]) * 0x632BE5AB         (as the synthetic data)
    key  = hash32(id*2654435761 + salt)
    ekey = hash32(key ^ (e*0x9E3779B9 + 0x85EBCA6B))
    u(k) = hash32(ekey ^ ((k+1)*0x27D4EB2F)) / 2^32         (exact in float64)

Train mode is ``train_crop_params`` with ``rng.uniform(a, b) = a + (b-a)*u`` and
``rng.randint(0, n-1) = int(u*n)`` on fixed counters: attempt a uses u(4a) for the area, u(4a+1)
for the ratio, u(4a+2) for the row, u(4a+3) for the column; the flip is u(40) < 0.5.

The only step where a device ``exp`` (or the reference's own ``math.exp``) can legitimately change
an integer is the rounding of ``sqrt(target*ar)`` / ``sqrt(target/ar)``: a sample is FRAGILE when
one of these values, in any attempt the reference evaluated, lies within ``FRAGILE_EPS`` of k + 0.5.
Relative errors of a few ulp (1e-16) in exp move the roots by < 1e-11 at sides <= 32768, so 1e-6
is generous; the tests assert that their seeds and epochs have NO fragile sample.
"""
import math
import os

import numpy as np

from pytorch_distributed_amd.data.synthetic import SPLIT_ID

M32 = 0xFFFFFFFF
FRAGILE_EPS = 1e-6
SCALE, RATIO = (0.08, 1.0), (3 / 4, 4 / 3)


def hash32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def epoch_key(sample_id: int, seed: int, split: str, epoch: int) -> int:
    salt = ((seed * 97 + SPLIT_ID[split]) * 0x632BE5AB) & M32
    key = hash32(((sample_id & M32) * 2654435761 + salt) & M32)
    return hash32(key ^ ((epoch * 0x9E3779B9 + 0x85EBCA6B) & M32))


def uniform(ekey: int, k: int) -> float:
    return hash32(ekey ^ (((k + 1) * 0x27D4EB2F) & M32)) / 4294967296.0


def _near_half(v: float) -> bool:
    return abs((v - math.floor(v)) - 0.5) <= FRAGILE_EPS


def draw_train(W: int, H: int, sample_id: int, seed: int, epoch: int, split: str = "train",
               scale=SCALE, ratio=RATIO):
    """``(box (x0, y0, x1, y1) ints, flip, attempts, fragile)``; attempts = 11 for the fallback."""
    ekey = epoch_key(sample_id, seed, split, epoch)
    area = W * H
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    box, fragile, attempts = None, False, 11
    for a in range(10):
        target = area * (scale[0] + (scale[1] - scale[0]) * uniform(ekey, 4 * a))
        ar = math.exp(l0 + (l1 - l0) * uniform(ekey, 4 * a + 1))
        fw, fh = math.sqrt(target * ar), math.sqrt(target / ar)
        fragile = fragile or _near_half(fw) or _near_half(fh)
        w, h = int(round(fw)), int(round(fh))
        if 0 < w <= W and 0 < h <= H:
            i = int(uniform(ekey, 4 * a + 2) * (H - h + 1))
            j = int(uniform(ekey, 4 * a + 3) * (W - w + 1))
            box, attempts = (j, i, j + w, i + h), a + 1
            break
    if box is None:
        in_ratio = W / H
        if in_ratio < ratio[0]:
            w, h = W, int(round(W / ratio[0]))
        elif in_ratio > ratio[1]:
            h, w = H, int(round(H * ratio[1]))
        else:
            w, h = W, H
        i, j = (H - h) // 2, (W - w) // 2
        box = (j, i, j + w, i + h)
    return box, uniform(ekey, 40) < 0.5, attempts, fragile


def draw_val(W: int, H: int, size: int, resize: int):
    """``val_crop_params`` written out (checked against it on the CPU)."""
    if W <= H:
        nw, nh = resize, int(resize * H / W)
    else:
        nh, nw = resize, int(resize * W / H)
    top = int(round((nh - size) / 2.0))
    left = int(round((nw - size) / 2.0))
    return (left * W / nw, top * H / nh, (left + size) * W / nw, (top + size) * H / nh)


# ------------------------------------------------------------------ shared fixtures
# the smallest set that reaches every branch: ordinary images; 5x200, where every train attempt
# fails (w >= sqrt(0.08*1000*0.75) > 5) and the in_ratio < 3/4 fallback runs; 200x5, the other one
SIZES = [(53, 37), (48, 64), (31, 31), (5, 200), (200, 5)]
N_IMAGES, BATCH, N_CLASSES = 11, 7, 3
SEEDS, EPOCHS = (0, 5), (0, 1, 2)


def fixture_sizes():
    return [SIZES[k % len(SIZES)] for k in range(N_IMAGES)]


def fixture_images(seed: int = 0):
    """N_IMAGES seeded uint8 HWC arrays in the order ``ImageFolder`` lists the tree of
    :func:`make_tree`, with their labels."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for W, H in fixture_sizes()]
    return images, [k * N_CLASSES // N_IMAGES for k in range(N_IMAGES)]


def make_tree(root: str, split: str = "train", seed: int = 0, images=None, labels=None):
    """Write the fixture images as PNGs (lossless) under ``<root>/<split>/c<label>/``; file names
    sort in fixture order, so dataset index k is fixture image k."""
    from PIL import Image
    if images is None:
        images, labels = fixture_images(seed)
    for k, (img, label) in enumerate(zip(images, labels)):
        d = os.path.join(root, split, f"c{label}")
        os.makedirs(d, exist_ok=True)
        Image.fromarray(img).save(os.path.join(d, f"img{k:04d}.png"))
    return images, labels


def make_packed(root: str, seed: int = 0, short_side: int = 256):
    """Fixture tree + ``train.pack`` / ``val.pack`` under ``root``; returns (images, labels)."""
    from pytorch_distributed_amd.data.packed import write_packed
    images, labels = make_tree(root, "train", seed)
    make_tree(root, "val", seed)
    for split in ("train", "val"):
        write_packed(root, split, os.path.join(root, split + ".pack"), short_side)
    return images, labels
