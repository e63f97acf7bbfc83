#!/usr/bin/env python
"""Generate an ImageNet-style folder of JPEGs for data-path measurements.

``<root>/{train,val}/n<class>/img<k>.jpg``: smooth random content (low-resolution noise enlarged
bicubically, plus a little per-pixel noise), so files compress and decode like photographs rather
than like white noise. Everything comes from ``--seed``; nothing is downloaded.

    python tools/make_jpeg_tree.py /tmp/tree --train 2000 --val 200 --size 500x375 --quality 90
"""
import argparse
import os

import numpy as np


def smooth_image(rng, W: int, H: int):
    from PIL import Image
    low = rng.integers(0, 256, (max(H // 32, 2), max(W // 32, 2), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((W, H), Image.BICUBIC), dtype=np.int16)
    a = a + rng.integers(-6, 7, a.shape, dtype=np.int16)
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8))


def make_tree(root: str, train: int, val: int, size=(500, 375), classes: int = 10, quality: int = 90,
              seed: int = 0) -> int:
    rng = np.random.default_rng(seed)
    nbytes = 0
    for split, n in (("train", train), ("val", val)):
        for k in range(n):
            d = os.path.join(root, split, f"n{k % classes:08d}")
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, f"img{k // classes}.jpg")
            smooth_image(rng, *size).save(path, quality=quality)
            nbytes += os.path.getsize(path)
    return nbytes


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("--train", type=int, default=2000)
    ap.add_argument("--val", type=int, default=200)
    ap.add_argument("--size", default="500x375")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    n = make_tree(a.root, a.train, a.val, (W, H), a.classes, a.quality, a.seed)
    print(f"{a.train + a.val} JPEGs, {n / 2**20:.1f} MiB under {a.root}")


if __name__ == "__main__":
    main()
