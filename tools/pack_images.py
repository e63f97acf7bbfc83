#!/usr/bin/env python
"""Pack an ImageNet-style folder into the files ``MX_DATA=packed:<dir>`` reads.

``<root>/{train,val}/<class>/*`` -> ``<out>/train.pack``, ``<out>/val.pack`` (format:
pytorch_distributed_amd/data/packed.py). Every image is decoded with PIL and, when its short side
exceeds ``--short-side``, shrunk once (bilinear) to the size ``Resize(short_side)`` gives; smaller
images are stored as they are.

    python tools/pack_images.py /data/imagenet /data/imagenet_packed --short-side 256 --workers 16
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_distributed_amd.data.packed import write_packed  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("out")
    ap.add_argument("--short-side", type=int, default=256)
    ap.add_argument("--splits", default="train,val")
    ap.add_argument("--workers", type=int, default=min(4, os.cpu_count() or 1),
                    help="decoding processes (at most min(16, cpu count)); 0: in this process")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for split in a.splits.split(","):
        t0 = time.perf_counter()
        r = write_packed(a.root, split, os.path.join(a.out, split + ".pack"), a.short_side, a.workers)
        dt = time.perf_counter() - t0
        print(f"{split}: {r['images']} images, {r['classes']} classes, {r['pixel_bytes'] / 2**20:.1f} MiB "
              f"of pixels ({r['pixel_bytes'] / r['images'] / 1024:.1f} KiB per image) in {dt:.1f} s "
              f"({r['images'] / dt:.0f} img/s)", flush=True)


if __name__ == "__main__":
    main()
