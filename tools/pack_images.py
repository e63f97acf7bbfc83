#!/usr/bin/env python
"""Pack an ImageNet-style folder into the files ``MX_DATA=packed:<dir>`` reads.

``<root>/{train,val}/<class>/*`` -> ``<out>/train.pack``, ``<out>/val.pack`` (format:
pytorch_distributed_amd/data/packed.py). Every image is decoded with PIL and, when its short side
exceeds ``--short-side``, shrunk once (bilinear) to the size ``Resize(short_side)`` gives; smaller
images are stored as they are.

``--format rgb`` (default) stores raw RGB, 3 bytes per pixel. ``--format yuv420`` stores luma at
full and chroma at half resolution in both directions (YCbCr 4:2:0, what almost every source JPEG
already carries), 1.5 bytes per pixel: the file, the one-time upload to the GPU, the per-batch upload
of ``MX_PACK_RESIDENT=host`` and the bytes the resample kernel reads all halve, so a split twice as
large stays resident. The cost: colour detail finer than two pixels of the stored image is averaged
(grey images are stored exactly, constant colours within 1.4 levels), and the resample kernel
converts to RGB once per output pixel. The reader takes the format from the file.

    python tools/pack_images.py /data/imagenet /data/imagenet_packed --short-side 256 --workers 16
    python tools/pack_images.py /data/imagenet /data/imagenet_yuv --format yuv420 --workers 16
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
    ap.add_argument("--format", choices=("rgb", "yuv420"), default="rgb",
                    help="record format: raw RGB, or YCbCr 4:2:0 at half the bytes")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for split in a.splits.split(","):
        t0 = time.perf_counter()
        r = write_packed(a.root, split, os.path.join(a.out, split + ".pack"), a.short_side, a.workers,
                         fmt=a.format)
        dt = time.perf_counter() - t0
        print(f"{split}: {r['format']}, {r['images']} images, {r['classes']} classes, {r['pixel_bytes'] / 2**20:.1f} MiB "
              f"of pixels ({r['pixel_bytes'] / r['images'] / 1024:.1f} KiB per image) in {dt:.1f} s "
              f"({r['images'] / dt:.0f} img/s)", flush=True)


if __name__ == "__main__":
    main()
