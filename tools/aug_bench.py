#!/usr/bin/env python
"""Measure the folder-image augmentation path (MX_AUG=gpu): the kernel alone and the loader alone.

1. Kernel: B packed WxH uint8 images, RandomResizedCrop boxes from a fixed seed, S=224, bf16 s2d;
   HIP events around each launch after warm-up; median, and the achieved GB/s against the bytes the
   launch has to move (source bytes inside the boxes + the output written).
2. Loader: a generated JPEG tree (tools/make_jpeg_tree.py), no model; images/s of the CPU path
   (PIL transforms in the workers) and of the GPU path (workers decode, one kernel per batch).

    python tools/aug_bench.py --tree /tmp/tree --workers 16 --json out.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_distributed_amd.data.folder import (ImageFolder, train_crop_params, train_params,  # noqa: E402
                                                 train_transform)
from pytorch_distributed_amd.ops import native_ops as K  # noqa: E402


def kernel_alone(B: int, W: int, H: int, S: int, reps: int, warmup: int, seed: int) -> dict:
    dev = torch.device("cuda")
    rng = random.Random(seed)
    ti = torch.zeros(B, 4, dtype=torch.int64)
    tf = torch.zeros(B, 4, dtype=torch.float64)
    box_bytes = 0
    for b in range(B):
        box, flip = train_crop_params(W, H, rng=rng)
        ti[b] = torch.tensor([b * H * W * 3, H, W, int(flip)])
        tf[b] = torch.tensor(box, dtype=torch.float64)
        box_bytes += (box[2] - box[0]) * (box[3] - box[1]) * 3
    g = torch.Generator().manual_seed(seed)
    packed = torch.randint(0, 256, (B * H * W * 3,), dtype=torch.uint8, generator=g).to(dev)
    out = torch.empty(B, S // 2, S // 2, 16, dtype=torch.bfloat16, device=dev)
    ti, tf = ti.pin_memory(), tf.pin_memory()
    for _ in range(warmup):
        K.aug_resize(packed, ti, tf, out, K.AUG_S2D)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.aug_resize(packed, ti, tf, out, K.AUG_S2D)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))     # includes the two 12.8 KB table uploads
    out_bytes = out.numel() * out.element_size()
    med = statistics.median(times)
    return {"B": B, "image": f"{W}x{H}", "S": S, "reps": reps, "ms_median": med, "ms_min": min(times),
            "ms_max": max(times), "bytes_in_boxes": box_bytes, "bytes_written": out_bytes,
            "packed_bytes": packed.numel(), "gbps": (box_bytes + out_bytes) / med / 1e6}


def loader_alone(root: str, mode: str, batch: int, workers: int, S: int, epochs: int) -> dict:
    dev = torch.device("cuda")
    if mode == "cpu":
        ds = ImageFolder(root, "train", train_transform(S))
        ld = ds.loader(batch, num_workers=workers)
    else:
        ds = ImageFolder(root, "train", raw_params=train_params())
        ld = ds.loader(batch, num_workers=workers, device=dev, dtype=torch.bfloat16, layout="s2d",
                       image_size=S)
    rates = []
    for _ in range(epochs):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for x, y in ld:
            x = x.to(dev, non_blocking=True)       # the CPU path's batches still have to get there
            n += x.shape[0]
        torch.cuda.synchronize()
        rates.append(n / (time.perf_counter() - t0))
    return {"mode": mode, "images": len(ds), "batch": batch, "workers": workers,
            "img_per_s": rates, "img_per_s_median": statistics.median(rates)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=None, help="JPEG tree (generated into a temp dir when absent)")
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--loader-batch", type=int, default=50,
                    help="DataLoader workers each build whole batches: keep batches >> workers")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--skip-loader", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aug_bench.py measures on a GPU; none is visible")
    res = {"kernel": kernel_alone(a.batch, 500, 375, 224, a.reps, 10, 0)}
    print(json.dumps(res["kernel"]), flush=True)
    if not a.skip_loader:
        tmp = None
        root = a.tree
        if root is None or not os.path.isdir(os.path.join(root, "train")):
            from make_jpeg_tree import make_tree
            tmp = tempfile.TemporaryDirectory()
            root = root or tmp.name
            make_tree(root, a.images, 0)
        for mode in ("cpu", "gpu", "cpu", "gpu"):      # alternate: other work shares the host
            r = loader_alone(root, mode, a.loader_batch, a.workers, 224, a.epochs)
            res.setdefault("loader_" + mode, []).append(r)
            print(json.dumps(r), flush=True)
        if tmp is not None:
            tmp.cleanup()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
