"""Real-image data path: ImageNet-style folder dataset + the reference's transforms.

The reference reads ImageNet through ``hfai.datasets.ImageNet`` (ffrecord) and
applies, for training, ``RandomResizedCrop(224) -> RandomHorizontalFlip() ->
ToTensor() -> Normalize(mean, std)`` and, for validation, ``Resize(256) ->
CenterCrop(224) -> ToTensor() -> Normalize`` (reference ``restnet_ddp.py:101-116``).
torchvision is not available, so the transforms are re-implemented on PIL +
numpy with the same parameters (scale (0.08, 1), ratio (3/4, 4/3), 10 attempts,
bilinear resampling, center-crop fallback).

Layout: ``<root>/<split>/<class_name>/*.{jpg,jpeg,png,...}``; classes are sorted
by name (``ImageFolder`` convention). Selected with ``MX_DATA=folder:<root>``.
Decoding runs in ``num_workers`` DataLoader worker processes with pinned
memory, as in the reference; the native engine converts the NCHW batch to its
space-to-depth layout on the GPU.

``MX_AUG=gpu`` (raw mode): the workers only decode and draw the crop parameters
(:func:`train_crop_params` / :func:`val_crop_params`); :func:`collate_raw` packs
the batch's uint8 images into one byte tensor plus two small tables, and the
loader uploads it and runs ONE HIP kernel (``csrc/augment.hip``) that resamples,
flips, normalises and writes the model-ready tensor.
"""
from __future__ import annotations

import math
import os
import random
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .synthetic import MEAN, STD

__all__ = ["ImageFolder", "train_transform", "val_transform", "FolderLoader", "train_crop_params",
           "val_crop_params", "train_params", "val_params", "collate_raw", "unpack_raw"]

_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".ppm", ".webp", ".tif", ".tiff")


def _to_tensor_normalized(img) -> torch.Tensor:
    a = np.asarray(img.convert("RGB"), dtype=np.float32) / 255.0
    a = (a - np.asarray(MEAN, dtype=np.float32)) / np.asarray(STD, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


def train_crop_params(W: int, H: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                      rng: Optional[random.Random] = None):
    """RandomResizedCrop box + RandomHorizontalFlip draw for a WxH image: ``((x0, y0, x1, y1),
    flip)``. Draws from ``rng`` per attempt ``uniform, uniform, randint, randint`` (the randints
    only on an accepted attempt), then one ``random()`` for the flip."""
    rng = rng or random
    area = W * H
    log_r = (math.log(ratio[0]), math.log(ratio[1]))
    box = None
    for _ in range(10):
        target = area * rng.uniform(*scale)
        ar = math.exp(rng.uniform(*log_r))
        w = int(round(math.sqrt(target * ar)))
        h = int(round(math.sqrt(target / ar)))
        if 0 < w <= W and 0 < h <= H:
            i = rng.randint(0, H - h)
            j = rng.randint(0, W - w)
            box = (j, i, j + w, i + h)
            break
    if box is None:  # fallback: center crop at the clamped ratio
        in_ratio = W / H
        if in_ratio < ratio[0]:
            w, h = W, int(round(W / ratio[0]))
        elif in_ratio > ratio[1]:
            h, w = H, int(round(H * ratio[1]))
        else:
            w, h = W, H
        i, j = (H - h) // 2, (W - w) // 2
        box = (j, i, j + w, i + h)
    return box, rng.random() < 0.5


def train_transform(size: int = 224, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                    rng: Optional[random.Random] = None) -> Callable:
    rng = rng or random.Random()

    def f(img):
        from PIL import Image
        W, H = img.size
        box, flip = train_crop_params(W, H, scale, ratio, rng)
        img = img.resize((size, size), Image.BILINEAR, box=box)
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        return _to_tensor_normalized(img)

    return f


def val_transform(size: int = 224, resize: int = 256) -> Callable:
    def f(img):
        from PIL import Image
        W, H = img.size
        if W <= H:
            nw, nh = resize, int(resize * H / W)
        else:
            nh, nw = resize, int(resize * W / H)
        img = img.resize((nw, nh), Image.BILINEAR)
        top = int(round((nh - size) / 2.0))
        left = int(round((nw - size) / 2.0))
        img = img.crop((left, top, left + size, top + size))
        return _to_tensor_normalized(img)

    return f


def val_crop_params(W: int, H: int, size: int = 224, resize: int = 256):
    """``Resize(resize) -> CenterCrop(size)`` of a WxH image as ONE resample: the fractional source
    box ``(x0, y0, x1, y1)`` that the crop window covers."""
    if W <= H:
        nw, nh = resize, int(resize * H / W)
    else:
        nh, nw = resize, int(resize * W / H)
    top = int(round((nh - size) / 2.0))
    left = int(round((nw - size) / 2.0))
    return (left * W / nw, top * H / nh, (left + size) * W / nw, (top + size) * H / nh)


def train_params(scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), rng: Optional[random.Random] = None) -> Callable:
    """Raw-mode counterpart of :func:`train_transform`: ``(W, H) -> (box, flip)``, same draws."""
    rng = rng or random.Random()
    return lambda W, H: train_crop_params(W, H, scale, ratio, rng)


def val_params(size: int = 224, resize: int = 256) -> Callable:
    """Raw-mode counterpart of :func:`val_transform`: ``(W, H) -> (box, False)``."""
    return lambda W, H: (val_crop_params(W, H, size, resize), False)


def collate_raw(samples):
    """Raw-mode batch -> ``(packed, table_i64, table_f64, labels)``: every image's HWC uint8 bytes
    back to back in ONE uint8 tensor; ``table_i64`` [B,4] = byte offset, H, W, flip; ``table_f64``
    [B,4] = box x0, y0, x1, y1; int64 labels."""
    B = len(samples)
    ti = torch.empty(B, 4, dtype=torch.int64)
    tf = torch.empty(B, 4, dtype=torch.float64)
    labels = torch.empty(B, dtype=torch.int64)
    off = 0
    for b, (img, label, (box, flip)) in enumerate(samples):
        H, W, _ = img.shape
        ti[b] = torch.tensor([off, H, W, int(flip)], dtype=torch.int64)
        tf[b] = torch.tensor(box, dtype=torch.float64)
        labels[b] = label
        off += H * W * 3
    if torch.utils.data.get_worker_info() is not None:
        # in a worker: build the batch in shared memory, as default_collate does, so handing it to
        # the main process copies nothing
        packed = torch.empty(0, dtype=torch.uint8).new(
            torch.empty(0, dtype=torch.uint8)._typed_storage()._new_shared(off)).resize_(off)
    else:
        packed = torch.empty(off, dtype=torch.uint8)
    for (img, _, _), o in zip(samples, ti[:, 0].tolist()):
        packed[o:o + img.numel()] = img.reshape(-1)
    return packed, ti, tf, labels


def unpack_raw(packed, table_i64):
    """The HWC uint8 images of a :func:`collate_raw` batch (views of ``packed``)."""
    return [packed[o:o + H * W * 3].view(H, W, 3) for o, H, W, _ in table_i64.tolist()]


class ImageFolder(torch.utils.data.Dataset):
    """``raw_params`` (a ``(W, H) -> (box, flip)`` callable, :func:`train_params` /
    :func:`val_params`) selects raw mode: items are ``(uint8 HWC image, label, (box, flip))``."""

    def __init__(self, root: str, split: str = "train", transform: Optional[Callable] = None,
                 raw_params: Optional[Callable] = None) -> None:
        d = os.path.join(root, split)
        if not os.path.isdir(d):
            raise FileNotFoundError(f"no '{split}' split under {root}")
        self.classes = sorted(e for e in os.listdir(d) if os.path.isdir(os.path.join(d, e)))
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples: List[Tuple[str, int]] = []
        for c in self.classes:
            cd = os.path.join(d, c)
            for fn in sorted(os.listdir(cd)):
                if fn.lower().endswith(_EXT):
                    self.samples.append((os.path.join(cd, fn), self.class_to_idx[c]))
        if not self.samples:
            raise FileNotFoundError(f"no images under {d}")
        self.transform = transform
        self.raw_params = raw_params
        self.split = split

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, i: int):
        from PIL import Image
        path, label = self.samples[i]
        with open(path, "rb") as fh:
            img = Image.open(fh)
            img.load()
        if self.raw_params is not None:
            a = torch.from_numpy(np.array(img.convert("RGB"), dtype=np.uint8))
            return a, label, self.raw_params(a.shape[1], a.shape[0])
        x = self.transform(img) if self.transform else _to_tensor_normalized(img)
        return x, label

    def loader(self, batch_size: int, sampler=None, num_workers: int = 4, pin_memory: bool = True,
               max_steps: Optional[int] = None, device=None, dtype: torch.dtype = torch.float32,
               layout: str = "nchw", image_size: Optional[int] = None, **_) -> "FolderLoader":
        """Raw mode (``raw_params``) needs the GPU ``device``, ``image_size`` and the batch's
        ``layout`` ("s2d" in the model ``dtype``, or "nchw" f32)."""
        return FolderLoader(self, batch_size, sampler, num_workers, pin_memory, max_steps,
                            device=device, dtype=dtype, layout=layout, image_size=image_size)


class _Slice(torch.utils.data.Sampler):
    def __init__(self, indices: Sequence[int]) -> None:
        self.indices = list(indices)

    def __iter__(self):
        return iter(self.indices)

    def __len__(self) -> int:
        return len(self.indices)


class FolderLoader:
    """DataLoader wrapper with the same ``iter_from`` / ``len`` contract as the synthetic loader.

    Over a raw-mode dataset it yields batches that are already model-ready on ``device`` (as the
    synthetic loader's ``generator=`` path does): the packed uint8 batch is uploaded and
    ``ops.native_ops.aug_resize`` runs on the current stream."""

    def __init__(self, ds: ImageFolder, batch_size: int, sampler, num_workers: int, pin_memory: bool,
                 max_steps: Optional[int], device=None, dtype: torch.dtype = torch.float32,
                 layout: str = "nchw", image_size: Optional[int] = None) -> None:
        self.ds, self.batch_size, self.sampler = ds, batch_size, sampler
        self.num_workers, self.pin_memory, self.max_steps = num_workers, pin_memory, max_steps
        self.device = torch.device(device) if device is not None else None
        self.dtype, self.layout, self.image_size = dtype, layout, image_size
        if ds.raw_params is not None:
            if self.device is None or self.device.type != "cuda":
                raise ValueError(f"MX_AUG=gpu resamples on the GPU (csrc/augment.hip); the loader's "
                                 f"device is {self.device}. Use MX_AUG=cpu on a CPU device.")
            if layout not in ("s2d", "nchw") or not image_size or image_size % 2:
                raise ValueError(f"raw mode needs layout s2d|nchw and an even image_size, got "
                                 f"{layout!r}, {image_size!r}")
            if layout == "nchw" and dtype != torch.float32:
                raise ValueError("the nchw layout is f32")

    def _to_device(self, batch):
        """Raw batch -> (model-ready x, labels) on the device: H2D copies + one kernel launch."""
        from ..ops import native_ops as K
        packed, ti, tf, labels = batch
        S, B = self.image_size, ti.shape[0]
        shape = (B, S // 2, S // 2, 16) if self.layout == "s2d" else (B, 3, S, S)
        x = torch.empty(shape, dtype=self.dtype, device=self.device)
        packed_d = packed.to(self.device, non_blocking=True)
        K.aug_resize(packed_d, ti, tf, x, K.AUG_S2D if self.layout == "s2d" else K.AUG_NCHW)
        return x, labels.to(self.device, non_blocking=True)

    def _indices(self) -> List[int]:
        if self.sampler is None:
            return list(range(len(self.ds)))
        return list(iter(self.sampler))

    def __len__(self) -> int:
        n = math.ceil(len(self._indices()) / self.batch_size)
        return n if self.max_steps is None else min(n, self.max_steps)

    def iter_from(self, start_step: int = 0) -> Iterator:
        idx = self._indices()[start_step * self.batch_size:len(self) * self.batch_size]
        raw = self.ds.raw_params is not None
        dl = torch.utils.data.DataLoader(self.ds, batch_size=self.batch_size, sampler=_Slice(idx),
                                         num_workers=self.num_workers, pin_memory=self.pin_memory
                                         and torch.cuda.is_available(),
                                         persistent_workers=False,
                                         collate_fn=collate_raw if raw else None)
        held = None
        for k, batch in enumerate(dl):
            if raw:
                # the pinned source of the queued copies stays referenced until the next batch
                held, batch = batch, self._to_device(batch)
            yield start_step + k, batch
        del held

    def __iter__(self):
        for _, b in self.iter_from(0):
            yield b
