"""Packed image files: a pre-decoded, pre-shrunk split in ONE file, resident on the GPU.

The reference reads ImageNet from pre-packed ``ffrecord`` files; the folder path
(``data/folder.py``) decodes JPEGs in DataLoader workers every step and is bound by them
(``profiles/aug_gpu.md`` section 2). A packed file holds every image of a split already decoded to
raw HWC uint8 RGB and shrunk once to a short side of ``short_side`` (never enlarged). It is read
with ``mmap`` and copied to the device once (:meth:`PackedImages.to_device`); after that a training
step uploads a batch of sample ids and launches two kernels of ``csrc/augment.hip``:
``aug_draw_kernel`` draws crop boxes and flips and looks up offsets, sizes and labels,
``aug_resize_kernel`` resamples the resident pixels through those tables into the model-ready batch.
Selected with ``MX_DATA=packed:<dir>`` (``<dir>/train.pack``, ``<dir>/val.pack``), written by
:func:`write_packed` / ``tools/pack_images.py``.

File layout, little-endian::

    header   72 B   "PDAPACK\\0", then 8 uint64: version, N, short_side, names offset, names bytes,
                    index offset, pixels offset, pixels bytes
    names           JSON list of class names in ImageFolder's sorted-directory order
    index           int64 [N, 4]: byte offset into the pixel section, H, W, label
    pixels          every image's record back to back

The version is the record format. Version 1 (``fmt="rgb"``): a record is the image's HWC uint8 RGB
bytes, ``3*H*W``. Version 2 (``fmt="yuv420"``): YCbCr 4:2:0, the layout almost every source JPEG
already has: the Y plane ``[H, W]``, then the CbCr plane ``[Hc, Wc, 2]`` (Cb and Cr interleaved) with
``Hc = (H+1)//2``, ``Wc = (W+1)//2``; ``H*W + 2*Hc*Wc`` bytes, half of the RGB record. H and W in the
index are the luma size in both. The encoding is exact integer arithmetic on the shrunk RGB image
(16-bit JFIF weights, :func:`encode_yuv420`): a 2x2 block of luma rows ``2j, 2j+1`` and columns
``2i, 2i+1`` shares one chroma sample, an odd last row or column is repeated. What a version-2 file
STORES is the real-valued image, never rounded,

    cb = Cb[y>>1][x>>1] - 128,  cr = Cr[y>>1][x>>1] - 128                   (nearest chroma)
    R = Y + 1.402 cr,   G = Y - 0.344136 cb - 0.714136 cr,   B = Y + 1.772 cb

which ``aug_resize_kernel`` resamples by filtering the three stored planes and converting (and
clamping to 0..255) once per output pixel. A grey pixel stores ``Y = v, Cb = Cr = 128`` and decodes
exactly; a constant colour comes back, after the clamp, within 1.384 levels (all 2^24 checked). The
cost is chroma at half resolution.

Shrinking the training images once changes what ``RandomResizedCrop`` samples from: the crop is
drawn on the stored image, so a crop that covers less than ``short_side``-scale detail is enlarged
from fewer source pixels than the original file had. Validation with ``short_side`` equal to the
``Resize`` size is the reference's ``Resize -> CenterCrop`` on the same resized image (bilinear,
same target size).
"""
from __future__ import annotations

import json
import math
import mmap
import os
import struct
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .sampler import SequentialIndices

__all__ = ["MAGIC", "VERSION", "FORMATS", "shrunk_size", "encode_yuv420", "write_packed",
           "PackedImages", "PackedStore", "PackedLoader"]

MAGIC = b"PDAPACK\0"
VERSION = 1                                  # the version of an RGB file
FORMATS = {"rgb": 1, "yuv420": 2}            # record format -> file version
_HEADER = struct.Struct("<8s8Q")
STAGE_BYTES = 256 << 20       # bound on the pinned staging memory of the device-residency upload


def shrunk_size(W: int, H: int, short_side: int) -> Tuple[int, int]:
    """``(nw, nh)`` a WxH image is stored at: ``val_transform``'s resize target for
    ``resize=short_side`` when the short side exceeds it, else the image's own size."""
    if min(W, H) <= short_side:
        return W, H
    if W <= H:
        return short_side, int(short_side * H / W)
    return int(short_side * W / H), short_side


def encode_yuv420(a: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(Y [H, W], CbCr [Hc, Wc, 2])`` uint8 of a uint8 HxWx3 RGB image, in exact integers::

        Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
        cb = -11059 R - 21709 G + 32768 B ;  cr = 32768 R - 27439 G - 5329 B     (per pixel)
        Cb[j][i] = clip((sum of cb over the 2x2 block + (128 << 18) + (1 << 17)) >> 18, 0, 255)

    and Cr likewise; an odd last row or column is repeated into the block. The shifted sums are
    never negative (|sum| <= 4 * 32768 * 255 < 128 << 18)."""
    H, W, _ = a.shape
    p = np.pad(a, ((0, H & 1), (0, W & 1), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    out = np.empty((Hc, Wc, 2), dtype=np.uint8)
    for k, c in enumerate((-11059 * R - 21709 * G + 32768 * B, 32768 * R - 27439 * G - 5329 * B)):
        s = c.reshape(Hc, 2, Wc, 2).sum(axis=(1, 3))
        out[..., k] = np.clip((s + (128 << 18) + (1 << 17)) >> 18, 0, 255)
    return np.ascontiguousarray(Y[:H, :W].astype(np.uint8)), out


def _decode(job):
    """``(H, W, record bytes as a flat uint8 array)`` of one file."""
    from PIL import Image
    path, short_side, fmt = job
    with open(path, "rb") as fh:
        img = Image.open(fh)
        img.load()
    img = img.convert("RGB")
    size = shrunk_size(img.size[0], img.size[1], short_side)
    if size != img.size:
        img = img.resize(size, Image.BILINEAR)
    a = np.ascontiguousarray(np.asarray(img, dtype=np.uint8))
    H, W, _ = a.shape
    if fmt == "yuv420":
        return H, W, np.concatenate([p.reshape(-1) for p in encode_yuv420(a)])
    return H, W, a.reshape(-1)


def write_packed(root: str, split: str, out_path: str, short_side: int = 256,
                 workers: int = 0, fmt: str = "rgb") -> dict:
    """Decode ``<root>/<split>/<class>/*`` with PIL and write the packed file ``out_path``
    sequentially. ``workers`` > 0 decodes (and encodes) in that many processes (at most
    ``min(16, cpu_count)``). ``fmt`` "rgb" writes a version-1 file, "yuv420" a version-2 file of
    half the pixel bytes (module docstring). Returns ``{"images", "classes", "pixel_bytes",
    "file_bytes", "format"}``."""
    from ..ops.native_ops import AUG_MAX_SIDE
    from .folder import ImageFolder
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {sorted(FORMATS)}, got {fmt!r}")
    if short_side < 1:
        raise ValueError(f"short_side must be positive, got {short_side}")
    ds = ImageFolder(root, split)
    N = len(ds)
    names = json.dumps(ds.classes).encode("utf-8")
    names_off = _HEADER.size
    index_off = (names_off + len(names) + 7) // 8 * 8
    pixels_off = (index_off + N * 32 + 63) // 64 * 64
    index = np.zeros((N, 4), dtype="<i8")
    jobs = [(path, short_side, fmt) for path, _ in ds.samples]
    pool = None
    workers = min(int(workers), 16, os.cpu_count() or 1)
    if workers > 0:
        import multiprocessing as mp
        pool = mp.get_context("spawn").Pool(workers)
        decoded = pool.imap(_decode, jobs, chunksize=16)
    else:
        decoded = map(_decode, jobs)
    try:
        with open(out_path, "wb") as fh:
            fh.write(b"\0" * pixels_off)
            off = 0
            for k, (H, W, a) in enumerate(decoded):
                if not (1 <= H <= AUG_MAX_SIDE and 1 <= W <= AUG_MAX_SIDE):
                    raise ValueError(f"{ds.samples[k][0]}: size {W}x{H} outside 1..{AUG_MAX_SIDE}")
                index[k] = (off, H, W, ds.samples[k][1])
                fh.write(a.tobytes())
                off += a.size
            fh.seek(0)
            fh.write(_HEADER.pack(MAGIC, FORMATS[fmt], N, short_side, names_off, len(names), index_off,
                                  pixels_off, off))
            fh.write(names)
            fh.seek(index_off)
            fh.write(index.tobytes())
    finally:
        if pool is not None:
            pool.terminate()
            pool.join()
    return {"images": N, "classes": len(ds.classes), "pixel_bytes": off, "file_bytes": pixels_off + off,
            "format": fmt}


class PackedImages:
    """A packed split, ``mmap``-ed read-only. The header and the WHOLE index are validated here,
    once, on the host: the kernels trust the index afterwards as they trust ``aug_check``-ed tables.
    A bad file raises ``ValueError`` naming the first bad record."""

    def __init__(self, path: str) -> None:
        from ..ops.native_ops import AUG_MAX_SIDE
        self.path = str(path)
        size = os.path.getsize(self.path)
        if size < _HEADER.size:
            raise ValueError(f"{self.path}: {size} bytes, shorter than the {_HEADER.size}-byte header")
        with open(self.path, "rb") as fh:
            self._mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        magic, version, N, short_side, names_off, names_len, index_off, pixels_off, pixels_len = \
            _HEADER.unpack_from(self._mm, 0)
        if magic != MAGIC:
            raise ValueError(f"{self.path}: bad magic {magic!r}, not a packed image file")
        versions = {v: f for f, v in FORMATS.items()}
        if version not in versions:
            raise ValueError(f"{self.path}: version {version}, this reader knows {sorted(versions)}")
        self.format = versions[version]
        if N < 1 or N >= 2 ** 31:
            raise ValueError(f"{self.path}: {N} records")
        if not (_HEADER.size <= names_off and names_off + names_len <= index_off and index_off % 8 == 0
                and index_off + N * 32 <= pixels_off):
            raise ValueError(f"{self.path}: header sections overlap or are out of order")
        if pixels_off + pixels_len != size:
            raise ValueError(f"{self.path}: truncated or padded: the header describes "
                             f"{pixels_off + pixels_len} bytes, the file has {size}")
        try:
            self.classes: List[str] = json.loads(bytes(self._mm[names_off:names_off + names_len]))
        except ValueError as e:
            raise ValueError(f"{self.path}: class names are not JSON: {e}") from None
        if not isinstance(self.classes, list) or not all(isinstance(c, str) for c in self.classes):
            raise ValueError(f"{self.path}: class names must be a JSON list of strings")
        self.n, self.short_side = int(N), int(short_side)
        self.index = np.frombuffer(self._mm, dtype="<i8", count=N * 4, offset=index_off).reshape(N, 4)
        self.pixels = np.frombuffer(self._mm, dtype=np.uint8, count=pixels_len, offset=pixels_off)
        off, H, W, label = (self.index[:, k] for k in range(4))
        bad_size = (H < 1) | (H > AUG_MAX_SIDE) | (W < 1) | (W > AUG_MAX_SIDE)
        if bad_size.any():
            k = int(np.argmax(bad_size))
            raise ValueError(f"{self.path}: record {k}: size {int(W[k])}x{int(H[k])} outside "
                             f"1..{AUG_MAX_SIDE}")
        if self.format == "rgb":
            nbytes = 3 * H * W                     # <= 3 * 2^30: no overflow
        else:
            nbytes = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
        bad_off = (off < 0) | (off > pixels_len - nbytes)
        if bad_off.any():
            k = int(np.argmax(bad_off))
            raise ValueError(f"{self.path}: record {k}: bytes [{int(off[k])}, {int(off[k] + nbytes[k])}) "
                             f"outside the pixel section of {pixels_len}")
        bad_label = (label < 0) | (label >= len(self.classes))
        if bad_label.any():
            k = int(np.argmax(bad_label))
            raise ValueError(f"{self.path}: record {k}: label {int(label[k])} outside the "
                             f"{len(self.classes)} classes")
        order = np.argsort(off, kind="stable")
        over = off[order][:-1] + nbytes[order][:-1] > off[order][1:]
        if over.any():
            k = int(order[1:][over].min())
            raise ValueError(f"{self.path}: record {k}: its bytes overlap another record's")
        self.nbytes = nbytes
        self.pixel_bytes = int(pixels_len)

    def __len__(self) -> int:
        return self.n

    def image(self, i: int) -> np.ndarray:
        """HWC uint8 RGB view of image ``i`` of a version-1 file."""
        if self.format != "rgb":
            raise ValueError(f"{self.path}: a {self.format} file stores no RGB bytes; planes(i) "
                             f"returns the stored Y and CbCr planes")
        off, H, W, _ = (int(v) for v in self.index[i])
        return self.pixels[off:off + 3 * H * W].reshape(H, W, 3)

    def planes(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(Y [H, W], CbCr [Hc, Wc, 2])`` uint8 views of image ``i`` of a version-2 file."""
        if self.format != "yuv420":
            raise ValueError(f"{self.path}: a {self.format} file stores no planes; image(i) returns "
                             f"the stored RGB bytes")
        off, H, W, _ = (int(v) for v in self.index[i])
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        return (self.pixels[off:off + H * W].reshape(H, W),
                self.pixels[off + H * W:off + H * W + 2 * Hc * Wc].reshape(Hc, Wc, 2))

    def label(self, i: int) -> int:
        return int(self.index[i, 3])

    def to_device(self, device, mode: str = "auto", stage_bytes: int = STAGE_BYTES) -> "PackedStore":
        """Make the split readable by the kernels on ``device``. ``device``: the pixel section is
        copied to one uint8 device tensor through pinned staging of at most ``stage_bytes``; ``host``:
        only the index goes up, each batch's records are gathered from the mmap and uploaded;
        ``auto``: ``device`` when the pixels take at most half of the free device memory."""
        return PackedStore(self, device, mode, stage_bytes)


class PackedStore:
    """A :class:`PackedImages` split made readable on one GPU; see :meth:`PackedImages.to_device`."""

    def __init__(self, images: PackedImages, device, mode: str = "auto",
                 stage_bytes: int = STAGE_BYTES) -> None:
        self.images = images
        self.format = images.format
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"packed images are resampled on the GPU (csrc/augment.hip); the device is "
                             f"{self.device}. Use MX_DATA=folder:<root> on a CPU device.")
        if mode not in ("auto", "device", "host"):
            raise ValueError(f"MX_PACK_RESIDENT must be auto|device|host, got {mode!r}")
        if not 1 <= stage_bytes <= STAGE_BYTES:
            raise ValueError(f"stage_bytes must be in 1..{STAGE_BYTES}")
        if mode == "auto":
            free, _ = torch.cuda.mem_get_info(self.device)
            mode = "device" if images.pixel_bytes <= free // 2 else "host"
            print(f"packed data: {images.path}: {images.pixel_bytes} {images.format} pixel bytes, {free} "
                  f"device bytes free -> {mode} residency", flush=True)
        else:
            print(f"packed data: {images.path}: {images.pixel_bytes} {images.format} pixel bytes -> {mode} "
                  f"residency (requested)", flush=True)
        self.mode = mode
        self.index_dev = torch.from_numpy(np.array(images.index, dtype=np.int64)).to(self.device)
        self.pixels_dev: Optional[torch.Tensor] = None
        self._slots = None
        self._turn = 0
        if mode == "device":
            self.pixels_dev = self._upload(images.pixels, stage_bytes)

    def _upload(self, src: np.ndarray, stage_bytes: int) -> torch.Tensor:
        n = src.size
        dst = torch.empty(n, dtype=torch.uint8, device=self.device)
        chunk = max(1, min(n, stage_bytes // 2))
        bufs = [torch.empty(chunk, dtype=torch.uint8).pin_memory() for _ in range(2 if n > chunk else 1)]
        events = [None] * len(bufs)
        for t, a in enumerate(range(0, n, chunk)):
            k = t % len(bufs)
            m = min(chunk, n - a)
            if events[k] is not None:
                events[k].synchronize()          # the copy that last read this buffer has finished
            bufs[k].numpy()[:m] = src[a:a + m]
            dst[a:a + m].copy_(bufs[k][:m], non_blocking=True)
            events[k] = torch.cuda.Event()
            events[k].record(torch.cuda.current_stream(self.device))
        torch.cuda.current_stream(self.device).synchronize()
        return dst

    def batch(self, ids: torch.Tensor):
        """``(device bytes, device int64 [B] byte offsets or None)`` for the host ids ``ids``:
        the resident pixel tensor, or (host residency) the batch's records gathered back to back
        into one of two pinned staging buffers and uploaded with one asynchronous copy."""
        if self.mode == "device":
            return self.pixels_dev, None
        im = self.images
        idl = ids.tolist()
        sizes = im.nbytes[idl]
        offs = np.zeros(len(idl), dtype=np.int64)
        np.cumsum(sizes[:-1], out=offs[1:])
        total = int(sizes.sum())
        if self._slots is None:
            self._slots = [{"buf": None, "off": None, "event": None} for _ in range(2)]
        slot = self._slots[self._turn]
        self._turn ^= 1
        if slot["event"] is not None:
            slot["event"].synchronize()          # the copies that last read this slot have finished
        if slot["buf"] is None or slot["buf"].numel() < total:
            slot["buf"] = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
        if slot["off"] is None or slot["off"].numel() != len(idl):
            slot["off"] = torch.empty(len(idl), dtype=torch.int64).pin_memory()
        stage = slot["buf"].numpy()
        for i, o, m in zip(idl, offs.tolist(), sizes.tolist()):
            src = int(im.index[i, 0])
            stage[o:o + m] = im.pixels[src:src + m]
        slot["off"].numpy()[:] = offs
        packed = slot["buf"][:total].to(self.device, non_blocking=True)
        off_dev = slot["off"].to(self.device, non_blocking=True)
        slot["event"] = torch.cuda.Event()
        slot["event"].record(torch.cuda.current_stream(self.device))
        return packed, off_dev


class PackedLoader:
    """Batches of a packed split, model-ready on the device, with the surface of ``FolderLoader``
    (``__len__``, ``__iter__``, ``iter_from(start_step)``, ``max_steps``). No worker processes: per
    batch the host slices the epoch's ids (the sampler's, or 0..N-1 in order without one, as the
    folder loader), uploads them and launches ``aug_draw`` + ``aug_resize_dev``.

    ``split`` "train" draws RandomResizedCrop + flip per (seed, epoch, sample id); "val" is
    ``Resize(resize) -> CenterCrop(image_size)``. :meth:`set_epoch` selects the epoch of the draws;
    a sampler's own ``set_epoch`` still selects the permutation."""

    def __init__(self, store: PackedStore, split: str, batch_size: int, sampler=None,
                 max_steps: Optional[int] = None, dtype: torch.dtype = torch.float32,
                 layout: str = "nchw", image_size: int = 224, resize: Optional[int] = None,
                 seed: int = 0, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)) -> None:
        if split not in ("train", "val"):
            raise ValueError(f"split must be train|val, got {split!r}")
        if layout not in ("s2d", "nchw") or not image_size or image_size % 2:
            raise ValueError(f"packed data needs layout s2d|nchw and an even image_size, got "
                             f"{layout!r}, {image_size!r}")
        if layout == "nchw" and dtype != torch.float32:
            raise ValueError("the nchw layout is f32")
        if batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        self.store, self.split, self.batch_size = store, split, batch_size
        self.sampler = sampler if sampler is not None else SequentialIndices(len(store.images))
        self.max_steps, self.dtype, self.layout, self.image_size = max_steps, dtype, layout, image_size
        self.resize = int(round(image_size * 256 / 224)) if resize is None else resize
        self.seed, self.scale, self.ratio = seed, tuple(scale), tuple(ratio)
        self.device = store.device
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        n = math.ceil(len(self.sampler) / self.batch_size)
        return n if self.max_steps is None else min(n, self.max_steps)

    def _indices(self) -> torch.Tensor:
        if hasattr(self.sampler, "index_tensor"):
            return self.sampler.index_tensor().to(torch.int64)
        return torch.as_tensor(list(iter(self.sampler)), dtype=torch.int64)

    def make_batch(self, ids: torch.Tensor):
        """(x, labels) on the device for the host int64 ids ``ids``."""
        from ..ops import native_ops as K
        ids = ids.contiguous()
        S, B = self.image_size, ids.numel()
        packed, batch_off = self.store.batch(ids)
        train = self.split == "train"
        ti, tf, labels = K.aug_draw(ids, self.store.index_dev, len(self.store.images), self.seed,
                                    self.split, self.epoch, K.AUG_TRAIN if train else K.AUG_VAL, S,
                                    self.resize, self.scale, self.ratio, batch_off=batch_off)
        shape = (B, S // 2, S // 2, 16) if self.layout == "s2d" else (B, 3, S, S)
        x = torch.empty(shape, dtype=self.dtype, device=self.device)
        K.aug_resize_dev(packed, ti, tf, x, K.AUG_S2D if self.layout == "s2d" else K.AUG_NCHW,
                         K.AUG_YUV420 if self.store.format == "yuv420" else K.AUG_RGB)
        return x, labels

    def iter_from(self, start_step: int = 0) -> Iterator:
        """Yield ``(step, batch)`` from ``start_step``; the skipped batches cost nothing."""
        idx = self._indices()
        for step in range(start_step, len(self)):
            yield step, self.make_batch(idx[step * self.batch_size:(step + 1) * self.batch_size])

    def __iter__(self):
        for _, b in self.iter_from(0):
            yield b
