"""Float64 reference of the YCbCr 4:2:0 packed format (data/packed.py version 2) and of the resample
kernel's format-1 path (csrc/augment.hip), with the fixtures their tests share.

Nothing here uses a kernel or the encoder of this project: the integer encoder below is written
from the format's formulas with plain Python loops over the 2x2 blocks, the stored image is the
float64 decode with nearest chroma, and the resample is ``aug_refs.resample`` on the three stored
planes. tests/test_packed_yuv_refs_cpu.py compares ``write_packed(fmt="yuv420")`` with the encoder
byte for byte; tests/test_packed_yuv_gpu.py compares the kernel and the loader with ``transform``.

Encoding of a uint8 RGB image (exact integers):

    Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
    cb = -11059 R - 21709 G + 32768 B ;  cr = 32768 R - 27439 G - 5329 B
    Cb[j][i] = clip((sum of cb over rows 2j, 2j+1 and columns 2i, 2i+1 + (128 << 18) + (1 << 17)) >> 18,
                    0, 255), Cr likewise; a missing odd row or column repeats the last one.

The stored image (real-valued, nothing rounded):

    cb = Cb[y>>1][x>>1] - 128, cr = Cr[y>>1][x>>1] - 128
    R = Y + 1.402 cr, G = Y - 0.344136 cb - 0.714136 cr, B = Y + 1.772 cb

The kernel's output before normalisation is clip(M . filtered (Y, cb, cr), 0, 255).

Error bound of the kernel against ``transform``, in levels (``accum_bound``): each of the three
filtered planes carries the (kh + kv + 8) 2^-23 255 term of the RGB path (chroma magnitudes are
<= 128 < 255); the conversion mixes them with weights whose absolute sum is at most
1 + 1.772 * 128/255 < 2, and itself adds at most 2 * 2^-23 * 255 (two f32 constants and two fma
roundings on values below 512); clamping is 1-Lipschitz. Hence (2 (kh + kv + 8) + 2) 2^-23 255
levels, plus half an ulp of the stored dtype.
"""
import numpy as np
import torch

import aug_refs as R
from pytorch_distributed_amd.data.synthetic import MEAN, STD

# rows: R, G, B from (Y, cb, cr)
M = np.array([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=np.float64)


def encode(img: np.ndarray):
    """(Y [H, W], CbCr [Hc, Wc, 2]) uint8 of a uint8 HxWx3 image; Python integers throughout."""
    H, W, _ = img.shape
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    px = img.tolist()
    Y = np.zeros((H, W), dtype=np.uint8)
    C = np.zeros((Hc, Wc, 2), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            r, g, b = px[y][x]
            Y[y, x] = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    for j in range(Hc):
        for i in range(Wc):
            sb = sr = 0
            for y in (2 * j, min(2 * j + 1, H - 1)):
                for x in (2 * i, min(2 * i + 1, W - 1)):
                    r, g, b = px[y][x]
                    sb += -11059 * r - 21709 * g + 32768 * b
                    sr += 32768 * r - 27439 * g - 5329 * b
            for k, s in enumerate((sb, sr)):
                v = s + (128 << 18) + (1 << 17)
                assert v >= 0
                C[j, i, k] = min(max(v >> 18, 0), 255)
    return Y, C


def record(planes) -> np.ndarray:
    """The record's bytes: the Y plane, then the interleaved CbCr plane."""
    return np.concatenate([planes[0].reshape(-1), planes[1].reshape(-1)])


def record_bytes(H: int, W: int) -> int:
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def stored_planes(planes) -> np.ndarray:
    """[H, W, 3] float64 (Y, Cb_up - 128, Cr_up - 128), chroma taken from [y>>1][x>>1]."""
    Y, C = planes
    H, W = Y.shape
    up = C[np.arange(H)[:, None] >> 1, np.arange(W)[None, :] >> 1].astype(np.float64) - 128.0
    return np.concatenate([Y.astype(np.float64)[..., None], up], axis=2)


def stored_image(planes) -> np.ndarray:
    """[H, W, 3] float64 RGB levels the record stores (unclipped, unrounded)."""
    return stored_planes(planes) @ M.T


def transform(planes, box, S: int, flip: bool) -> np.ndarray:
    """Normalised [3, S, S] float64: resample the stored planes, convert, clip, normalise."""
    F = R.resample(stored_planes(planes), box, S)
    if flip:
        F = F[:, ::-1]
    rgb = np.clip(F @ M.T, 0.0, 255.0)
    v = (rgb / 255.0 - np.asarray(MEAN, dtype=np.float64)) / np.asarray(STD, dtype=np.float64)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def batch_nchw(planes_list, boxes, flips, S: int) -> np.ndarray:
    return np.stack([transform(p, b, S, f) for p, b, f in zip(planes_list, boxes, flips)])


def accum_bound(kh: int, kv: int) -> np.ndarray:
    """[3] per-channel bound in normalised units: (2 (kh + kv + 8) + 2) 2^-23 255 levels."""
    return (2 * (kh + kv + 8) + 2) * 2.0 ** -23 * 255.0 / (255.0 * np.asarray(STD, dtype=np.float64))


def pack(planes_list, boxes, flips, gaps=None):
    """The kernel's inputs for a list of (Y, CbCr) planes: (packed uint8 tensor, table_i64 [B,4] =
    byte offset, H, W, flip, table_f64 [B,4] = box). ``gaps[b]`` bytes of 0xFF go in front of
    record b; the default (1 or 2 bytes) makes every offset odd whatever the record sizes are."""
    B = len(planes_list)
    ti = torch.zeros(B, 4, dtype=torch.int64)
    tf = torch.zeros(B, 4, dtype=torch.float64)
    chunks, off = [], 0
    for b, (planes, box, flip) in enumerate(zip(planes_list, boxes, flips)):
        H, W = planes[0].shape
        gap = gaps[b] if gaps is not None else 2 - (off + 1) % 2
        chunks.append(np.full(gap, 0xFF, dtype=np.uint8))
        off += gap
        ti[b] = torch.tensor([off, H, W, int(flip)])
        tf[b] = torch.tensor([float(v) for v in box], dtype=torch.float64)
        rec = record(planes)
        assert rec.size == record_bytes(H, W)
        chunks.append(rec)
        off += rec.size
    return torch.from_numpy(np.concatenate(chunks)), ti, tf
