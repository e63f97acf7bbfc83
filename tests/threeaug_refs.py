"""Float64 numpy reference of the 3-Augment (csrc/threeaug.hip, pytorch_distributed_amd/threeaug.py),
written from the definition alone, and the inputs and hand-made tables the CPU and GPU tests share."""
import numpy as np
import torch

S2D, NCHW = 0, 1
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
THR = 128 / 255
PAD = 7.0            # the sentinel in the s2d padding slots
# (B, S, R): the smallest size that runs; reflection from both sides across almost the whole image;
# 36 = the smallest even side above the 32 x 32 tile + 2: ragged tiles both ways, halos crossing tile
# and image edges; 13 (NCHW only): an odd side, S*S % 4 != 0
SHAPES = [(1, 2, 1), (3, 12, 11), (2, 36, 11)]
NCHW_ONLY = [(2, 13, 11)]
KINDS = 6            # table kind k: sample b takes op (k + b) % 3, blur rows sigma 0.1 / 2.0 in turn


def pixels(x, layout):
    """``[B, S, S, 3]`` of a batch in ``layout`` (a copy)."""
    if layout == NCHW:
        return np.moveaxis(x, 1, -1).copy()
    B, h = x.shape[:2]
    return x[..., :12].reshape(B, h, h, 2, 2, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * h, 3)


def unpixels(img, like, layout):
    """``img`` back in ``layout``; the s2d padding slots come from ``like``."""
    if layout == NCHW:
        return np.moveaxis(img, -1, 1).copy()
    B, h = like.shape[:2]
    out = like.astype(img.dtype)
    out[..., :12] = img.reshape(B, h, 2, h, 2, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B, h, h, 12)
    return out


def _blur_axis(img, w, R, axis, dtype):
    pad = [(0, 0)] * img.ndim
    pad[axis] = (R, R)
    p = np.pad(img, pad, mode="reflect")
    n, acc = img.shape[axis], np.zeros_like(img)
    for k in range(2 * R + 1):                                  # ascending taps, sequential sums
        acc = acc + dtype(w[abs(k - R)]) * np.take(p, range(k, k + n), axis=axis)
    return acc


def three_aug_ref(x, table, layout, dtype=np.float64):
    """The definition on the batch's stored values ``x`` with the table's op, R and float32 weights
    (widened). ``dtype`` float32 evaluates the same formulas in single precision (the tolerance's
    yardstick)."""
    x = np.asarray(x, dtype)
    mean, std = MEAN.astype(dtype), STD.astype(dtype)
    img = np.clip(pixels(x, layout) * std + mean, 0, 1)
    wts = np.ascontiguousarray(table[:, 4:]).view(np.float32)
    for b, (op, R) in enumerate(zip(table[:, 0], table[:, 2])):
        v = img[b]
        if op == 0:
            v = np.repeat((dtype(0.2989) * v[..., 0] + dtype(0.587) * v[..., 1] + dtype(0.114) * v[..., 2])[..., None], 3, -1)
        elif op == 1:
            v = np.where(v >= dtype(THR), 1 - v, v)
        else:
            v = _blur_axis(_blur_axis(v, wts[b], R, 1, dtype), wts[b], R, 0, dtype)
        img[b] = v
    return unpixels((img - mean) / std, x, layout)


def hand_table(k, B, R):
    from pytorch_distributed_amd.threeaug import three_aug_table
    return three_aug_table([(k + b) % 3 for b in range(B)], [(0.1, 2.0)[((k + b) // 3) % 2] for b in range(B)], R)


def levels_input(layout, dtype, B, S):
    """Normalised k/255 levels (seeded) rounded to ``dtype``, the first pixels of every image forced
    below 0, above 1 and onto 0, 1 and the levels around the solarize threshold; a level whose stored
    value un-normalises to within 1e-4 of 128/255 moves up by two until none does."""
    k = np.random.default_rng(S * 137 + B).integers(0, 256, (B, S * S, 3))
    forced = [(-20, 280, 0), (255, 127, 129), (128, 128, 128), (126, 130, 300)]
    for n, px in enumerate(forced[:S * S]):
        k[:, n] = px
    for _ in range(8):
        img = torch.tensor(((k / 255 - MEAN) / STD).reshape(B, S, S, 3)).to(dtype)
        near = np.abs(img.double().numpy().reshape(B, S * S, 3) * STD + MEAN - THR) < 1e-4
        if not near.any():
            break
        k = k + 2 * near
    assert not near.any()
    if layout == NCHW:
        return img.permute(0, 3, 1, 2).contiguous()
    x = torch.full((B, S // 2, S // 2, 16), PAD, dtype=dtype)
    x[..., :12] = img.reshape(B, S // 2, 2, S // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, S // 2, S // 2, 12)
    return x
