"""Float64 numpy reference of RandAugment (csrc/randaug.hip, pytorch_distributed_amd/randaug.py),
written from the definition alone, with the inputs and hand-made rows the CPU and GPU tests share.
Images are handled as stored values [B, S, S, 3]; images() / the layouts convert."""
import numpy as np
import torch

from jitter_refs import MEAN, NCHW, PAD, S2D, STD, levels_input

GEO, EQUALIZE, POSTERIZE = range(1, 6), 13, 10


def images(x, layout):
    """[B, S, S, 3] float64 of a stored batch (tensor) in ``layout``"""
    x = x.double().numpy()
    if layout == NCHW:
        return np.moveaxis(x, 1, -1).copy()
    B, h = x.shape[:2]
    return x[..., :12].reshape(B, h, h, 2, 2, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * h, 2 * h, 3)


def coeffs(op, mag, S):
    """the six affine coefficients of geometric op ``op`` at magnitude ``mag`` (shear factor, pixels, degrees)"""
    if op == 5:
        a, h = np.deg2rad(mag), S / 2
        c, s = np.cos(a), np.sin(a)
        return [c, -s, h - c * h + s * h, s, c, h - s * h - c * h]
    return {1: [1, mag, 0, 0, 1, 0], 2: [1, 0, 0, mag, 1, 0], 3: [1, 0, -mag, 0, 1, 0], 4: [1, 0, 0, 0, 1, -mag]}[op]


def slot_ref(st, op, par, co, dtype=np.float64):
    """One slot on a sample's stored values ``st`` [S, S, 3]: (new stored values before the rounding
    to the batch dtype, the elements [S, S, 3] a float32 evaluation may legitimately decide otherwise).
    ``dtype`` float32 evaluates the colour formulas in single precision (the tolerance's yardstick)."""
    S, skip = st.shape[0], np.zeros(st.shape, bool)
    if op in GEO:
        a = np.asarray(co, np.float32).astype(np.float64)
        c = np.arange(S) + 0.5
        cy, cx = c[:, None], c[None, :]
        u, v = a[0] * cx + a[1] * cy + a[2], a[3] * cx + a[4] * cy + a[5]
        skip[:] = ((np.abs(u - np.rint(u)) < 1e-3) | (np.abs(v - np.rint(v)) < 1e-3))[..., None]
        ui, vi = np.floor(u).astype(int), np.floor(v).astype(int)
        inside = (ui >= 0) & (ui < S) & (vi >= 0) & (vi < S)
        return np.where(inside[..., None], st[vi.clip(0, S - 1), ui.clip(0, S - 1)], 0.0), skip
    st, mean, std = st.astype(dtype), MEAN.astype(dtype), STD.astype(dtype)
    raw = st * std + mean
    img = np.clip(raw, 0, 1)
    f, keep = dtype(np.float32(par)), np.zeros(3, bool)
    gray = dtype(0.2989) * img[..., 0] + dtype(0.587) * img[..., 1] + dtype(0.114) * img[..., 2]
    q = np.floor(255 * img + dtype(0.5)).astype(int)
    tie = np.abs(255 * img - np.floor(255 * img) - 0.5) < 1e-3
    if op == 6:
        new = np.clip(f * img, 0, 1)
    elif op == 7:
        new = np.clip(f * img + ((1 - f) * gray)[..., None], 0, 1)
    elif op == 8:
        new = np.clip(f * img + (1 - f) * dtype(gray.mean(dtype=np.float64)), 0, 1)
    elif op == 9 and S > 2:
        blur = img.copy()
        blur[1:-1, 1:-1] = sum(img[1 + dy:S - 1 + dy, 1 + dx:S - 1 + dx] * dtype(5 if dy == dx == 0 else 1)
                               for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / dtype(13)
        new = np.clip(f * img + (1 - f) * blur, 0, 1)
    elif op == POSTERIZE:
        new, skip = (q & int(par)).astype(dtype) / dtype(255), tie
    elif op == 11:
        new, skip = np.where(img >= f, 1 - img, img), np.abs(img - f) < 1e-6
    elif op == 12:
        lo, hi = img.min((0, 1)), img.max((0, 1))
        keep = hi == lo
        new = np.clip((img - lo) * (1 / np.where(keep, dtype(1), hi - lo)), 0, 1)
    elif op == EQUALIZE:
        new, skip = img.copy(), tie              # (the tests assert that no element of an Equalize input ties)
        for c in range(3):
            hist = np.bincount(q[..., c].ravel(), minlength=256)
            step = (S * S - hist[np.flatnonzero(hist)[-1]]) // 255
            keep[c] = step == 0
            if step:
                lut = np.minimum(255, (np.cumsum(hist) - hist + step // 2) // step)
                new[..., c] = lut[q[..., c]].astype(dtype) / dtype(255)
    else:
        new, keep = img, np.ones(3, bool)
    same = np.where(img == raw, st, (img - mean) / std)
    return np.where(keep, same, (new - mean) / std), skip


def _round(a, tdtype):
    return torch.tensor(np.asarray(a, np.float64)).to(tdtype).double().numpy()


def chain_ref(imgs, ops, par, co, tdtype, dtype=np.float64):
    """Every sample's slots in turn on stored images ``imgs`` [B, S, S, 3], each but the last rounded to
    the torch dtype ``tdtype`` (the last one's rounding is the one the tests' bound allows for):
    (result, skipped elements, an Equalize input held a tie). A skipped element
    stays skipped through later slots: gathered by a geometric op, spread over the 3x3 window by
    Sharpness, over the whole sample by the ops that take a sample-wide statistic."""
    out, skip, eq_tie = np.empty(imgs.shape), np.zeros(imgs.shape, bool), False
    for b in range(imgs.shape[0]):
        st, sk = imgs[b], np.zeros(imgs[b].shape, bool)
        for j in range(ops.shape[1]):
            op = int(ops[b, j])
            new, s = slot_ref(st, op, par[b, j], co[b, j], dtype)
            if op in GEO:
                sk = (slot_ref(sk.astype(float), op, 0, co[b, j])[0] > 0) | s
            else:
                eq_tie |= op == EQUALIZE and bool(s.any())
                if sk.any() and (op in (8, 12, EQUALIZE) or op == 9):
                    sk[:] = True                 # (coarse on purpose: the tests bound the skipped share)
                sk = sk | s
            st = _round(new, tdtype) if j + 1 < ops.shape[1] else new
        out[b], skip[b] = st, sk
    return out, skip, eq_tie


# ---- shared inputs: (op, magnitude) rows; sample b of table kind k takes row (k + b) % len(ROWS).
# magnitude: the shear factor, the pixels, the degrees, f, the posterize mask, the threshold
ROWS = [(0, 0), (1, 0.137), (1, -0.29), (2, 0.3), (2, -0.061), (3, 1), (3, -2), (4, 1), (4, -2), (5, 17.3),
        (5, -7.0), (6, 1.27), (6, 0.73), (7, 1.9), (7, 0.1), (8, 1.27), (8, 0.73), (9, 1.9), (9, 0.1),
        (10, 0xF0), (10, 0xFE), (11, 0.7), (11, 0.3), (12, 0), (13, 0)]


def hand_rows(k, B, S):
    """(ops [B, 1], params [B, 1], coeffs [B, 1, 6]) of table kind k"""
    rows = [ROWS[(k + b) % len(ROWS)] for b in range(B)]
    ops = np.array([[r[0]] for r in rows])
    par = np.array([[0.0 if r[0] in GEO else r[1]] for r in rows])
    co = np.array([[coeffs(r[0], r[1], S) if r[0] in GEO else [0.0] * 6] for r in rows])
    return ops, par, co


def randaug_input(layout, dtype, B, S):
    """jitter_refs.levels_input; the last sample of a batch of several has constant red and green
    channels (AutoContrast's hi == lo, Equalize's step == 0) beside a varied blue one"""
    img = torch.tensor(images(levels_input(layout, torch.float64, B, S), layout))
    if B > 1:
        img[-1, ..., 0], img[-1, ..., 1] = (77 / 255 - MEAN[0]) / STD[0], (200 / 255 - MEAN[1]) / STD[1]
    img = img.to(dtype)
    if layout == NCHW:
        return img.permute(0, 3, 1, 2).contiguous()
    x = torch.full((B, S // 2, S // 2, 16), PAD, dtype=dtype)
    x[..., :12] = img.reshape(B, S // 2, 2, S // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, S // 2, S // 2, 12)
    return x
