"""Float64 numpy reference of the colour jitter (csrc/jitter.hip, pytorch_distributed_amd/jitter.py),
written from the definition alone, and the inputs and hand-made tables the CPU and GPU tests share."""
import numpy as np
import torch

S2D, NCHW = 0, 1
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def _hue(img, fh):
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    maxc, minc = img.max(-1), img.min(-1)
    cr = maxc - minc
    eq = cr == 0
    s = cr / np.where(eq, 1, maxc)
    crd = np.where(eq, 1, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    h6 = np.where(maxc == r, bc - gc, np.where(maxc == g, 2 + rc - bc, 4 + gc - rc))
    h = np.mod(np.fmod(h6 / 6 + 1, 1) + fh, 1)
    i = np.floor(6 * h)
    f = 6 * h - i
    v = maxc
    p, q, t = (np.clip(v * (1 - w * s), 0, 1) for w in (1, f, 1 - f))
    six = np.stack([np.stack(c, -1) for c in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))])
    return np.take_along_axis(six, (i.astype(int) % 6)[None, ..., None], 0)[0]


def jitter_ref(x, factors, orders, layout, dtype=np.float64):
    """The definition on the batch's stored values ``x``: ``factors`` [B, 4] (brightness, contrast,
    saturation, hue; taken as float32), ``orders`` [B, 4] (ops 0..3 in order, -1 = none). ``dtype``
    float32 evaluates the same formulas in single precision (the tolerance's yardstick)."""
    x = np.asarray(x, dtype)
    B = x.shape[0]
    pix = x[..., :12].reshape(B, -1, 3) if layout == S2D else np.moveaxis(x, 1, -1).reshape(B, -1, 3)
    mean, std, res = MEAN.astype(dtype), STD.astype(dtype), np.empty_like(pix)
    for b in range(B):
        img = np.clip(pix[b] * std + mean, 0, 1)
        fb, fc, fs, fh = np.asarray(factors[b], np.float32).astype(dtype)
        for op in orders[b]:
            gray = dtype(0.2989) * img[:, 0] + dtype(0.587) * img[:, 1] + dtype(0.114) * img[:, 2]
            if op == 0:
                img = np.clip(fb * img, 0, 1)
            elif op == 1:
                img = np.clip(fc * img + (1 - fc) * dtype(gray.mean(dtype=np.float64)), 0, 1)
            elif op == 2:
                img = np.clip(fs * img + (1 - fs) * gray[:, None], 0, 1)
            elif op == 3:
                img = _hue(img, fh)
        res[b] = (img - mean) / std
    out = x.copy()
    if layout == S2D:
        out[..., :12] = res.reshape(*x.shape[:3], 12)
        return out
    return np.moveaxis(res.reshape(B, x.shape[2], x.shape[3], 3), -1, 1)


# ---- shared inputs: (factors, order) rows; sample b of table kind k takes row (k + b) % len(ROWS)
ROWS = [((1.3, 1, 1, 0), (0, -1, -1, -1)), ((1, 0.6, 1, 0), (-1, 1, -1, -1)),       # each op alone
        ((1, 1, 1.4, 0), (-1, -1, 2, -1)), ((1, 1, 1, 0.1), (3, -1, -1, -1)),
        ((1.2, 0.7, 1.3, -0.2), (1, 0, 2, 3)), ((0.8, 1.4, 0.5, 0.3), (3, 2, 0, 1)),   # contrast first / last
        ((0, 1.5, 1, 0), (0, 1, -1, -1)), ((1, 1, 1, 0.5), (-1, -1, -1, 3)),          # range ends
        ((1, 1, 1, -0.5), (-1, 3, -1, -1)), ((1, 1, 1, 0), (-1, -1, -1, -1))]         # ..., all skipped
PAD = 7.0            # the sentinel in the s2d padding slots


def hand_table(k, B):
    rows = [ROWS[(k + b) % len(ROWS)] for b in range(B)]
    return np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows])


def levels_input(layout, dtype, B, S):
    """Normalised k/255 levels (seeded), the first pixels of every image forced onto r = g = b, the
    max-channel ties r = g > b, g = b > r and r = b > g, 0 and 1; rounded to ``dtype``, in ``layout``."""
    k = np.random.default_rng(S * 131 + B).integers(0, 256, (B, S * S, 3))
    forced = [(90, 90, 90), (200, 200, 40), (10, 160, 160), (0, 0, 0), (250, 30, 250), (255, 255, 255)]
    for n, px in enumerate(forced[:S * S]):
        k[:, n] = px
    img = torch.tensor(((k / 255 - MEAN) / STD).reshape(B, S, S, 3)).to(dtype)
    if layout == NCHW:
        return img.permute(0, 3, 1, 2).contiguous()
    x = torch.full((B, S // 2, S // 2, 16), PAD, dtype=dtype)
    x[..., :12] = img.reshape(B, S // 2, 2, S // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(B, S // 2, S // 2, 12)
    return x
