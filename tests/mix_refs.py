"""float64 references for the soft-target loss and the batch mixing (tests/test_soft_xent_gpu.py,
tests/test_batch_mix_gpu.py, tests/test_mix_cpu.py).

Everything here runs on the CPU and uses no kernel of this project; tests/test_mix_refs_cpu.py
checks these functions against torch where torch's behaviour is defined.
"""
import torch

F64 = torch.float64
S2D, NCHW = 0, 1
MIXUP, CUTMIX = 0, 1


def soft_target(K: int, a, b, lam: float, eps: float):
    """q[r][k] = eps/K + (1-eps) * (lam*[k==a_r] + (1-lam)*[k==b_r]) in float64; ``b`` None: b = a."""
    B = a.shape[0]
    b = a if b is None else b
    q = torch.full((B, K), eps / K, dtype=F64)
    ar = torch.arange(B)
    q[ar, a] += (1.0 - eps) * lam
    q[ar, b] += (1.0 - eps) * (1.0 - lam)
    return q


def xent_soft_ref(x64, a, b, lam: float, eps: float):
    """(loss_rows, dloss_rows/dlogits) in float64 against :func:`soft_target`: lse(x) - sum_k q_k x_k
    and softmax(x) - q."""
    x = x64.to(F64)
    q = soft_target(x.shape[1], a, b, lam, eps)
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    # lse - sum q x with both parts shifted by m (sum q = 1)
    rows = torch.log(s).squeeze(1) - (q * (x - m)).sum(1)
    return rows, e / s - q


def s2d_from_nchw(x):
    """[B, 3, S, S] -> [B, S/2, S/2, 16] by the stem's space-to-depth formula (csrc/misc.hip):
    X'[i][j][(p*2+q)*3+c] = x[c][2i+p][2j+q], slots 12..15 zero. Explicit index arithmetic."""
    B, C, S, _ = x.shape
    assert C == 3 and S % 2 == 0
    out = torch.zeros(B, S // 2, S // 2, 16, dtype=x.dtype)
    for p in range(2):
        for q in range(2):
            for c in range(3):
                out[:, :, :, (p * 2 + q) * 3 + c] = x[:, c, p::2, q::2]
    return out


def nchw_from_s2d(x):
    """The inverse re-layout (slots 12..15 dropped)."""
    B, S2, _, _ = x.shape
    out = torch.zeros(B, 3, 2 * S2, 2 * S2, dtype=x.dtype)
    for p in range(2):
        for q in range(2):
            for c in range(3):
                out[:, c, p::2, q::2] = x[:, :, :, (p * 2 + q) * 3 + c]
    return out


def f32_weights(lam: float):
    """(lam, 1 - lam) as the kernel receives them: lam rounded to float32, then one float32
    subtraction from 1; returned as Python floats (exact)."""
    lam32 = torch.tensor(lam, dtype=torch.float32)
    oml32 = torch.tensor(1.0, dtype=torch.float32) - lam32
    return float(lam32), float(oml32)


def batch_mix_ref(x, layout: int, mode: int, lam: float, box=None):
    """Sample b mixed with sample (b-1) mod B, by index arithmetic on an NCHW view (an s2d input is
    re-laid to NCHW, mixed there and laid back; its slots 12..15 come out 0).

    MIXUP: float64 ``lam32*x[b] + oml32*x[b-1]`` with the float32 weights of :func:`f32_weights`,
    returned in float64 (the caller bounds the rounding). CUTMIX: pixel (y, x) with y1 <= y < y2
    and x1 <= x < x2 is the partner's element, every other x[b]'s, in x's own dtype (a select)."""
    img = nchw_from_s2d(x) if layout == S2D else x
    B, _, S, _ = img.shape
    idx = [(b - 1) % B for b in range(B)]
    part = img[idx]
    if mode == MIXUP:
        lam32, oml32 = f32_weights(lam)
        out = lam32 * img.to(F64) + oml32 * part.to(F64)
    else:
        y1, y2, x1, x2 = box
        yy = torch.arange(S)[:, None]
        xx = torch.arange(S)[None, :]
        inside = (yy >= y1) & (yy < y2) & (xx >= x1) & (xx < x2)
        out = torch.where(inside[None, None], part, img)
    return s2d_from_nchw(out) if layout == S2D else out
