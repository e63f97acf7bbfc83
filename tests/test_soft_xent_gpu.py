"""xent_soft (csrc/mix.hip), the soft-target cross-entropy of label smoothing / mixup / CutMix, on
the grid of test_xent_edges (tests/test_head_kernels_gpu.py) against the float64 reference of
tests/mix_refs.py; and the wrapper's refusals."""
import math

import pytest
import torch

import head_refs as H
import mix_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
U24 = 2.0 ** -24

# (eps, lam, labels_b): None = no second label set, "roll" = labels.roll(1, 0), "same" = labels
COMBOS = [(0.0, 1.0, None), (0.1, 1.0, None), (0.0, 0.3, "roll"), (0.1, 0.3, "roll"),
          (0.1, 0.0, "roll"), (0.1, 0.5, "same")]


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def _strided_logits(x64, fill, lead=3, trail=5):
    B, Kc = x64.shape
    wide = torch.full((B, lead + Kc + trail), fill, dtype=torch.float32)
    wide[:, lead:lead + Kc] = x64.float()
    wide = wide.to(DEV)
    view = wide[:, lead:lead + Kc]
    assert view.stride(0) > Kc
    return wide, view


def _labels(B, Kc, g, flip):
    lab = torch.randint(0, Kc, (B,), generator=g)
    lab[0] = 0 if (B == 1 and flip) else Kc - 1
    if B > 1:
        lab[B - 1] = 0
    return lab


def _sync_cpu(*ts):
    torch.cuda.synchronize()
    return [t.cpu() for t in ts]


@pytest.mark.parametrize("Kc", [10, 63, 64, 65, 1000])
def test_xent_soft_edges(Kc):
    """xent_soft over B in {1,4,5,37}, strided NaN-padded logits, dlog [B, ld] bf16 / fp16 (ld = K
    rounded up to 64, and 1024) pre-filled with a sentinel, labels forced to 0 and K-1, logits x3,
    x30 (peaked) and x3 + 100, gscale = 1/B, with and without the device loss scale 65536, crossed
    with (eps, lam, labels_b) in COMBOS. The reference is evaluated at the float32 values of eps and
    lam that the kernel receives.

    The kernel: m = max x, d_k = x_k - m, s = sum exp(d_k), c = sum d_k (64 lanes, then a butterfly),
    u = eps/K, wa = (1-eps)*lam, wb = (1-eps)*(1-lam), q_k = u + wa[k==a] + wb[k==b],
    loss_row = (m + log s) - (wa*x_a + wb*x_b + (u*c + eps*m)), dlog = (exp(d_k)/s - q_k)*gscale*gdev.
    The bounds follow from these formulas, none from an output:

    loss_rows: the bound of test_xent_edges, 1e-5*|ref| + 4 * 2^-23 * M with M = max(1, max|x|),
    for m + log s and the final subtraction; plus 4 * 2^-23 * M for the weighted target term: wa and
    wb carry two roundings each and their products one (<= 3 * 2^-24 * (wa|x_a| + wb|x_b|) <=
    3 * 2^-24 * (1-eps) * M), eps*m one (2^-24 * eps * M), and three additions of partial sums that
    are at most M (3 * 2^-24 * M): under 8 * 2^-24 * M; plus the class sum: each d_k is rounded once,
    a lane adds ceil(K/64) of them and the butterfly six more, and u carries one rounding and its
    product another, so |u*c - (eps/K) sum d_k| <= eps * (ceil(K/64) + 9) * 2^-24 * max|x_k - m|.

    dlog[:, :K]: within ulp_out of float64 (softmax - q) * gscale * gdev plus the two allowances of
    test_xent_edges: 2^-126 (the hardware exponential flushes subnormal results) everywhere, and
    eps_p * p_k with eps_p = 2^-24 * (13 + 2|x_k - m| + 2 ln K + ceil(K/64)), the relative error of
    p_k = exp(d_k)/s that survives when p_k - q_k cancels -- at every column with q_k > 0 (every
    column when eps > 0, columns a and b with a non-zero weight otherwise). Columns >= K are 0.

    Worst err/bound ratios are printed; for (0, 1, none) also whether loss_rows and dlog are
    bit-equal to xent's (information, not asserted: the two expressions may contract differently)."""
    K = _k()
    g = H._gen(Kc)
    worst_rows = worst_g = 0.0
    same_rows = same_dlog = n_same = 0
    chunks = -(-Kc // 64)
    for B in (1, 4, 5, 37):
        base = torch.randn(B, Kc, generator=g, dtype=F64)
        ar = torch.arange(B)
        for vi, x64 in enumerate((base * 3, base * 30, base * 3 + 100)):
            x64 = x64.float().to(F64)            # the kernel's f32 inputs, exactly
            M = max(1.0, float(x64.abs().max()))
            dmax = x64.max(1).values - x64.min(1).values          # max |x_k - m| per row
            eps_p = U24 * (13 + 2 * (x64.max(1, keepdim=True).values - x64) + 2 * math.log(Kc) + chunks)
            for li, ld in enumerate(sorted({(Kc + 63) // 64 * 64, 1024})):
                labels = _labels(B, Kc, g, flip=li == 1)
                wide, logits = _strided_logits(x64, float("nan"))
                lab_d = labels.to(DEV)
                for eps, lam, bk in COMBOS:
                    lab_b = None if bk is None else (labels.roll(1, 0) if bk == "roll" else labels.clone())
                    lab_bd = None if lab_b is None else lab_b.to(DEV)
                    rows_ref, grad_ref = R.xent_soft_ref(x64, labels, lab_b, _f32(lam), _f32(eps))
                    q = R.soft_target(Kc, labels, lab_b, _f32(lam), _f32(eps))
                    row_bound = (1e-5 * rows_ref.abs() + 8 * H.EPS32 * M
                                 + eps * (chunks + 9) * U24 * dmax)
                    allow = torch.full_like(grad_ref, 2.0 ** -126)
                    allow += torch.where(q > 0, eps_p * (grad_ref + q), torch.zeros_like(q))
                    tag0 = (B, vi, ld, eps, lam, bk)
                    for dtype, gd in ((torch.bfloat16, None), (torch.float16, None), (torch.float16, 65536.0)):
                        rows = torch.full((B,), -5.0, device=DEV)
                        loss = torch.full((), -5.0, device=DEV)
                        dlog = torch.full((B, ld), 7.0, device=DEV, dtype=dtype)
                        gdev = torch.tensor([gd], device=DEV) if gd else None
                        K.xent_soft(logits, lab_d, rows, loss, labels_b=lab_bd, lam=lam, eps=eps,
                                    dlog=dlog, gscale=1.0 / B, gdev=gdev)
                        rows_c, loss_c, dlog_c = _sync_cpu(rows, loss, dlog)
                        err = (rows_c.to(F64) - rows_ref).abs()
                        worst_rows = max(worst_rows, float((err / row_bound).max()))
                        assert bool((err <= row_bound).all()), (tag0, dtype, gd, float((err / row_bound).max()))
                        torch.testing.assert_close(loss_c.to(F64), rows_ref.mean(), rtol=1e-4, atol=1e-4)
                        s = (1.0 / B) * (gd or 1.0)
                        ok, w = H.within_ulp(dlog_c[:, :Kc], grad_ref * s, dtype, extra=allow * s)
                        worst_g = max(worst_g, w)
                        assert bool(ok.all()), (tag0, dtype, gd, w)
                        assert bool((dlog_c[:, Kc:] == 0).all()) and not bool(dlog_c.isnan().any())
                        if (eps, lam, bk) == (0.0, 1.0, None):
                            rows_h = torch.full((B,), -5.0, device=DEV)
                            dlog_h = torch.full((B, ld), 7.0, device=DEV, dtype=dtype)
                            K.xent(logits, lab_d, rows_h, None, dlog=dlog_h, gscale=1.0 / B, gdev=gdev)
                            rows_hc, dlog_hc = _sync_cpu(rows_h, dlog_h)
                            n_same += 1
                            same_rows += int(H.same_bits(rows_hc, rows_c))
                            same_dlog += int(H.same_bits(dlog_hc, dlog_c))
                    # dlog=None: the loss is still written; loss=None: the rows are written
                    rows = torch.full((B,), -5.0, device=DEV)
                    loss = torch.full((), -5.0, device=DEV)
                    K.xent_soft(logits, lab_d, rows, loss, labels_b=lab_bd, lam=lam, eps=eps)
                    rows2 = torch.full((B,), -5.0, device=DEV)
                    K.xent_soft(logits, lab_d, rows2, None, labels_b=lab_bd, lam=lam, eps=eps)
                    rows_c, loss_c, rows2_c = _sync_cpu(rows, loss, rows2)
                    torch.testing.assert_close(loss_c.to(F64), rows_ref.mean(), rtol=1e-4, atol=1e-4)
                    assert bool(((rows_c.to(F64) - rows_ref).abs() <= row_bound).all()), tag0
                    assert torch.equal(rows2_c, rows_c)
                assert bool(wide.isnan().sum().item() == B * 8)     # the padding is untouched
    print(f"xent_soft K={Kc}: worst loss_rows err/bound {worst_rows:.3g}, dlog err/bound {worst_g:.3g}; "
          f"at (0, 1, none) bit-equal to xent in loss_rows {same_rows}/{n_same}, dlog {same_dlog}/{n_same}")


def test_xent_soft_refusals():
    """eps = 1, lam = 1.5, a labels_b of another shape or dtype, a missing loss_rows: ValueError
    before the launch, nothing written."""
    K = _k()
    x = torch.zeros(4, 10, device=DEV)
    lab = torch.zeros(4, dtype=torch.long, device=DEV)
    rows = torch.full((4,), -5.0, device=DEV)
    loss = torch.full((), -5.0, device=DEV)
    for kw in (dict(eps=1.0), dict(lam=1.5), dict(lam=-0.25), dict(eps=float("nan")),
               dict(labels_b=torch.zeros(3, dtype=torch.long, device=DEV)),
               dict(labels_b=torch.zeros(4, dtype=torch.int32, device=DEV)),
               dict(dlog=torch.zeros(4, 8, device=DEV, dtype=torch.bfloat16))):
        with pytest.raises(ValueError):
            K.xent_soft(x, lab, rows, loss, **kw)
    with pytest.raises(ValueError):
        K.xent_soft(x, lab, None, loss)
    torch.cuda.synchronize()
    assert bool((rows == -5.0).all()) and float(loss) == -5.0
    K.xent_soft(x, lab, rows, loss, eps=0.1)                 # (the good call does launch)
    torch.cuda.synchronize()
    assert abs(float(loss) - math.log(10.0)) < 1e-5
