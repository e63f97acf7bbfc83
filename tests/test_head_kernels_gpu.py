"""Edge-case numerics of the small kernels at both ends of the step: stem pool / max-pool backward,
tail pool, cross-entropy, top-k, fc bias gradient, fused SGD, 16-bit casts, AMP scan and the
eval-mode BatchNorm coefficients.

Every reference is float64 on the CPU or exact integer logic (tests/head_refs.py, itself checked
against torch in tests/test_head_refs_cpu.py); no kernel of this project serves as a reference.
Bounds: ``ulp_out`` (one spacing of the output dtype at the reference: half for the rounding, half
for a flipped rounding near a tie) for kernels that compute in f32 and round once; the summation
bound n * 2^-23 * sum|terms| for f32 sums; bit equality where the inputs make f32 arithmetic exact.
"""
import math

import pytest
import torch

import head_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
U24 = 2.0 ** -24


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _dev(x64, dtype):
    """float64 reference data (exact in ``dtype``'s f32 superset) -> device tensor of ``dtype``."""
    t = R.to_dtype(x64, dtype)
    assert torch.equal(t.to(F64), x64), "input not representable in the kernel's dtype"
    return t.to(DEV)


def _sync_cpu(*ts):
    torch.cuda.synchronize()
    return [t.cpu() for t in ts]


# ------------------------------------------------------------------ 1. stem pool / max-pool backward
POOL_SHAPES = [(1, 2, 2, 8), (2, 5, 7, 8), (1, 9, 4, 72), (3, 12, 12, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_pool_argmax_and_maxpool_bwd_pixel_exact(shape, dtype):
    """relu(bn(y)) -> 3x3/2/1 max-pool: output bit-equal, argmax bytes byte-equal (first maximum
    in scan order; the quantised inputs tie often), and maxpool_bwd bit-equal to an explicit
    scatter, for the true argmax and for arbitrary valid bytes, with and without a second
    gradient. All inputs are dyadic so every f32 product and sum is exact (checked in f32 and f64
    by head_refs.pool_case)."""
    K = _k()
    N, H, W, C = shape
    c = R.pool_case(*shape)
    Ho, Wo = R.pool_dims(H, W)
    y = _dev(c["y"], dtype)
    sc, sh = _dev(c["sc"], torch.float32), _dev(c["sh"], torch.float32)
    out = torch.full((N, Ho, Wo, C), -7.0, device=DEV, dtype=dtype)
    arg = torch.full((N, Ho, Wo, C), 0xEE, device=DEV, dtype=torch.uint8)
    K.stem_pool(y, sc, sh, out, arg)
    out_c, arg_c = _sync_cpu(out, arg)
    assert R.same_bits(out_c, R.to_dtype(c["out"], dtype))
    assert torch.equal(arg_c, c["arg"])
    dout, dout2 = _dev(c["dout"], dtype), _dev(c["dout2"], dtype)
    for an in ("arg", "fake"):
        a = c[an].to(DEV)
        for two in (False, True):
            din = torch.full((N, H, W, C), 99.0, device=DEV, dtype=dtype)
            K.maxpool_bwd(dout, a, din, dout2=dout2 if two else None)
            (din_c,) = _sync_cpu(din)
            assert R.same_bits(din_c, R.to_dtype(c[("scatter", an, two)], dtype)), (an, two)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", [(2, 5, 7, 8), (3, 12, 12, 64)], ids=lambda s: "x".join(map(str, s)))
def test_stem_bwd_reduce_pixel_exact(shape, dtype):
    """One-pass stem backward: dz bit-equal to scatter * (sc*y+sh > 0) rounded to the dtype (the
    same independent scatter as above, not K.maxpool_bwd), and its per-block partials [G][2][C],
    summed in float64, within n * 2^-23 * sum|terms| (n = N*H*W) of the float64 sums of that
    stored dz and of dz*y."""
    K = _k()
    N, H, W, C = shape
    c = R.pool_case(*shape)
    y = _dev(c["y"], dtype)
    sc, sh = _dev(c["sc"], torch.float32), _dev(c["sh"], torch.float32)
    dout, dout2 = _dev(c["dout"], dtype), _dev(c["dout2"], dtype)
    ws = K.Workspace(DEV)
    for an in ("arg", "fake"):
        a = c[an].to(DEV)
        for two in (False, True):
            dz = torch.full((N, H, W, C), 99.0, device=DEV, dtype=dtype)
            part, G, nq = K.stem_bwd_reduce(ws, dout, a, y, sc, sh, dz, dout2=dout2 if two else None)
            dz_c, part_c = _sync_cpu(dz, part)
            sc64 = c[("scatter", an, two)]
            ref_dz = R.to_dtype(torch.where(c["mask"] > 0, sc64, torch.zeros_like(sc64)), dtype)
            assert R.same_bits(dz_c, ref_dz), (an, two)
            assert nq == 2
            got = part_c[:G * 2 * C].view(G, 2, C).to(F64).sum(0)
            d64 = ref_dz.to(F64)
            n = N * H * W
            for q, terms in enumerate((d64, d64 * c["y"])):
                ref = terms.sum((0, 1, 2))
                bound = n * R.EPS32 * terms.abs().sum((0, 1, 2))
                err = (got[q] - ref).abs()
                print(f"stem_bwd_reduce {shape} {dtype} {an} two={two} q{q}: worst err/bound "
                      f"{float((err / bound.clamp_min(1e-300)).max()):.3g}")
                assert bool((err <= bound).all()), (an, two, q)


# ------------------------------------------------------------------ 2. tail pool
TAIL_SHAPES = [(1, 1, 1, 8), (3, 7, 7, 512), (2, 7, 7, 2048), (2, 5, 10, 2056)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tail_pool_modes_and_second_trip(shape, dtype):
    """mean_hw relu(y*sc+sh + s), s = res (mode 1) or y2*sc2+sh2 (mode 2), against float64, per
    output: |err| <= ulp_out(ref) + HW * 2^-23 * sum|terms|. The inputs make every term exact in
    f32 (head_refs.tail_case checks that in f32 and f64), so the bound covers exactly what the
    kernel rounds: the f32 sum, the 1/HW product and the store. C = 2056 (C/8 = 257) takes the
    kernel's second trip over its 256 threads."""
    K = _k()
    N, H, W, C = shape
    c = R.tail_case(*shape)
    y, r = _dev(c["y"], dtype), _dev(c["res"], dtype)
    sc, sh, sc2, sh2 = (_dev(c[k], torch.float32) for k in ("sc", "sh", "sc2", "sh2"))
    for mode in (1, 2):
        out = torch.full((N, C), -3.0, device=DEV, dtype=dtype)
        if mode == 1:
            K.tail_pool(y, sc, sh, out, res=r)
        else:
            K.tail_pool(y, sc, sh, out, y2=r, scale2=sc2, shift2=sh2)
        (got,) = _sync_cpu(out)
        ok, worst = R.within_ulp(got, c[("ref", mode)], dtype, extra=c[("sumbound", mode)])
        print(f"tail_pool {shape} {dtype} mode {mode}: worst err/bound {worst:.3g}")
        assert bool(ok.all()), (mode, worst)


# ------------------------------------------------------------------ 3. cross-entropy
def _strided_logits(x64, fill, lead=3, trail=5):
    """[B, K] f32 logits as a column slice of a wider buffer whose other columns hold ``fill``."""
    B, Kc = x64.shape
    wide = torch.full((B, lead + Kc + trail), fill, dtype=torch.float32)
    wide[:, lead:lead + Kc] = x64.float()
    wide = wide.to(DEV)
    view = wide[:, lead:lead + Kc]
    assert view.stride(0) > Kc
    return wide, view


def _xent_labels(B, Kc, g, flip):
    lab = torch.randint(0, Kc, (B,), generator=g)
    lab[0] = 0 if (B == 1 and flip) else Kc - 1
    if B > 1:
        lab[B - 1] = 0
    return lab


@pytest.mark.parametrize("Kc", [10, 63, 64, 65, 1000])
def test_xent_edges(Kc):
    """xent over B in {1,4,5,37}, strided NaN-padded logits, dlog [B, ld] bf16 / fp16 (ld = K
    rounded up to 64, and 1024) pre-filled with a sentinel, labels forced to 0 and K-1, logits
    x3, x30 (peaked) and x3 + 100, gscale = 1/B, with and without the device loss scale 65536.

    loss_rows: |err| <= 1e-5*|ref| + 4 * 2^-23 * max(1, max|logit|) (rounding of m + log s).
    dlog[:, :K]: within ulp_out of float64 (softmax - onehot) * gscale * gdev; columns >= K are 0.

    Two allowances in dlog are derived from the kernel's formula g = (e_k / s - [k == label]) *
    gscale * gdev with e_k = __expf(x_k - m), none from its output:
    - The hardware exponential flushes a result below the smallest f32 normal to zero, so p = e / s
      carries an absolute error of up to 2^-126: the bound adds 2^-126 * gscale * gdev. It shows
      only in bf16 dlog on the peaked rows, where the reference gradient itself is below 1.2e-38.
    - At the label the kernel subtracts 1 from p in f32. When p -> 1 (peaked rows) the difference
      cancels and the relative error eps_p of p survives as an absolute error eps_p * p. The f32
      forward error of p is eps_p <= 2^-24 * (13 + 2|x_label - m| + 2 ln K + ceil(K/64)): 2 for
      the exponential (1 ulp) and 2|x_label - m| for the roundings of x - m and of its product
      with log2 e; for s the same per term, weighted by p_k (sum p_k (m - x_k) <= ln K), plus
      ceil(K/64) + 6 additions; 2 for the reciprocal, 1 for the product. The bound adds
      eps_p * p_label * gscale * gdev at the label column only (about 2e-6 of the scale at
      K = 1000); every other entry keeps the plain ulp_out bound."""
    K = _k()
    g = R._gen(Kc)
    worst_rows = worst_g = worst_0 = 0.0
    for B in (1, 4, 5, 37):
        base = torch.randn(B, Kc, generator=g, dtype=F64)
        for vi, x64 in enumerate((base * 3, base * 30, base * 3 + 100)):
            x64 = x64.float().to(F64)            # the kernel's f32 inputs, exactly
            for li, ld in enumerate(sorted({(Kc + 63) // 64 * 64, 1024})):
                labels = _xent_labels(B, Kc, g, flip=li == 1)
                rows_ref, grad_ref = R.xent_ref(x64, labels)
                wide, logits = _strided_logits(x64, float("nan"))
                lab_d = labels.to(DEV)
                row_bound = 1e-5 * rows_ref.abs() + 4 * R.EPS32 * max(1.0, float(x64.abs().max()))
                # derived allowances (docstring), in units of gscale * gdev
                ar = torch.arange(B)
                eps_p = U24 * (13 + 2 * (x64.max(1).values - x64[ar, labels]) + 2 * math.log(Kc)
                               + -(-Kc // 64))
                allow = torch.full_like(grad_ref, 2.0 ** -126)
                allow[ar, labels] += eps_p * (grad_ref[ar, labels] + 1.0)
                for dtype, gd in ((torch.bfloat16, None), (torch.float16, None), (torch.float16, 65536.0)):
                    rows = torch.full((B,), -5.0, device=DEV)
                    loss = torch.full((), -5.0, device=DEV)
                    dlog = torch.full((B, ld), 7.0, device=DEV, dtype=dtype)
                    gdev = torch.tensor([gd], device=DEV) if gd else None
                    K.xent(logits, lab_d, rows, loss, dlog=dlog, gscale=1.0 / B, gdev=gdev)
                    rows_c, loss_c, dlog_c = _sync_cpu(rows, loss, dlog)
                    err = (rows_c.to(F64) - rows_ref).abs()
                    worst_rows = max(worst_rows, float((err / row_bound).max()))
                    assert bool((err <= row_bound).all()), (B, vi, ld, dtype, gd)
                    torch.testing.assert_close(loss_c.to(F64), rows_ref.mean(), rtol=1e-4, atol=1e-4)
                    s = (1.0 / B) * (gd or 1.0)
                    ok, w = R.within_ulp(dlog_c[:, :Kc], grad_ref * s, dtype, extra=allow * s)
                    worst_g = max(worst_g, w)
                    worst_0 = max(worst_0, R.within_ulp(dlog_c[:, :Kc], grad_ref * s, dtype)[1])
                    assert bool(ok.all()), (B, vi, ld, dtype, gd, w)
                    assert bool((dlog_c[:, Kc:] == 0).all()) and not bool(dlog_c.isnan().any())
                # dlog=None: the loss is still written; loss=None: the rows are written
                rows = torch.full((B,), -5.0, device=DEV)
                loss = torch.full((), -5.0, device=DEV)
                K.xent(logits, lab_d, rows, loss)
                rows2 = torch.full((B,), -5.0, device=DEV)
                K.xent(logits, lab_d, rows2, None)
                rows_c, loss_c, rows2_c = _sync_cpu(rows, loss, rows2)
                torch.testing.assert_close(loss_c.to(F64), rows_ref.mean(), rtol=1e-4, atol=1e-4)
                assert bool(((rows_c.to(F64) - rows_ref).abs() <= row_bound).all())
                assert torch.equal(rows2_c, rows_c)
                assert bool(wide.isnan().sum().item() == B * 8)     # the padding is untouched
    print(f"xent K={Kc}: worst loss_rows err/bound {worst_rows:.3g}, dlog err/bound {worst_g:.3g} "
          f"(plain ulp_out alone {worst_0:.3g})")


def test_xent_rejects_missing_loss_rows():
    """The kernel always writes loss_rows: the wrapper refuses None instead of launching."""
    K = _k()
    with pytest.raises(ValueError):
        K.xent(torch.zeros(2, 4, device=DEV), torch.zeros(2, dtype=torch.long, device=DEV), None, None)


# ------------------------------------------------------------------ 4. top-k
def _topk_rows(Kc, g):
    """Rows of tie-dense logits with their labels: small-integer draws, all-equal rows, rows with
    exactly 4 / exactly 5 strictly greater entries, duplicates of the label's value below and
    above its index."""
    rows, labs = [], []
    for lab in range(min(7, Kc)):                       # all-equal rows, labels 0..6
        rows.append(torch.full((Kc,), 2.0))
        labs.append(lab)
    for ngt in (4, 5):                                  # exactly ngt strictly greater
        if Kc - 1 >= ngt:
            for lab in (0, Kc - 1, Kc // 2):
                r = torch.zeros(Kc)
                r[lab] = 1.0
                others = [i for i in range(Kc) if i != lab]
                pick = torch.randperm(len(others), generator=g)[:ngt].tolist()
                for i in pick:
                    r[others[i]] = 3.0
                rows.append(r)
                labs.append(lab)
    lab = Kc // 2                                       # duplicates of the label's value
    for lower, higher in ((4, 0), (5, 0), (0, 6), (3, 1), (4, 3), (1, 0), (0, 1)):
        if lower <= lab and higher <= Kc - lab - 1:
            r = torch.full((Kc,), -1.0)
            r[lab] = 5.0
            lo = torch.randperm(lab, generator=g)[:lower].tolist()
            hi = (lab + 1 + torch.randperm(Kc - lab - 1, generator=g)[:higher]).tolist()
            assert len(lo) == lower and len(hi) == higher
            r[lo + hi] = 5.0
            rows.append(r)
            labs.append(lab)
    return rows, labs


@pytest.mark.parametrize("Kc", [3, 5, 65, 1000])
def test_topk_hits_ties(Kc):
    """Top-1 / top-5 counters against exact integer logic on tie-dense logits (an untrained or
    collapsed network ties exactly): lower index first. The logits are a strided view whose
    padding columns hold +inf (NaN would compare false both ways and hide a read past K);
    ``hits`` starts non-zero because the kernel accumulates."""
    K = _k()
    g = R._gen(100 + Kc)
    crafted, clabs = _topk_rows(Kc, g)
    for B in (1, 5, 257):
        x = torch.randint(-2, 3, (B, Kc), generator=g).float()
        labels = torch.randint(0, Kc, (B,), generator=g)
        n = min(B, len(crafted))
        off = 0 if B != 5 else 7 % max(1, len(crafted) - n + 1)
        for i in range(n):
            x[i] = crafted[off + i]
            labels[i] = clabs[off + i]
        t1, t5 = R.topk_ref(x, labels)
        _, view = _strided_logits(x.to(F64), float("inf"))
        hits = torch.tensor([11.0, 23.0], device=DEV)
        K.topk_hits(view, labels.to(DEV), hits)
        (h,) = _sync_cpu(hits)
        assert h.tolist() == [11.0 + t1, 23.0 + t5], (B, h.tolist(), t1, t5)


# ------------------------------------------------------------------ 5. col_sum
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("C", [10, 64, 1000])
def test_col_sum_edges(C, dtype):
    """fc bias gradient: out[c] = scale * sum_r x[r][c] (+ out[c]) against float64 within the
    summation bound rows * 2^-23 * sum|terms| (terms = scale * x[r][c]; accumulate adds one f32
    rounding of the result). Columns >= C of x are NaN; out is longer than C and the sentinel
    behind C must survive."""
    K = _k()
    g = R._gen(C)
    worst = 0.0
    for rows in (1, 15, 16, 17, 400):
        for ld in sorted({C, 1024}):
            x = torch.full((rows, ld), float("nan"), dtype=dtype)
            x[:, :C] = torch.randn(rows, C, generator=g).to(dtype)
            x_d = x.to(DEV)
            x64 = x[:, :C].to(F64)
            for scale in (1.0, 1.0 / 400):
                sc32 = float(torch.tensor(scale, dtype=torch.float32))   # the kernel's argument
                terms = x64 * sc32
                for acc in (False, True):
                    pre = torch.randn(C + 5, generator=g)
                    pre[C:] = -77.0
                    out = pre.to(DEV)
                    K.col_sum(x_d, C, out, scale=scale, accumulate=acc)
                    (got,) = _sync_cpu(out)
                    ref = terms.sum(0) + (pre[:C].to(F64) if acc else 0.0)
                    bound = rows * R.EPS32 * terms.abs().sum(0)
                    if acc:
                        bound = bound + R.ulp_out(ref, torch.float32)
                    err = (got[:C].to(F64) - ref).abs()
                    worst = max(worst, float((err / bound).max()))
                    assert bool((err <= bound).all()), (rows, ld, scale, acc)
                    assert bool((got[C:] == -77.0).all())
    print(f"col_sum C={C} {dtype}: worst err/bound {worst:.3g}")


# ------------------------------------------------------------------ 6. casts and SGD
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cast_flat_bit_exact(dtype):
    """cast_flat == torch's CPU cast, bit for bit (NaN as 'is NaN'), on the edge vector of
    head_refs.cast_edge_values followed by random data; n = 1, 255, and 2,097,152 + 257 (one
    grid-stride trip past the 8192 x 256 cap plus a ragged end). Elements behind n stay."""
    K = _k()
    n_big = 2097152 + 257
    src = R.cast_input(n_big)
    src_d = src.to(DEV)
    for n in (1, 255, n_big):
        out = torch.full((n + 3,), 9.0, device=DEV, dtype=dtype)
        K.cast_flat(src_d[:n], out[:n])
        (got,) = _sync_cpu(out)
        ok = R.cast_matches(got[:n], src[:n])
        bad = (~ok).nonzero().flatten()[:8].tolist()
        assert not bad, (n, bad, [src[i].item() for i in bad], [got[i].item() for i in bad])
        assert bool((got[n:] == 9.0).all())


SGD_CFGS = [(0.9, 1e-4, None), (0.0, 1e-4, None), (0.9, 0.0, None), (0.9, 1e-4, 0.25)]


def _sgd_inputs(n, g):
    p = torch.randn(n, generator=g)
    edge = torch.tensor([7.0e4, 2.0e-6, -1.0e5, 3.1e-7, 65520.0, -5.0e-8, 6.0e-5])
    k = min(n, edge.numel())
    p[:k] = edge[:k]
    if n > 100:
        p[-3:] = torch.tensor([-8.0e4, 4.0e-7, 66000.0])      # the ragged tail too
    return p, torch.randn(n, generator=g)


def _sgd_check(K, n, shadow_dtype, momentum, wd, inv, g):
    lr = 0.1
    p0, g0 = _sgd_inputs(n, g)
    ref = R.sgd_ref(p0, g0, 3, lr, momentum, wd, inv if inv is not None else 1.0)
    p, gr = p0.to(DEV), g0.to(DEV)
    buf = torch.full((n,), float("nan"), device=DEV)      # stale: the first step must not read it
    sh = torch.full((n,), 3.0, device=DEV, dtype=shadow_dtype) if shadow_dtype else None
    inv_d = torch.tensor([inv], device=DEV) if inv is not None else None
    zero = torch.zeros(1, device=DEV) if inv is not None else None
    for it in range(3):
        K.sgd_flat(p, gr, buf, sh, lr, momentum, wd, initialized=it > 0, inv_scale=inv_d,
                   found_inf=zero)
        p_c, b_c = _sync_cpu(p, buf)
        tag = (n, shadow_dtype, momentum, wd, inv, it)
        assert bool(p_c.isfinite().all()) and bool(b_c.isfinite().all()), tag
        torch.testing.assert_close(p_c.to(F64), ref[it][0], rtol=1e-6, atol=1e-6, msg=str(tag))
        torch.testing.assert_close(b_c.to(F64), ref[it][1], rtol=1e-6, atol=1e-6, msg=str(tag))
        if sh is not None:      # the shadow is the cast of the kernel's own updated p
            (s_c,) = _sync_cpu(sh)
            assert bool(R.cast_matches(s_c, p_c).all()), tag
    # overflow step: nothing moves, bit for bit
    one = torch.ones(1, device=DEV)
    before = [t.clone() for t in (p, buf) + ((sh,) if sh is not None else ())]
    K.sgd_flat(p, gr, buf, sh, lr, momentum, wd, initialized=True, inv_scale=inv_d, found_inf=one)
    torch.cuda.synchronize()
    for a, b in zip(before, (p, buf) + ((sh,) if sh is not None else ())):
        assert R.same_bits(a, b), (n, shadow_dtype, momentum, wd, inv)


@pytest.mark.parametrize("shadow", [torch.bfloat16, torch.float16, None], ids=["bf16", "fp16", "none"])
def test_sgd_flat_small_sizes_and_flags(shadow):
    """n = 1..7 (tail only, n % 4 in {0,1,2,3}), three steps against the float64 torch-SGD
    emulation at rtol = atol = 1e-6 for p and buf: momentum 0, weight decay 0, inv_scale, a first
    step over a NaN momentum buffer, p holding fp16-overflowing and fp16-subnormal values (the
    shadow bit-equals torch's cast of the updated p), and found_inf leaving p, buf and the shadow
    bit-unchanged."""
    K = _k()
    g = R._gen(3)
    for n in (1, 2, 3, 4, 5, 7):
        for momentum, wd, inv in SGD_CFGS:
            _sgd_check(K, n, shadow, momentum, wd, inv, g)


def test_sgd_flat_past_the_grid_cap():
    """n = 8,388,608 + 4*256 + 3: the vec4 loop passes its 8192-block cap (a second grid-stride
    trip for one block's worth of quads) and leaves a 3-element tail; a single launch per step."""
    K = _k()
    _sgd_check(K, 8388608 + 4 * 256 + 3, torch.bfloat16, 0.9, 1e-4, None, R._gen(4))


# ------------------------------------------------------------------ 7. amp_scan additions
def test_amp_scan_small_untracked_and_growth_overflow():
    """n = 4; tracker=None publishes found_inf and 1/scale and leaves the scale alone; a growth
    step whose product overflows (2e38 * 2) keeps the scale and resets the tracker, as
    torch._amp_update_scale_ does. The arrival workspace reads [0, 0] after every launch."""
    K = _k()
    ws = torch.zeros(2, dtype=torch.int32, device=DEV)
    fi, inv = torch.full((1,), 5.0, device=DEV), torch.full((1,), 5.0, device=DEV)
    for bad in (None, float("inf"), float("nan")):
        for pos in range(4):
            gg = torch.tensor([1.0, -2.0, 3.0e38, 0.0], device=DEV)
            if bad is not None:
                gg[pos] = bad
            # untracked: scale untouched
            scale = torch.tensor([1024.0], device=DEV)
            K.amp_scan(gg, fi, inv, scale, None, ws, 2.0, 0.5, 1)
            torch.cuda.synchronize()
            assert fi.item() == (0.0 if bad is None else 1.0)
            assert inv.item() == 1.0 / 1024 and scale.item() == 1024.0
            assert ws.tolist() == [0, 0]
            # tracked, against torch's own state machine (interval 2: second clean step grows)
            scale, tracker = torch.tensor([2.0e38], device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
            s_ref, t_ref = scale.clone(), tracker.clone()
            fr = torch.tensor([0.0 if bad is None else 1.0], device=DEV)
            inv_ref = s_ref.double().reciprocal().float()
            K.amp_scan(gg, fi, inv, scale, tracker, ws, 2.0, 0.5, 2)
            torch._amp_update_scale_(s_ref, t_ref, fr, 2.0, 0.5, 2)
            torch.cuda.synchronize()
            assert fi.item() == fr.item()
            assert inv.item() == inv_ref.item()
            assert scale.item() == s_ref.item() and tracker.item() == t_ref.item()
            if bad is None:     # the guarded growth: scale kept, tracker reset
                assert scale.item() == float(torch.tensor(2.0e38)) and tracker.item() == 0
            assert ws.tolist() == [0, 0]


# ------------------------------------------------------------------ 8. bn_eval_coeffs
@pytest.mark.parametrize("C", [1, 64, 255, 257, 2048])
def test_bn_eval_coeffs(C):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale against float64, with var
    holding 0 and 1e4 and gamma holding 0 and negative values.

    Yardstick: torch's float32 rsqrt(var + eps) on the CPU against float64 measures 5.4e-8 to
    9.7e-8 relative on these inputs (the f32 add's rounding included; computed again below, never
    from the kernel). The kernel gets twice that plus the two f32 multiplications (2 * 2^-24):
    |scale err| <= tol * |scale|, |shift err| <= tol * |mean * scale| + ulp_f32(shift), the last
    term being the rounding of the final subtraction. Entries beyond C stay untouched."""
    K = _k()
    g = R._gen(C)
    eps = 1e-5
    var = torch.rand(C, generator=g) * 2 + 0.01
    gamma = torch.randn(C, generator=g)
    var[0] = 0.0
    gamma[C // 2] = -1.5
    if C > 1:
        var[1], var[C - 1] = 1e4, 0.0
        gamma[0], gamma[C - 1] = 0.0, -0.25
    beta, mean = torch.randn(C, generator=g), torch.randn(C, generator=g) * 3
    yard = R.rsqrt_yardstick(var, eps)
    assert 0 < yard < 2.0 ** -22
    tol = 2 * yard + 2 * U24
    sc_ref, sh_ref = R.bn_eval_ref(gamma, beta, mean, var, float(torch.tensor(eps, dtype=torch.float32)))
    scale = torch.full((C + 4,), -9.0, device=DEV)
    shift = torch.full((C + 4,), -9.0, device=DEV)
    K.bn_eval_coeffs(gamma.to(DEV), beta.to(DEV), mean.to(DEV), var.to(DEV), eps, scale, shift)
    sc, sh = _sync_cpu(scale, shift)
    e_sc = (sc[:C].to(F64) - sc_ref).abs()
    e_sh = (sh[:C].to(F64) - sh_ref).abs()
    b_sh = tol * (mean.to(F64) * sc_ref).abs() + R.ulp_out(sh_ref, torch.float32)
    print(f"bn_eval_coeffs C={C}: yardstick {yard:.3g}, worst scale rel err "
          f"{float((e_sc / sc_ref.abs().clamp_min(1e-300)).max()):.3g}, shift err/bound "
          f"{float((e_sh / b_sh).max()):.3g}")
    assert bool((e_sc <= tol * sc_ref.abs()).all())
    assert bool((e_sh <= b_sh).all())
    assert bool((sc[C:] == -9.0).all()) and bool((sh[C:] == -9.0).all())
