"""batch_mix (csrc/mix.hip): mixup and CutMix of a finished batch, in both layouts, against the
index-arithmetic reference of tests/mix_refs.py (checked on the CPU in tests/test_mix_refs_cpu.py)."""
import functools

import pytest
import torch

import head_refs as H
import mix_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
U24 = 2.0 ** -24
GUARD = 64           # elements on each side of ``out`` (a multiple of 16 bytes in every dtype)

CASES = ([(R.S2D, dt, S) for dt in (torch.float32, torch.bfloat16, torch.float16) for S in (4, 10, 32)]
         + [(R.NCHW, torch.float32, S) for S in (4, 6, 10, 32)])   # 4: rows of 16 bytes
IDS = [f"{'s2d' if l == R.S2D else 'nchw'}-{str(dt).split('.')[1]}-S{S}" for l, dt, S in CASES]


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


@functools.lru_cache(maxsize=None)
def _input(layout, dtype, S, B):
    """Random images with -0, +0, the largest finite value of both signs and (in one sample) a NaN
    planted at pixels of every row / column parity. Treat as read-only."""
    g = H._gen(100 * S + 10 * B + layout)
    img = torch.randn(B, 3, S, S, generator=g).to(dtype)
    fmax = torch.finfo(dtype).max
    img[0, 0, 0, 0] = -0.0
    img[0, 1, 1, 1] = 0.0
    img[0, 2, 1, 0] = -fmax
    img[B - 1, 2, S - 1, S - 1] = fmax
    img[B - 1, 0, 0, 1] = -0.0
    img[min(1, B - 1), 1, 1, S - 1] = float("nan")
    return R.s2d_from_nchw(img) if layout == R.S2D else img


def _boxes(S):
    return {"empty": (1, 1, 0, S), "whole": (0, S, 0, S), "odd pixel": (1, 2, 3, 4),
            "flush with 0": (0, 2, 0, 3), "flush with S": (S - 3, S, S - 2, S),
            "one row": (2, 3, 0, S), "one column": (1, S - 1, 1, 2)}


def _run(K, x_cpu, layout, mode, lam, box, grid_cap=0):
    """batch_mix into the middle of a sentinel-filled buffer; returns the output on the CPU after
    checking the guard bands and that the input kept its bits."""
    x = x_cpu.to(DEV)
    n = x.numel()
    big = torch.full((n + 2 * GUARD,), 7.0, dtype=x.dtype, device=DEV)
    out = big[GUARD:GUARD + n].view(x.shape)
    assert out.data_ptr() % 16 == 0
    if grid_cap:     # the launcher itself, validated like the wrapper's call, with a capped grid
        from pytorch_distributed_amd.ops import ext
        _, S, bx = K.batch_mix_check(x, out, layout, mode, lam, box)
        rc = ext.lib().pda_batch_mix(x.data_ptr(), out.data_ptr(), x.shape[0], S, ext.dt_of(x), layout,
                                     mode, *K.mix_weights(lam), *bx, grid_cap,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        K.batch_mix(x, out, layout, mode, lam, box)
    torch.cuda.synchronize()
    big_c = big.cpu()
    fresh = torch.full((GUARD,), 7.0, dtype=x.dtype)
    assert H.same_bits(big_c[:GUARD], fresh) and H.same_bits(big_c[GUARD + n:], fresh), "guard band written"
    assert H.same_bits(x.cpu(), x_cpu), "the input was written"
    return big_c[GUARD:GUARD + n].view(x.shape)


def _pads_zero(out, layout):
    if layout == R.S2D:
        it = {2: torch.int16, 4: torch.int32}[out.element_size()]
        assert int(torch.count_nonzero(out[..., 12:].contiguous().view(it))) == 0, "slots 12..15"


@pytest.mark.parametrize("layout,dtype,S", CASES, ids=IDS)
def test_cutmix_is_a_bit_exact_select(layout, dtype, S):
    """B in {1, 2, 3, 5} x seven boxes: the empty box, the whole image, one pixel at odd (y, x) (it
    splits an s2d 2x2 group), boxes flush with row / column 0 and with S, one row, one column. The
    output bit-equals the reference (the NaN and the signed zeros travel with their pixels), the
    guard bands and the input are intact, s2d slots 12..15 stay 0."""
    K = _k()
    for B in (1, 2, 3, 5):
        x = _input(layout, dtype, S, B)
        for name, box in _boxes(S).items():
            ref = R.batch_mix_ref(x, layout, R.CUTMIX, 0.5, box)
            out = _run(K, x, layout, K.MIX_CUTMIX, 0.5, box)
            assert H.same_bits(out, ref), (B, name, box)
            _pads_zero(out, layout)
            if name == "empty":
                assert H.same_bits(out, x)
            if name == "whole":
                assert H.same_bits(out, x.roll(1, 0))
        if B == 5:      # two blocks in all: both grid-stride loops iterate
            box = _boxes(S)["odd pixel"]
            out = _run(K, x, layout, K.MIX_CUTMIX, 0.5, box, grid_cap=2)
            assert H.same_bits(out, R.batch_mix_ref(x, layout, R.CUTMIX, 0.5, box))


@pytest.mark.parametrize("layout,dtype,S", CASES, ids=IDS)
def test_mixup_within_the_f32_bound(layout, dtype, S):
    """B in {1, 2, 5}, lam in {0, 1, 0.5, 0.3}. The kernel evaluates lam*a + (1-lam)*b in f32 (two
    products and one sum, or a product and a fused multiply-add: at most three roundings of
    relative size 2^-24) and rounds once to the output dtype:
    |err| <= ulp_out(ref) + 3 * 2^-24 * (|lam*a| + |(1-lam)*b|), against the float64 value at the
    float32 weights the kernel receives. At lam = 1 and lam = 0 the output equals x[b] and the
    partner as numbers (a -0 may come out as +0). A NaN comes out wherever either source has one
    (0 * NaN is NaN), and nowhere else."""
    K = _k()
    worst = 0.0
    for B in (1, 2, 5):
        x = _input(layout, dtype, S, B)
        part = x.roll(1, 0)
        for lam in (0.0, 1.0, 0.5, 0.3):
            for cap in ((0, 2) if (B == 5 and lam == 0.3) else (0,)):
                ref = R.batch_mix_ref(x, layout, R.MIXUP, lam, None)
                out = _run(K, x, layout, K.MIX_MIXUP, lam, None, grid_cap=cap)
                nan = x.isnan() | part.isnan()
                assert torch.equal(ref.isnan(), nan) and torch.equal(out.isnan(), nan), (B, lam)
                _pads_zero(out, layout)
                fin = ~nan
                if lam in (0.0, 1.0):
                    src = x if lam == 1.0 else part
                    assert bool((out[fin] == src[fin]).all()), (B, lam)
                    continue
                lam32, oml32 = R.f32_weights(lam)
                extra = 3 * U24 * ((lam32 * x.to(F64)).abs() + (oml32 * part.to(F64)).abs())
                ok, w = H.within_ulp(out[fin], ref[fin], dtype, extra=extra[fin])
                worst = max(worst, w)
                assert bool(ok.all()), (B, lam, cap, w)
    print(f"batch_mix mixup {IDS[CASES.index((layout, dtype, S))]}: worst err/bound {worst:.3g}")


def test_batch_mix_refusals():
    """An aliasing or overlapping out, a box outside the image, the NCHW layout in bf16, another
    shape for out: ValueError before the launch. An odd S cannot be written as an s2d shape
    ([B, S/2, S/2, 16]); the launcher itself, which takes S, returns -2 for it and launches nothing."""
    from pytorch_distributed_amd.ops import ext
    K = _k()
    s = torch.ones(2, 4, 4, 16, device=DEV, dtype=torch.bfloat16)
    o = torch.full_like(s, 7.0)
    n = torch.ones(2, 3, 8, 8, device=DEV)
    on = torch.full_like(n, 7.0)
    flat = torch.ones(2 * s.numel(), device=DEV, dtype=torch.bfloat16)
    over = (flat[:s.numel()].view(s.shape), flat[s.numel() // 2:s.numel() // 2 + s.numel()].view(s.shape))
    bad = [
        (s, s, K.AUG_S2D, K.MIX_MIXUP, 0.5, None),
        (over[0], over[1], K.AUG_S2D, K.MIX_MIXUP, 0.5, None),
        (s, o, K.AUG_S2D, K.MIX_CUTMIX, 0.5, (0, 9, 0, 8)),
        (s, o, K.AUG_S2D, K.MIX_CUTMIX, 0.5, (-1, 4, 0, 8)),
        (s, o, K.AUG_S2D, K.MIX_CUTMIX, 0.5, (0, 8, 5, 4)),
        (n, on, K.AUG_NCHW, K.MIX_CUTMIX, 0.5, (0, 8, 0, 9)),
        (n.bfloat16(), on.bfloat16(), K.AUG_NCHW, K.MIX_MIXUP, 0.5, None),
        (n, on[:, :, :6, :6].contiguous(), K.AUG_NCHW, K.MIX_MIXUP, 0.5, None),
        (s, o, K.AUG_S2D, K.MIX_MIXUP, 1.5, None),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            K.batch_mix(*args)
    rc = ext.lib().pda_batch_mix(s.data_ptr(), o.data_ptr(), 2, 7, 1, K.AUG_S2D, K.MIX_MIXUP, 0.5, 0.5,
                                 0, 0, 0, 0, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -2
    # pointers that are not 16-byte aligned: refused by the wrapper and by the launcher, in both layouts
    pool = torch.ones(n.numel() + 4, device=DEV)
    odd = pool[1:1 + n.numel()].view(n.shape)
    with pytest.raises(ValueError, match="aligned"):
        K.batch_mix(odd, on, K.AUG_NCHW, K.MIX_MIXUP, 0.5)
    for layout, a, b, side, dt in ((K.AUG_NCHW, odd, on, 8, 0), (K.AUG_S2D, s, o, 8, 1)):
        rc = ext.lib().pda_batch_mix(a.data_ptr() + (0 if layout == K.AUG_NCHW else 2), b.data_ptr(),
                                     2, side, dt, layout, K.MIX_MIXUP, 0.5, 0.5, 0, 0, 0, 0, 0,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == -2
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((on == 7.0).all())
    K.batch_mix(s, o, K.AUG_S2D, K.MIX_MIXUP, 0.5)           # (the good call does launch)
    torch.cuda.synchronize()
    assert bool((o == 1.0).all())
