"""The gradient-clip kernel on the GPU (csrc/clip.hip) against tests/clip_refs.py.

Tables: "sizes" -- segments of 1, 3, 4, 5, SEG_CHUNK - 1, SEG_CHUNK, SEG_CHUNK + 1 and 2 * SEG_CHUNK + 2
elements with unowned gaps in front, between and behind; "many" -- 640 one-chunk segments, so the
last block has more slab entries than threads and its stride loop iterates. Unowned elements hold
NaN in every test: any result that is not NaN proves they were not read.

Bounds. Integer data (|g| <= 2, sum of squares a perfect square): every double sum and the sqrt
are exact, so out[0] and out[1] bit-equal the reference. Generic data: the double accumulation and
the double sqrt each err by at most one unit in the last place of double, which moves the float32
rounding by at most one step -- out[0] within one float32 ulp of the float64 norm rounded to
float32. The update fed the kernel's coefficient bit-equals the same launch fed the reference
coefficient from the host, and meets the float64 reference at rtol = atol = 1e-6, the bound of
tests/test_optim_gpu.py.
"""
import functools
import math

import numpy as np
import pytest
import torch

import clip_refs as CR
import head_refs as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
INV = 2.0 ** -7
CANARY64 = 0x7FF8BEEF0BADF00D
CANARY32 = 0x7FC0BEEF


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _layout(name):
    """(n, [(offset, size)]): segments with gaps of at least 4 unowned elements around each."""
    S = _k().SEG_CHUNK
    assert S == 4096
    sizes = {"sizes": [1, 3, 4, 5, S - 1, S, S + 1, 2 * S + 2],
             "many": [1 + (i * 7) % 11 for i in range(640)]}[name]
    off, segs = 4, []
    for size in sizes:
        segs.append((off, size))
        off = (off + size + 3) // 4 * 4 + 4
    return off, segs


@functools.lru_cache(maxsize=None)
def _tables(name):
    K = _k()
    n, segs = _layout(name)
    t, nblk = K.seg_tables(segs, [{"lr": 0.0}] * len(segs), DEV)
    assert nblk == sum(-(-s // K.SEG_CHUNK) for _, s in segs)
    return t


def _fill(name, values):
    """NaN everywhere, ``values`` (1-D, as long as the segments together) inside the segments."""
    n, segs = _layout(name)
    g = torch.full((n,), float("nan"))
    at = 0
    for off, size in segs:
        g[off:off + size] = values[at:at + size]
        at += size
    assert at == values.numel()
    return g


def _square_ints(total, seed=21):
    """``total`` integers in [-2, 2] whose sum of squares is a perfect square (zeros turned into +-1
    until it is), as float32, and the root."""
    v = torch.randint(-2, 3, (total,), generator=H._gen(seed))
    s = int((v * v).sum())
    root = math.isqrt(s - 1) + 1
    need = root * root - s
    zeros = (v == 0).nonzero().flatten()
    assert 0 <= need <= zeros.numel()
    v[zeros[:need]] = torch.tensor([1, -1]).repeat(need // 2 + 1)[:need]
    assert int((v * v).sum()) == root * root
    return v.to(torch.float32), root


@functools.lru_cache(maxsize=None)
def _integer_gradient(name):
    n, segs = _layout(name)
    v, root = _square_ints(sum(s for _, s in segs))
    return _fill(name, v), root


@functools.lru_cache(maxsize=None)
def _float_gradient(name):
    n, segs = _layout(name)
    return _fill(name, torch.randn(sum(s for _, s in segs), generator=H._gen(22)) * 0.37)


class _Bufs:
    """slab, cnt and out inside larger canary-filled buffers (guard bands of 8 / 4 elements)."""

    def __init__(self, nblk):
        self.slab_all = torch.full((nblk + 16,), CANARY64, dtype=torch.int64).view(F64).to(DEV)
        self.out_all = torch.full((10,), CANARY32, dtype=torch.int64).to(torch.int32).view(
            torch.float32).to(DEV)
        self.slab, self.out = self.slab_all[8:8 + nblk], self.out_all[4:6]
        self.cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.nblk = nblk

    def guards_intact(self):
        s, o = _bits(self.slab_all), _bits(self.out_all)
        return (bool((s[:8] == CANARY64).all()) and bool((s[8 + self.nblk:] == CANARY64).all())
                and bool((o[:4] == CANARY32).all()) and bool((o[6:] == CANARY32).all()))

    def untouched(self):
        return (self.guards_intact() and bool((_bits(self.slab) == CANARY64).all())
                and bool((_bits(self.out) == CANARY32).all()) and int(self.cnt.item()) == 0)


def _launch(name, g, max_norm, inv=None, found=None, bufs=None):
    K = _k()
    t = _tables(name)
    b = bufs or _Bufs(t.nblocks)
    inv_d = torch.tensor([inv], dtype=torch.float32, device=DEV) if inv is not None else None
    found_d = torch.tensor([found], dtype=torch.float32, device=DEV) if found is not None else None
    K.grad_clip(g, t, max_norm, b.slab, b.cnt, b.out, inv_scale=inv_d, found_inf=found_d)
    torch.cuda.synchronize()
    return b


def _same32(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.int32) == b.view(np.int32))


# ------------------------------------------------------------------ norms and coefficients
@pytest.mark.parametrize("inv", [None, INV], ids=["noinv", "inv"])
@pytest.mark.parametrize("name", ["sizes", "many"])
def test_integer_data_gives_exact_norm_and_coefficient(name, inv):
    g, root = _integer_gradient(name)
    n, segs = _layout(name)
    inv1 = 1.0 if inv is None else inv
    for max_norm in (1.0, 0.37, 1e9):
        b = _launch(name, g.to(DEV), max_norm, inv)
        out = b.out.cpu().numpy()
        want_norm = CR.norm32(g, segs, inv1)
        assert float(want_norm) == root * inv1              # exact by construction
        want = CR.scale32(g, segs, max_norm, inv1)
        print(f"{name} inv={inv} max_norm={max_norm}: out={out.tolist()} want=({want_norm}, {want})")
        assert _same32(out[0], want_norm) and _same32(out[1], want)
        assert b.guards_intact() and int(b.cnt.item()) == 0
    assert float(want) == inv1                              # max_norm far above: coefficient 1


@pytest.mark.parametrize("name", ["sizes", "many"])
def test_float_data_within_one_ulp_guards_counter_and_repeat(name):
    g = _float_gradient(name)
    n, segs = _layout(name)
    gd = g.to(DEV)
    b = _launch(name, gd, 1.0)
    first = (_bits(b.out).clone(), _bits(b.slab).clone())
    want = CR.norm32(g, segs)
    got = np.float32(b.out[0].item())
    ulps = abs(int(got.view(np.int32)) - int(want.view(np.int32)))
    print(f"{name}: norm {got!r} want {want!r} ({ulps} ulp), scale {b.out[1].item()!r}")
    assert ulps <= 1
    assert _same32(b.out[1].item(), CR.coef32(got, 1.0))     # the coefficient of the published norm
    assert bool(b.slab.isfinite().all()) and bool((b.slab >= 0).all())
    assert float(b.slab.sum().sqrt()) == pytest.approx(CR.norm64(g, segs), rel=1e-14)
    assert b.guards_intact() and int(b.cnt.item()) == 0
    _launch(name, gd, 1.0, bufs=b)                            # the second, identical launch
    assert torch.equal(_bits(b.out), first[0]) and torch.equal(_bits(b.slab), first[1])
    assert b.guards_intact() and int(b.cnt.item()) == 0
    assert torch.equal(_bits(gd), _bits(g))                   # the gradient is only read


def test_found_inf_and_non_finite_gradients():
    n, segs = _layout("sizes")
    g = _float_gradient("sizes")
    for inv in (None, INV):
        inv1 = 1.0 if inv is None else inv
        b = _launch("sizes", g.to(DEV), 0.01, inv, found=1.0)
        assert _same32(b.out[1].item(), inv1)
        assert abs(int(np.float32(b.out[0].item()).view(np.int32))
                   - int(CR.norm32(g, segs, inv1).view(np.int32))) <= 1
        b = _launch("sizes", g.to(DEV), 0.01, inv, found=0.0)
        assert _same32(b.out[1].item(), np.float32(inv1) * CR.coef32(b.out[0].item(), 0.01))
        assert 0 < b.out[1].item() < inv1
    off, size = segs[6]
    bad = g.clone()
    bad[off + size - 1] = float("inf")
    b = _launch("sizes", bad.to(DEV), 1.0, INV)
    assert b.out[0].item() == math.inf and b.out[1].item() == 0.0
    bad[off + size - 1] = float("nan")
    b = _launch("sizes", bad.to(DEV), 1.0)
    assert math.isnan(b.out[0].item()) and math.isnan(b.out[1].item())


def test_refusals_launch_nothing():
    K = _k()
    S = K.SEG_CHUNK
    n, segs = _layout("sizes")
    g = _float_gradient("sizes").to(DEV)
    good = _tables("sizes")
    h = [{"lr": 0.0}]
    long_row = (K.BlkRow * 1)()
    long_row[0].first, long_row[0].seg, long_row[0].count = 0, 0, S + 4
    empty_row = (K.BlkRow * 1)()
    bad_tables = {"offset": K.seg_tables([(6, 8)], h, DEV)[0],
                  "past n": K.seg_tables([(n - 8, 12)], h, DEV)[0],
                  "overlap": K.seg_tables([(0, 16), (8, 16)], h * 2, DEV)[0],
                  "count above the chunk": K.SegTables(good.seg_host, long_row, DEV),
                  "count zero": K.SegTables(good.seg_host, empty_row, DEV),
                  "no rows": K.seg_tables([], [], DEV)[0]}
    b = _Bufs(good.nblocks)
    for name, t in bad_tables.items():
        with pytest.raises(ValueError, match="grad_clip"):
            K.grad_clip(g, t, 1.0, b.slab, b.cnt, b.out)
        torch.cuda.synchronize()
        assert b.untouched(), name
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_norm"):
            K.grad_clip(g, good, bad, b.slab, b.cnt, b.out)
    with pytest.raises(ValueError, match="grad_clip"):       # a host gradient
        K.grad_clip(g.cpu(), good, 1.0, b.slab, b.cnt, b.out)
    with pytest.raises(ValueError, match="grad_clip"):       # a host output
        K.grad_clip(g, good, 1.0, b.slab, b.cnt, torch.zeros(2))
    with pytest.raises(ValueError, match="grad_clip"):       # a slab shorter than the block table
        K.grad_clip(g, good, 1.0, b.slab[:-1], b.cnt, b.out)
    with pytest.raises(ValueError, match="grad_clip"):       # an f64 gradient
        K.grad_clip(g.double(), good, 1.0, b.slab, b.cnt, b.out)
    torch.cuda.synchronize()
    assert b.untouched()
    K.grad_clip(g, good, 1.0, b.slab, b.cnt, b.out)          # (the good arguments do launch)
    torch.cuda.synchronize()
    assert not b.untouched() and b.guards_intact()


# ------------------------------------------------------------------ the update fed by the kernel
GROUPS = [dict(lr=0.1, momentum=0.9, weight_decay=1e-4),
          dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True),
          dict(lr=0.1, momentum=0.9, weight_decay=1e-4, lars=0.02)]
SHADOWS = {"none": None, "bf16": torch.bfloat16}


def _two_steps(kind, sdt, inv, scale_from_kernel, max_norm):
    """Two updates on the same gradient (the first over an uninitialised momentum buffer): p, buf
    and shadow after each, with the SGD's inv_scale either out[1:2] of grad_clip or a host-made
    tensor of the reference coefficient. The gradient is the integer one, whose norm the kernel
    gets exactly, so the two coefficients are the same bits by construction; the weights are
    generic floats."""
    K = _k()
    n, segs = _layout("sizes")
    g = _integer_gradient("sizes")[0]
    p = torch.where(g.isnan(), g, torch.randn(n, generator=H._gen(23)))
    if kind == "flat":          # sgd_flat runs over one contiguous range, of a ragged length
        n = segs[-1][1]
        p, g, segs = torch.randn(n, generator=H._gen(24)), _square_ints(n, 25)[0], [(0, n)]
        hyper = [GROUPS[0]]
    else:
        hyper = [GROUPS[i % 3] for i in range(len(segs))]
    tables, _ = K.seg_tables(segs, hyper, DEV)
    pd, gd = p.to(DEV), g.to(DEV)
    buf = torch.full((n,), float("nan"), device=DEV)
    sh = torch.zeros(n, dtype=sdt, device=DEV) if sdt is not None else None
    inv_d = torch.tensor([inv], dtype=torch.float32, device=DEV) if inv is not None else None
    b = _Bufs(tables.nblocks)
    snaps = []
    for it in range(2):
        if scale_from_kernel:
            K.grad_clip(gd, tables, max_norm, b.slab, b.cnt, b.out, inv_scale=inv_d)
            scale = b.out[1:2]
        else:
            scale = torch.tensor([CR.scale32(g, segs, max_norm, 1.0 if inv is None else inv)],
                                 dtype=torch.float32).to(DEV)
        if kind == "flat":
            h = hyper[0]
            K.sgd_flat(pd, gd, buf, sh, h["lr"], h["momentum"], h["weight_decay"], it > 0,
                       inv_scale=scale)
        else:
            K.seg_norms(pd, gd, tables)
            K.sgd_seg(pd, gd, buf, sh, tables, initialized=it > 0, inv_scale=scale)
        torch.cuda.synchronize()
        snaps.append(tuple(None if t is None else t.cpu() for t in (pd, buf, sh)))
    return snaps, (p, g, segs, hyper)


@pytest.mark.parametrize("shadow,inv", [("none", None), ("bf16", INV)], ids=["f32-noinv", "bf16-inv"])
@pytest.mark.parametrize("kind", ["flat", "seg"])
def test_update_fed_by_the_kernel(kind, shadow, inv):
    """sgd_flat, and sgd_seg over plain, Nesterov and LARS groups, fed out[1:2]: bit-equal to the
    launch fed the reference coefficient, and within the optimizer's bound of the float64 reference."""
    sdt, max_norm = SHADOWS[shadow], 0.5
    inv1 = 1.0 if inv is None else inv
    got, (p, g, segs, hyper) = _two_steps(kind, sdt, inv, True, max_norm)
    host, _ = _two_steps(kind, sdt, inv, False, max_norm)
    scale = CR.scale32(g, segs, max_norm, inv1)
    assert 0 < float(scale) < inv1                                    # the clip is active
    ref = CR.clipped_sgd_ref(torch.nan_to_num(p), torch.nan_to_num(g), segs, hyper, 2, max_norm, inv1)
    for it in range(2):
        for a, b in zip(got[it], host[it]):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), f"step {it}"
        pk, bk, sk = got[it]
        for off, size in segs:
            sl = slice(off, off + size)
            torch.testing.assert_close(pk[sl].to(F64), ref[it][0][sl].to(F64), rtol=1e-6, atol=1e-6)
            torch.testing.assert_close(bk[sl].to(F64), ref[it][1][sl].to(F64), rtol=1e-6, atol=1e-6)
            if sk is not None:
                assert bool(H.cast_matches(sk[sl], pk[sl]).all())
    assert not torch.equal(got[1][0], got[0][0])
