"""Random erasing on the device (csrc/erase.hip): the box draw and the in-place erase, bit for bit
against the float64 / index-arithmetic reference of tests/erase_refs.py (checked on the CPU in
tests/test_erase_refs_cpu.py), and BatchEraser on the device against itself on the CPU."""
import math

import numpy as np
import pytest
import torch

import erase_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64           # elements on each side of the batch (a multiple of 16 bytes in every dtype)
SENTINEL = 0x5A5A5A5A

CASES = ([(R.S2D, dt, S) for dt in (torch.float32, torch.bfloat16, torch.float16) for S in (4, 10, 32)]
         + [(R.NCHW, torch.float32, S) for S in (4, 6, 10, 32)])   # 4: rows of 16 bytes
IDS = [f"{'s2d' if l == R.S2D else 'nchw'}-{str(dt).split('.')[1]}-S{S}" for l, dt, S in CASES]


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ the draw
def _drawn(K, seed, rank, epoch, step, B, S, p, scale=R.SCALE, ratio=R.RATIO):
    from pytorch_distributed_amd.erase import batch_key
    table = torch.full((B, 4), SENTINEL, dtype=torch.int32, device=DEV)
    K.erase_draw(table, S, batch_key(seed, rank, epoch, step), p, scale, ratio)
    return table


def test_erase_draw_equals_the_reference_over_the_grid():
    """The CPU test's grid (seeds x ranks x epochs x steps x S, B = 64) at p in (0, 0.25, 1): the
    device table equals erase_refs.draw as integers. The grid holds no fragile sample (asserted in
    tests/test_erase_refs_cpu.py and again here), so exp's last bits cannot excuse a difference.
    All launches first, one read-back."""
    K = _k()
    jobs = [(g, p) for g in R.grid() for p in R.PROBS]
    tables = [_drawn(K, seed, rank, epoch, step, R.BATCH, S, p) for (seed, rank, epoch, step, S), p in jobs]
    got = torch.stack(tables).cpu().numpy()
    bad = []
    for k, ((seed, rank, epoch, step, S), p) in enumerate(jobs):
        boxes, _, frag = R.grid_draw(seed, rank, epoch, step, S, p)
        assert not any(frag)
        if not np.array_equal(got[k], boxes):
            bad.append((seed, rank, epoch, step, S, p))
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 65, 257])
def test_erase_draw_ragged_grids_and_the_boundary_bounds(B):
    """B = 1, 65 and 257 (one thread, a ragged block, a second block); the default bounds, the
    bounds that refuse all ten attempts (h = w = S, strict comparison) and those that give
    h = w = S - 1 at offsets {0, 1}."""
    K = _k()
    for S in (4, 10, 32, 224):
        for scale, ratio in ((R.SCALE, R.RATIO), R.REFUSED, R.almost(S)):
            boxes, accepted, frag = R.draw(3, 1, 2, 9, B, S, 1.0, scale, ratio)
            assert not any(frag)
            got = _drawn(K, 3, 1, 2, 9, B, S, 1.0, scale, ratio).cpu().numpy()
            assert np.array_equal(got, boxes), (B, S, scale, ratio)
            if (scale, ratio) == R.REFUSED:
                assert not got.any()
            elif scale != R.SCALE:
                assert set(accepted) == {0} and set((got[:, 1] - got[:, 0]).tolist()) == {S - 1}


def test_erase_draw_launcher_refusals_leave_the_table():
    from pytorch_distributed_amd.ops import ext
    K = _k()
    table = torch.full((9, 4), SENTINEL, dtype=torch.int32, device=DEV)
    t = table.data_ptr()
    l0, l1 = math.log(0.3), math.log(3.3)
    nan, inf = float("nan"), float("inf")
    good = dict(B=8, S=32, bkey=1, p=0.5, s0=0.02, s1=0.33, l0=l0, l1=l1, boxes=t)
    bad = [dict(B=0), dict(B=-1), dict(S=0), dict(S=-4), dict(p=-0.1), dict(p=1.5), dict(p=nan),
           dict(s0=0.5, s1=0.2), dict(l0=l1, l1=l0), dict(s1=inf), dict(s0=nan), dict(l0=-inf),
           dict(l1=nan), dict(s0=-0.1), dict(boxes=None), dict(boxes=t + 2)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        rc = ext.lib().pda_erase_draw(a["B"], a["S"], a["bkey"], a["p"], a["s0"], a["s1"], a["l0"], a["l1"],
                                      a["boxes"], _st())
        assert rc == -2, kw
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all())
    for args in ((table, 32, 1, 1.5), (table, 0, 1, 0.5), (table, 32, 1, 0.5, (0.5, 0.2)),
                 (table, 32, 1, 0.5, R.SCALE, (3.0, 0.3)), (table.long(), 32, 1, 0.5)):
        with pytest.raises(ValueError, match="erase_draw"):
            K.erase_draw(*args)
    torch.cuda.synchronize()
    assert bool((table == SENTINEL).all())
    rc = ext.lib().pda_erase_draw(*[good[k] for k in ("B", "S", "bkey", "p", "s0", "s1", "l0", "l1", "boxes")],
                                  _st())                     # (the good call does launch: 8 of 9 rows)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((table[:8] == SENTINEL).any()) and bool((table[8] == SENTINEL).all())


# ------------------------------------------------------------------ the erase
def _run(K, x_cpu, boxes, layout, grid_cap=0):
    """batch_erase on a batch that sits between two sentinel bands; returns the WHOLE buffer's bits
    and the expected ones (bands + erase_refs.erased)."""
    n = x_cpu.numel()
    big = torch.full((n + 2 * GUARD,), 7.0, dtype=x_cpu.dtype)
    want = big.clone()
    big[GUARD:GUARD + n] = x_cpu.reshape(-1)
    want[GUARD:GUARD + n] = R.erased(x_cpu, boxes, layout).reshape(-1)
    big = big.to(DEV)
    x = big[GUARD:GUARD + n].view(x_cpu.shape)
    assert x.data_ptr() % 16 == 0
    table = torch.tensor(np.asarray(boxes), dtype=torch.int32, device=DEV)
    if grid_cap:     # the launcher itself, validated like the wrapper's call, with a capped grid
        from pytorch_distributed_amd.ops import ext
        B, S = K.batch_erase_check(x, table, layout)
        rc = ext.lib().pda_batch_erase(x.data_ptr(), table.data_ptr(), B, S, ext.dt_of(x), layout, grid_cap,
                                       _st())
        assert rc == 0
    else:
        K.batch_erase(x, table, layout)
    torch.cuda.synchronize()
    return R.bits(big), R.bits(want)


@pytest.mark.parametrize("layout,dtype,S", CASES, ids=IDS)
def test_batch_erase_is_bit_exact_and_touches_nothing_else(layout, dtype, S):
    """B = 8, one hand-written box per sample: empty, the whole image, one pixel at odd (y, x) (it
    splits an s2d 2x2 group), flush with 0, flush with S, one row, one column, and one that reaches
    outside [0, S] on both sides (negative too), which the kernel clamps. The input has NaNs with
    payloads, -0 and +-max inside and outside the boxes and 3.0 in the s2d padding slots. The whole
    buffer, guard bands included, equals the reference as integers (+0.0 is not -0.0), with the
    natural grid and with grid_cap 1 and 2 (both grid-stride loops iterate)."""
    K = _k()
    x = R.planted_input(layout, dtype, S)
    kinds = R.box_kinds(S)
    boxes = list(kinds.values())
    for cap in (0, 1, 2):
        got, want = _run(K, x, boxes, layout, cap)
        assert torch.equal(got, want), cap
    n = x[0].numel()
    per = [slice(GUARD + b * n, GUARD + (b + 1) * n) for b in range(8)]
    xb = R.bits(x).reshape(8, -1)
    names = list(kinds)
    assert torch.equal(got[per[names.index("empty")]], xb[names.index("empty")])
    b = names.index("whole")
    img = got[per[b]].view(x[0].shape)
    if layout == R.S2D:
        assert int(torch.count_nonzero(img[..., :12])) == 0
        assert torch.equal(img[..., 12:], R.bits(x)[b][..., 12:]), "padding slots"
    else:
        assert int(torch.count_nonzero(img)) == 0
    b = names.index("odd pixel")
    assert int((got[per[b]] != xb[b]).sum()) <= 3                  # three elements


@pytest.mark.parametrize("layout,dtype,S", [(R.S2D, torch.bfloat16, 32), (R.NCHW, torch.float32, 10)],
                         ids=["s2d-bf16", "nchw-f32"])
def test_batch_erase_on_drawn_tables(layout, dtype, S):
    """The two launches as BatchEraser makes them: a table drawn on the device (p = 1), then the
    erase, against the reference draw and erase."""
    from pytorch_distributed_amd.erase import batch_key
    K = _k()
    x_cpu = R.planted_input(layout, dtype, S)
    boxes = R.draw(1, 0, 3, 4, 8, S, 1.0)[0]
    x = x_cpu.to(DEV)
    table = torch.empty(8, 4, dtype=torch.int32, device=DEV)
    K.erase_draw(table, S, batch_key(1, 0, 3, 4), 1.0)
    K.batch_erase(x, table, layout)
    torch.cuda.synchronize()
    assert np.array_equal(table.cpu().numpy(), boxes)
    assert torch.equal(R.bits(x), R.bits(R.erased(x_cpu, boxes, layout)))


def test_batch_erase_refusals():
    """Unaligned x or table, odd S in the s2d layout, a 16-bit NCHW batch: -2 from the launcher,
    ValueError from the wrapper, nothing written."""
    from pytorch_distributed_amd.ops import ext
    K = _k()
    L = ext.lib()
    s = torch.ones(2, 4, 4, 16, device=DEV, dtype=torch.bfloat16)
    n = torch.ones(2, 3, 8, 8, device=DEV)
    whole = torch.tensor([[0, 8, 0, 8]] * 2, dtype=torch.int32, device=DEV)
    t = whole.data_ptr()
    pool = torch.ones(n.numel() + 4, device=DEV)
    odd = pool[1:1 + n.numel()].view(n.shape)
    assert odd.data_ptr() % 16
    with pytest.raises(ValueError, match="aligned"):
        K.batch_erase(odd, whole, K.AUG_NCHW)
    calls = [
        (odd.data_ptr(), t, 2, 8, 0, K.AUG_NCHW, 0),          # x not 16-byte aligned
        (s.data_ptr() + 2, t, 2, 8, 1, K.AUG_S2D, 0),
        (n.data_ptr(), t + 2, 2, 8, 0, K.AUG_NCHW, 0),        # table not 4-byte aligned
        (s.data_ptr(), t, 2, 7, 1, K.AUG_S2D, 0),             # odd S in s2d
        (n.data_ptr(), t, 2, 8, 1, K.AUG_NCHW, 0),            # NCHW is f32
        (n.data_ptr(), t, 2, 8, 2, K.AUG_NCHW, 0),
        (s.data_ptr(), t, 2, 8, 3, K.AUG_S2D, 0),             # no such dtype
        (n.data_ptr(), t, 2, 8, 0, 2, 0),                     # no such layout
        (n.data_ptr(), t, 0, 8, 0, K.AUG_NCHW, 0),
        (n.data_ptr(), t, 2, 0, 0, K.AUG_NCHW, 0),
        (n.data_ptr(), t, 2, 8, 0, K.AUG_NCHW, -1),
        (None, t, 2, 8, 0, K.AUG_NCHW, 0),
        (n.data_ptr(), None, 2, 8, 0, K.AUG_NCHW, 0),
    ]
    for c in calls:
        assert L.pda_batch_erase(*c, _st()) == -2, c
    for args in ((n.bfloat16(), whole, K.AUG_NCHW), (n, whole, K.AUG_S2D), (n, whole.long(), K.AUG_NCHW),
                 (n, whole[:1], K.AUG_NCHW)):
        with pytest.raises(ValueError, match="batch_erase"):
            K.batch_erase(*args)
    torch.cuda.synchronize()
    assert bool((s == 1.0).all()) and bool((n == 1.0).all()) and bool((pool == 1.0).all())
    K.batch_erase(n, whole, K.AUG_NCHW)                        # (the good call does launch)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(n)) == 0


# ------------------------------------------------------------------ BatchEraser
class _Ctx:
    def __init__(self, engine):
        self.rank, self.engine = 1, engine


@pytest.mark.parametrize("layout,dtype", [(R.S2D, torch.bfloat16), (R.NCHW, torch.float32)],
                         ids=["s2d-bf16", "nchw-f32"])
def test_batch_eraser_device_equals_cpu(layout, dtype):
    """p = 0.5, two steps: the device branch (two launches into a persistent table) and the CPU
    branch (draw_erase + erase_torch) leave the same bits; the second call reuses the table and
    makes no host synchronisation."""
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.erase import BatchEraser
    S, B = 32, 8
    cfg = config_for("single", env={"MX_IMAGE_SIZE": str(S), "MX_RANDOM_ERASE": "0.5", "MX_SEED": "5"})
    dev_eraser, cpu_eraser = BatchEraser(cfg, _Ctx("native")), BatchEraser(cfg, _Ctx("torch"))
    x0 = R.planted_input(layout, dtype, S, B)
    ptrs, hit = [], 0
    for step in range(2):
        xd, xc = x0.to(DEV), x0.clone()
        torch.cuda.synchronize()
        if step:
            torch.cuda.set_sync_debug_mode("error")
        try:
            out = dev_eraser(xd, 1, step)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert out is xd and cpu_eraser(xc, 1, step) is xc
        torch.cuda.synchronize()
        assert torch.equal(R.bits(xd), R.bits(xc))
        boxes = R.draw(5, 1, 1, step, B, S, 0.5)[0]
        assert np.array_equal(dev_eraser.table.cpu().numpy(), boxes)
        hit += int((boxes[:, 1] > boxes[:, 0]).sum())
        ptrs.append(dev_eraser.table.data_ptr())
    assert ptrs[0] == ptrs[1] and cpu_eraser.table is None
    assert 0 < hit < 2 * B
    with pytest.raises(ValueError, match="neither"):
        dev_eraser(torch.zeros(2, 5, 7, device=DEV), 0, 0)
    with pytest.raises(ValueError, match="12x12"):
        dev_eraser(torch.zeros(2, 3, 12, 12, device=DEV), 0, 0)
