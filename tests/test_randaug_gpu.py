"""RandAugment on the device (csrc/randaug.hip) against the float64 reference of tests/randaug_refs.py:
the statistics and the apply on hand-made one-slot tables, the draw against its host mirror bit for
bit, the chain beside the jitter and the erase, the refusals, and MX_GRAPH=1 against the eager run."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import randaug_refs as R
from pytorch_distributed_amd import randaug as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 8 x the largest deviation of chain_ref evaluated in numpy float32 from chain_ref in float64 over the
# f32 cases and rows below (1.102e-6, a Color row at (2, 64); profiles/randaug.md): room for another
# legitimate association of the same float32 operations, nothing more
TOL32 = 8 * 1.102e-6

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SHAPES = [(1, 2), (3, 6), (2, 64)]
CASES = ([(R.S2D, dt, B, S) for dt in (F32, BF16, F16) for B, S in SHAPES]
         + [(R.NCHW, F32, B, S) for B, S in SHAPES + [(2, 5)]])
IDS = [f"{'s2d' if l == R.S2D else 'nchw'}-{str(dt).split('.')[1]}-B{B}-S{S}" for l, dt, B, S in CASES]


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bound(want, dtype, tol=TOL32):
    """|out - ref| allowed: tol, plus half a 16-bit ulp of the reference for one rounding"""
    if dtype == F32:
        return np.full_like(want, tol)
    e = np.frexp(want)[1] - 1                                   # |want| in [2^e, 2^(e+1))
    return np.ldexp(0.5, (e - 7) if dtype == BF16 else np.maximum(e, -14) - 10) + tol


@functools.lru_cache(maxsize=None)
def _reference(layout, dtype, B, S, k):
    """(input, reference, skipped elements) of table kind k: computed once, shared by both grid caps"""
    x0 = R.randaug_input(layout, dtype, B, S)
    want, skip, eq_tie = R.chain_ref(R.images(x0, layout), *R.hand_rows(k, B, S), dtype)
    assert not eq_tie, "an Equalize input lies on a tie of floor(255 x + 0.5)"
    assert skip.mean() <= 0.02, float(skip.mean())
    return x0, want, skip


def _check(got, want, skip, geo, dtype, what):
    """geometric samples exactly, the rest within the bound, outside the skipped elements"""
    err = np.abs(got - want)
    print(f"{what}: max |out - ref| = {err[~skip].max():.3e}, skipped {skip.mean():.4f}")
    assert (err[geo][~skip[geo]] == 0).all(), what
    assert (err[~skip] <= _bound(want, dtype)[~skip]).all(), (what, float(err[~skip].max()))


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("layout,dtype,B,S", CASES, ids=IDS)
def test_stats_and_apply_against_the_reference(layout, dtype, B, S, cap):
    """Every row of randaug_refs.ROWS, rotated over the samples. grid_cap 2 makes the stride loops
    iterate and samples share blocks."""
    K = _k()
    stats = torch.empty(B * K.randaug_stat_row(), dtype=torch.int32, device=DEV)
    slab = torch.empty(B * K.randaug_bps(B, S, dtype, layout, cap), dtype=torch.float64, device=DEV)
    assert S < 64 or slab.numel() // B > 1 or cap                # several partials per sample
    for k in range(len(R.ROWS)):
        x0, want, skip = _reference(layout, dtype, B, S, k)
        ops, par, co = R.hand_rows(k, B, S)
        table = torch.tensor(A.pack_table(ops, par, co), device=DEV)
        src, outs = x0.to(DEV), []
        for _ in range(2):
            dst = torch.full_like(src, -3.0)
            stats.zero_()
            K.randaug_stats(src, table, 0, stats, slab, layout, grid_cap=cap)
            K.randaug_apply(src, dst, table, 0, stats, slab, layout, grid_cap=cap)
            outs.append(dst.cpu())
        got = outs[0]
        assert torch.equal(_bits(got), _bits(outs[1])), "two launches differ"
        assert torch.equal(_bits(src.cpu()), _bits(x0)), "the source was written"
        _check(R.images(got, layout), want, skip, np.isin(ops[:, 0], R.GEO), dtype, f"kind {k}")
        if layout == R.S2D:
            assert torch.equal(_bits(got[..., 12:]), _bits(x0[..., 12:])), "padding slots"
        for b in np.flatnonzero(ops[:, 0] == 0):                 # Identity: bits kept off the clamp
            x01 = R.images(x0, layout)[b] * R.STD + R.MEAN
            keep = (x01 > 1e-6) & (x01 < 1 - 1e-6)                # (f32 and f64 agree the clamp is idle)
            assert keep.any() and (R.images(got, layout)[b][keep] == R.images(x0, layout)[b][keep]).all()


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("n,m", [(1, 0), (2, 9), (4, 30)])
def test_randaug_draw_equals_the_host_mirror(B, n, m):
    K = _k()
    for key in ((0, 0, 0, 0), (7, 3, 2, 11)):
        table = torch.full((B, n, 8), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        stats = torch.full((n * B * K.randaug_stat_row(),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        K.randaug_draw(table, stats, 224, A.batch_key(*key), m)
        want = A.draw_randaug(*key, B, 224, n, m)
        assert np.array_equal(table.cpu().numpy(), want), key
        rows = stats.view(n, B, -1).cpu().numpy()                # zeroed exactly where a slot accumulates
        acc = np.isin(want[..., 0], (12, 13)).T
        assert not rows[acc].any() and (rows[~acc] == 0x5A5A5A5A).all()


class _Ctx:
    rank, engine = 1, "native"


@pytest.mark.parametrize("n,m", [(2, 9), (3, 30)])
def test_the_chain_then_jitter_and_erase_as_the_trainer_orders_them(n, m):
    """BatchRandAugment on a tiny bf16 s2d batch: the host mirror's table, the result in the loader's
    batch (n even) or the second buffer (n odd), the reference chain; then BatchJitter and BatchEraser
    take whichever tensor it returned."""
    from jitter_refs import jitter_ref
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.erase import BatchEraser, draw_erase, erase_torch
    from pytorch_distributed_amd.jitter import BatchJitter, draw_jitter, table_parts
    B, S = 3, 6
    cfg = config_for("single", env={"MX_IMAGE_SIZE": str(S), "MX_RAND_AUGMENT": f"{n},{m}", "MX_SEED": "5",
                                    "MX_COLOR_JITTER": "0.4,0.4,0.4,0.1", "MX_RANDOM_ERASE": "1"})
    x0 = R.randaug_input(R.S2D, BF16, B, S)
    aug, x = A.BatchRandAugment(cfg, _Ctx()), x0.to(DEV)
    y = aug(x, 2, 7)
    table = A.draw_randaug(5, 1, 2, 7, B, S, n, m)
    assert np.array_equal(aug.table.cpu().numpy(), table)
    assert y.data_ptr() == (aug.buf if n % 2 else x).data_ptr()
    ops, par, co = A.table_parts(table)
    want, skip, eq_tie = R.chain_ref(R.images(x0, R.S2D), ops, par, co, BF16)
    assert not eq_tie and skip.mean() <= 0.02
    _check(R.images(y.cpu(), R.S2D), want, skip, np.zeros(B, bool), BF16, f"chain {ops.tolist()}")
    assert torch.equal(_bits(y.cpu()[..., 12:]), _bits(x0[..., 12:])), "padding slots"
    mid = y.cpu()
    z = BatchEraser(cfg, _Ctx())(BatchJitter(cfg, _Ctx())(y, 2, 7), 2, 7).cpu()
    ref = torch.tensor(jitter_ref(mid.double().numpy(), *table_parts(draw_jitter(5, 1, 2, 7, B, cfg.color_jitter)), R.S2D))
    erase_torch(ref, draw_erase(5, 1, 2, 7, B, S, 1.0), R.S2D)
    err = (z.double() - ref).abs().numpy()[..., :12]
    assert (err <= _bound(ref.numpy()[..., :12], BF16, 8 * 4.367e-6)).all(), float(err.max())   # (the jitter's TOL32)


def test_refusals_launch_nothing():
    from pytorch_distributed_amd.ops import ext
    K, L, st = _k(), ext.lib(), torch.cuda.current_stream().cuda_stream
    B, S, row = 4, 8, K.randaug_stat_row()
    table = torch.full((B, 2, 8), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    stats = torch.full((2 * B * row,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    x, y = torch.ones(B, 3, S, S, device=DEV), torch.full((B, 3, S, S), 2.0, device=DEV)
    slab = torch.zeros(B * K.randaug_bps(B, S, F32, R.NCHW), dtype=torch.float64, device=DEV)
    t, s = table.data_ptr(), stats.data_ptr()
    for kw in (dict(B=0), dict(n=0), dict(n=5), dict(m=-1), dict(m=31), dict(S=0), dict(t=None), dict(t=t + 2),
               dict(s=None), dict(s=s + 4), dict(len=2 * B * row - 1)):
        a = {**dict(B=B, n=2, m=9, S=S, t=t, s=s, len=stats.numel()), **kw}
        assert L.pda_randaug_draw(a["B"], a["n"], a["m"], a["S"], 1, a["t"], a["s"], a["len"], st) == -2, kw
    ms = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
    good = dict(x=x.data_ptr(), y=y.data_ptr(), t=t, n=2, slot=1, s=s, len=stats.numel(), slab=slab.data_ptr(),
                sl=slab.numel(), B=B, S=S, dt=0, layout=1)
    for kw in (dict(x=x.data_ptr() + 4), dict(x=None), dict(t=None), dict(t=t + 2), dict(n=0), dict(n=5), dict(slot=2),
               dict(slot=-1), dict(s=None), dict(s=s + 4), dict(len=2 * B * row - 1), dict(slab=None), dict(sl=3),
               dict(slab=slab.data_ptr() + 4), dict(dt=1), dict(B=0), dict(S=0), dict(layout=2)):
        a = {**good, **kw}
        tail = (a["B"], a["S"], a["dt"], a["layout"], *ms, 0, st)
        assert L.pda_randaug_stats(a["x"], a["t"], a["n"], a["slot"], a["s"], a["len"], a["slab"], a["sl"], *tail) == -2, kw
        assert L.pda_randaug_apply(a["x"], a["y"], a["t"], a["n"], a["slot"], a["s"], a["len"], a["slab"], a["sl"], *tail) == -2, kw
    for kw in (dict(y=x.data_ptr()), dict(y=x.data_ptr() + 16), dict(y=None), dict(y=y.data_ptr() + 4)):   # aliased, bad dst
        a = {**good, **kw}
        assert L.pda_randaug_apply(a["x"], a["y"], t, 2, 1, s, stats.numel(), slab.data_ptr(), slab.numel(), B, S, 0, 1,
                                   *ms, 0, st) == -2, kw
    for bad in ((table, stats, S, 1, 31), (table, stats, 0, 1, 9), (table[:, :, :5], stats, S, 1, 9),
                (table, stats[:5], S, 1, 9), (table.long(), stats, S, 1, 9)):
        with pytest.raises(ValueError, match="randaug_draw"):
            K.randaug_draw(*bad)
    for bad in ((x, x, table, 0, stats, slab), (x, y, table, 2, stats, slab), (x, y, table[:3], 0, stats, slab),
                (x, y, table, 0, stats, slab[:3]), (x, y, table, 0, stats.float(), slab), (x, y.double(), table, 0, stats, slab),
                (x.bfloat16(), y.bfloat16(), table, 0, stats, slab)):
        with pytest.raises(ValueError, match="randaug_apply"):
            K.randaug_apply(*bad, R.NCHW)
    torch.cuda.synchronize()
    assert bool((table == 0x5A5A5A5A).all()) and bool((stats == 0x5A5A5A5A).all())
    assert bool((x == 1).all()) and bool((y == 2).all()) and bool((slab == 0).all())


def test_graph_mode_trains_on_the_augmented_batch(tmp_path, capsys, monkeypatch):
    """MX_GRAPH=1 needs no refusal: the captured step copies the batch it is handed, after the chain and
    on the same stream, so two replayed steps end with the eager run's weights. The apply ran n times
    per training step of either run (2 x n per step over the two) on the engine's s2d bf16 batch."""
    from pytorch_distributed_amd import trainer
    from pytorch_distributed_amd.config import config_for
    K = _k()
    models, calls, real_build, real_apply = [], [], trainer.build_model, K.randaug_apply
    monkeypatch.setattr(trainer, "build_model", lambda *a: models.append(real_build(*a)) or models[-1])
    monkeypatch.setattr(K, "randaug_apply", lambda src, *a: calls.append((tuple(src.shape), src.dtype))
                        or real_apply(src, *a))
    for sub, env in (("eager", {}), ("graph", {"MX_GRAPH": "1"})):
        trainer.run(config_for("single", env={
            "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
            "MX_BATCH": "8", "MX_IMAGE_SIZE": "64", "MX_DTYPE": "bf16", "MX_LOG_EVERY": "0", "MX_WORKERS": "0",
            "MX_RAND_AUGMENT": "3,9", "MX_SAVE_PATH": str(tmp_path / sub), **env}), "single")
    capsys.readouterr()
    torch.cuda.synchronize()
    assert calls == [((8, 32, 32, 16), BF16)] * (2 * 2 * 3)
    eager, graph = models
    assert torch.equal(_bits(eager.flat_params), _bits(graph.flat_params))
    assert torch.equal(_bits(eager.flat_buffers), _bits(graph.flat_buffers))
