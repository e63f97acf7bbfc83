"""Colour jitter on the device (csrc/jitter.hip) against the float64 reference of tests/jitter_refs.py:
the apply (and its mean pass) on hand-made tables, the draw against its host mirror bit for bit, the
trainer's order beside the erase, and MX_GRAPH=1 against the eager run."""
import ctypes

import numpy as np
import pytest
import torch

import jitter_refs as R
from pytorch_distributed_amd import jitter as J

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 8 x the largest deviation of jitter_ref evaluated in numpy float32 from jitter_ref in float64 over
# the f32 cases and tables below (4.367e-6, profiles/jitter.md): room for another legitimate association
# of the same float32 operations (* (1 / std) for / std, the mean summed in double), nothing more
TOL32 = 8 * 4.367e-6

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


def _bound(want, dtype):
    """|out - ref| allowed: tol32, plus half a 16-bit ulp of the reference for one rounding"""
    if dtype == F32:
        return np.full_like(want, TOL32)
    e = np.frexp(want)[1] - 1                                   # |want| in [2^e, 2^(e+1))
    return np.ldexp(0.5, (e - 7) if dtype == BF16 else np.maximum(e, -14) - 10) + TOL32


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("layout,dtype,B,S", CASES, ids=IDS)
def test_batch_jitter_against_the_reference(layout, dtype, B, S, cap):
    """Every table kind of jitter_refs.ROWS, rotated over the samples: each op alone, all four with
    contrast first and last, fb = 0, fh = +-0.5, all skipped. grid_cap 2 makes both stride loops
    iterate and samples share blocks."""
    K = _k()
    x0 = R.levels_input(layout, dtype, B, S)
    x64 = x0.double().numpy()
    slab = torch.empty(B * K.jitter_bps(B, S, dtype, layout, cap), dtype=torch.float64, device=DEV)
    assert S < 64 or slab.numel() // B > 1 or cap                # several partials per sample
    for k in range(len(R.ROWS)):
        factors, orders = R.hand_table(k, B)
        table = torch.tensor(J.jitter_table(factors, orders), device=DEV)
        outs = []
        for _ in range(2):
            x = x0.to(DEV)
            K.batch_jitter(x, table, layout, slab, grid_cap=cap)
            outs.append(x.cpu())
        got = outs[0]
        assert torch.equal(_bits(got), _bits(outs[1])), "two launches differ"
        want = R.jitter_ref(x64, factors, orders, layout)
        pix = (slice(None),) * 3 + (slice(0, 12),) if layout == R.S2D else ()
        err = np.abs(got.double().numpy() - want)[pix]
        print(f"kind {k}: max |out - ref| = {err.max():.3e}")
        assert (err <= _bound(want[pix], dtype)).all(), (k, float(err.max()))
        if layout == R.S2D:
            assert torch.equal(_bits(got[..., 12:]), _bits(x0[..., 12:])), "padding slots"
        for b in np.flatnonzero((orders < 0).all(1)):           # all skipped: bits kept off the clamp
            c = np.arange(12) % 3 if layout == R.S2D else np.arange(3)[:, None, None]
            x01 = x64[b][pix[1:]] * R.STD[c] + R.MEAN[c]
            keep = torch.tensor((x01 > 1e-6) & (x01 < 1 - 1e-6))  # (f32 and f64 agree the clamp is idle)
            assert keep.any() and torch.equal(_bits(got[b][pix[1:]])[keep], _bits(x0[b][pix[1:]])[keep])


@pytest.mark.parametrize("B", [1, 257])
@pytest.mark.parametrize("strengths", [(0.4, 0.3, 0.2, 0.1), (0.4, 0, 0.2, 0), (2.0, 0, 0, 0.5)])
def test_jitter_draw_equals_the_host_mirror(B, strengths):
    K = _k()
    for key in ((0, 0, 0, 0), (7, 3, 2, 11)):
        table = torch.full((B, 5), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        K.jitter_draw(table, J.batch_key(*key), strengths)
        assert np.array_equal(table.cpu().numpy(), J.draw_jitter(*key, B, strengths)), key


def test_refusals_launch_nothing():
    from pytorch_distributed_amd.ops import ext
    K, L, st = _k(), ext.lib(), torch.cuda.current_stream().cuda_stream
    table = torch.full((4, 5), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    x = torch.ones(4, 3, 8, 8, device=DEV)
    slab = torch.zeros(4 * K.jitter_bps(4, 8, F32, R.NCHW), dtype=torch.float64, device=DEV)
    t, nan, inf = table.data_ptr(), float("nan"), float("inf")
    for b, c, s, h, p in ((-0.1, 0, 0, 0, t), (0, nan, 0, 0, t), (0, 0, inf, 0, t), (0, 0, 0, 0.6, t),
                          (0, 0, 0, -0.1, t), (0.4, 0.4, 0.4, 0.1, None), (0.4, 0.4, 0.4, 0.1, t + 2)):
        assert L.pda_jitter_draw(4, 1, b, c, s, h, p, st) == -2
    for bad in ((-0.1, 0, 0, 0), (0, 0, 0, 0.6), (0, nan, 0, 0), (0.4, 0.4, 0.4)):
        with pytest.raises(ValueError, match="jitter_draw"):
            K.jitter_draw(table, 1, bad)
    ms = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
    good = dict(x=x.data_ptr(), t=t, slab=slab.data_ptr(), n=slab.numel(), B=4, S=8, dt=0, layout=1)
    for kw in (dict(x=x.data_ptr() + 4), dict(t=None), dict(t=t + 2), dict(slab=None), dict(n=3),
               dict(slab=slab.data_ptr() + 4), dict(dt=1), dict(B=0)):
        a = {**good, **kw}
        assert L.pda_jitter_mean(a["x"], a["t"], a["slab"], a["n"], a["B"], a["S"], a["dt"], a["layout"], *ms, 0, st) == -2, kw
        assert L.pda_batch_jitter(a["x"], a["t"], a["slab"], a["n"], 1, a["B"], a["S"], a["dt"], a["layout"], *ms, 0, st) == -2, kw
    for args in ((x.bfloat16(), table, R.NCHW, slab), (x, table[:3], R.NCHW, slab), (x, table, R.NCHW, slab[:3]),
                 (x, table, R.NCHW, slab.float()), (x, table.long(), R.NCHW, None)):
        with pytest.raises(ValueError, match="batch_jitter"):
            K.batch_jitter(*args)
    torch.cuda.synchronize()
    assert bool((table == 0x5A5A5A5A).all()) and bool((x == 1).all()) and bool((slab == 0).all())


class _Ctx:
    rank, engine = 1, "native"


def test_jitter_then_erase_as_the_trainer_orders_them():
    """BatchJitter, then BatchEraser, on a tiny bf16 s2d batch with all three variables on (the mixer
    takes what they leave): the reference jitter of the drawn table, its erase boxes zeroed."""
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.erase import BatchEraser, draw_erase, erase_torch
    B, S = 3, 6
    cfg = config_for("single", env={"MX_IMAGE_SIZE": str(S), "MX_COLOR_JITTER": "0.4,0.4,0.4,0.1",
                                    "MX_RANDOM_ERASE": "1", "MX_CUTMIX": "1", "MX_SEED": "5"})
    x0 = R.levels_input(R.S2D, BF16, B, S)
    jit = J.BatchJitter(cfg, _Ctx())
    x = BatchEraser(cfg, _Ctx())(jit(x0.to(DEV), 2, 7), 2, 7).cpu()
    table = J.draw_jitter(5, 1, 2, 7, B, cfg.color_jitter)
    assert np.array_equal(jit.table.cpu().numpy(), table)
    want = torch.tensor(R.jitter_ref(x0.double().numpy(), *J.table_parts(table), R.S2D))
    boxes = draw_erase(5, 1, 2, 7, B, S, 1.0)
    erase_torch(want, boxes, R.S2D)
    assert (boxes[:, 1] > boxes[:, 0]).any() and bool((x[..., :12] == 0).any())
    err = (x.double() - want).abs().numpy()[..., :12]
    assert (err <= _bound(want.numpy()[..., :12], BF16)).all(), float(err.max())


def test_graph_mode_trains_on_the_jittered_batch(tmp_path, capsys, monkeypatch):
    """MX_GRAPH=1 needs no refusal: the captured step copies the batch it is handed, after the jitter
    and on the same stream, so two replayed steps end with the eager run's weights. The jitter ran
    once per training step on the engine's s2d bf16 batch, with a slab (contrast is on)."""
    from pytorch_distributed_amd import trainer
    from pytorch_distributed_amd.config import config_for
    K = _k()
    models, calls, real_build, real_jitter = [], [], trainer.build_model, K.batch_jitter
    monkeypatch.setattr(trainer, "build_model", lambda *a: models.append(real_build(*a)) or models[-1])
    monkeypatch.setattr(K, "batch_jitter", lambda x, t, l, slab: calls.append((tuple(x.shape), x.dtype, slab is None))
                        or real_jitter(x, t, l, slab))
    for sub, env in (("eager", {}), ("graph", {"MX_GRAPH": "1"})):
        trainer.run(config_for("single", env={
            "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
            "MX_BATCH": "8", "MX_IMAGE_SIZE": "64", "MX_DTYPE": "bf16", "MX_LOG_EVERY": "0", "MX_WORKERS": "0",
            "MX_COLOR_JITTER": "0.4", "MX_SAVE_PATH": str(tmp_path / sub), **env}), "single")
    capsys.readouterr()
    torch.cuda.synchronize()
    assert calls == [((8, 32, 32, 16), BF16, False)] * 4
    eager, graph = models
    assert torch.equal(_bits(eager.flat_params), _bits(graph.flat_params))
    assert torch.equal(_bits(eager.flat_buffers), _bits(graph.flat_buffers))
