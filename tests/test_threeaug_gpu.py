"""3-Augment on the device (csrc/threeaug.hip) against the float64 reference of tests/threeaug_refs.py:
the apply on hand-made tables, its refusals, the draw against its host mirror, the trainer's order
beside the jitter and the erase, and MX_GRAPH=1 against the eager run."""
import numpy as np
import pytest
import torch

import threeaug_refs as R
from pytorch_distributed_amd import threeaug as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 8 x the largest deviation of three_aug_ref evaluated in numpy float32 from three_aug_ref in float64
# over the f32 cases and tables below (1.034e-6, profiles/threeaug.md): room for another legitimate
# association of the same float32 operations (fmaf for * and +, * (1 / std) for / std), nothing more
TOL32 = 8 * 1.034e-6

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CASES = ([(R.S2D, dt, *s) for dt in (F32, BF16, F16) for s in R.SHAPES]
         + [(R.NCHW, F32, *s) for s in R.SHAPES + R.NCHW_ONLY])
IDS = [f"{'s2d' if l == R.S2D else 'nchw'}-{str(dt).split('.')[1]}-B{B}-S{S}" for l, dt, B, S, _ in CASES]


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
@pytest.mark.parametrize("layout,dtype,B,S,r", CASES, ids=IDS)
def test_three_aug_against_the_reference(layout, dtype, B, S, r, cap):
    """Every table kind of threeaug_refs: the three ops rotated over the samples, the blur rows with
    the weights of sigma 0.1 and 2.0. grid_cap 2 makes the tile and sample loops iterate."""
    K = _k()
    x0 = R.levels_input(layout, dtype, B, S)
    x64, src = x0.double().numpy(), x0.to(DEV)
    pix = (slice(None),) * 3 + (slice(0, 12),) if layout == R.S2D else ()
    for k in range(R.KINDS):
        table = R.hand_table(k, B, r)
        outs = []
        for _ in range(2):
            dst = torch.full_like(src, -3.0)
            K.three_aug(src, dst, torch.tensor(table, device=DEV), layout, grid_cap=cap)
            outs.append(dst.cpu())
        got = outs[0]
        assert torch.equal(_bits(got), _bits(outs[1])), "two launches differ"
        want = R.three_aug_ref(x64, table, layout)
        err = np.abs(got.double().numpy() - want)[pix]
        print(f"kind {k}: max |out - ref| = {err.max():.3e}")
        assert (err <= _bound(want[pix], dtype)).all(), (k, float(err.max()))
        if layout == R.S2D:
            assert torch.equal(_bits(got[..., 12:]), _bits(x0[..., 12:])), "padding slots"
    assert torch.equal(_bits(src.cpu()), _bits(x0)), "src was written"


def test_refusals_launch_nothing():
    K = _k()
    x = R.levels_input(R.S2D, BF16, 2, 12).to(DEV)
    dst = torch.full_like(x, -3.0)
    good = R.hand_table(2, 2, 11)
    bad_r, big_r, bad_op = good.copy(), good.copy(), good.copy()
    bad_r[1, 2], big_r[0, 2], bad_op[1, 0] = 0, 12, 3
    dev = lambda t: torch.tensor(t, device=DEV)
    tiny = torch.zeros(2, 1, 1, 16, dtype=BF16, device=DEV)                 # 2 x 2 images under R = 2
    calls = [(x, x, dev(good)), (x, x[:1], dev(good)), (x, dst, dev(bad_r)), (x, dst, dev(big_r)),
             (x, dst, dev(bad_op)), (x, dst, dev(good)[:1]), (x, dst, dev(good).long()),
             (tiny, torch.zeros_like(tiny), dev(R.hand_table(2, 2, 2)))]
    for args in calls:
        with pytest.raises(ValueError, match="three_aug"):
            K.three_aug(*args, R.S2D)
    with pytest.raises(ValueError, match="three_aug"):                      # an odd side has no s2d batch
        K.three_aug(torch.zeros(2, 3, 13, 13, device=DEV), torch.zeros(2, 3, 13, 13, device=DEV), dev(good), R.S2D)
    table = torch.full((2, 16), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    for r in (0, 12, -1, 1.5):
        with pytest.raises(ValueError, match="three_aug_draw"):
            K.three_aug_draw(table, 1, r)
    from pytorch_distributed_amd.ops import ext
    L, st = ext.lib(), torch.cuda.current_stream().cuda_stream
    import ctypes
    ms = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)
    t = dev(good)
    for s, d, tp, S in ((x.data_ptr(), x.data_ptr() + 64, t.data_ptr(), 12), (x.data_ptr(), dst.data_ptr(), None, 12),
                        (x.data_ptr(), dst.data_ptr(), t.data_ptr() + 2, 12), (x.data_ptr(), dst.data_ptr(), t.data_ptr(), 13)):
        assert L.pda_three_aug(s, d, tp, 2, S, 1, 0, *ms, 0, st) == -2
    for R_, tp in ((0, table.data_ptr()), (12, table.data_ptr()), (11, None), (11, table.data_ptr() + 2)):
        assert L.pda_three_aug_draw(2, R_, 1, tp, st) == -2
    torch.cuda.synchronize()
    assert bool((dst == -3).all()) and bool((table == 0x5A5A5A5A).all())


@pytest.mark.parametrize("B,r", [(1, 1), (300, 11), (300, 4)])
def test_draw_against_the_host_mirror(B, r):
    K = _k()
    tables = []
    for key in ((0, 0, 0, 0), (7, 3, 2, 11), (8, 3, 2, 11), (7, 4, 2, 11), (7, 3, 3, 11), (7, 3, 2, 12)):
        table = torch.full((B, 16), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        K.three_aug_draw(table, T.batch_key(*key), r)
        got, want = table.cpu().numpy(), T.draw_three_aug(*key, B, r)
        assert np.array_equal(got[:, :4], want[:, :4]), key            # op, sigma bits, R, 0
        assert np.abs(got[:, 4:].astype(np.int64) - want[:, 4:]).max() <= 1, key   # positive floats: 1 ulp
        assert (got[:, 5 + r:] == 0).all()
        tables.append(got)
    assert B < 300 or set(tables[1][:, 0]) == {0, 1, 2}
    assert all(not np.array_equal(tables[1], t) for t in tables[2:])


class _Ctx:
    rank, engine = 1, "native"


def test_three_augment_then_jitter_then_erase():
    """The three Batch* objects in the trainer's order against the six launches made by hand on the
    same keys, bit for bit, and the 3-Augment stage against the reference of its drawn table."""
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.erase import BatchEraser, batch_key as erase_key
    from pytorch_distributed_amd.jitter import BatchJitter, batch_key as jitter_key
    K, (B, S) = _k(), (6, 36)
    cfg = config_for("single", env={"MX_IMAGE_SIZE": str(S), "MX_THREE_AUGMENT": "1", "MX_COLOR_JITTER": "0.4",
                                    "MX_RANDOM_ERASE": "1", "MX_SEED": "5"})
    x0 = R.levels_input(R.S2D, BF16, B, S)
    three = T.BatchThreeAugment(cfg, _Ctx())
    y = three(x0.to(DEV), 2, 7)
    table = T.draw_three_aug(5, 1, 2, 7, B)
    assert np.array_equal(three.table.cpu().numpy()[:, :3], table[:, :3]) and len(set(table[:, 0])) == 3
    want = R.three_aug_ref(x0.double().numpy(), three.table.cpu().numpy(), R.S2D)[..., :12]
    err = np.abs(y.cpu().double().numpy()[..., :12] - want)
    assert (err <= _bound(want, BF16)).all(), float(err.max())
    got = BatchEraser(cfg, _Ctx())(BatchJitter(cfg, _Ctx())(y, 2, 7), 2, 7)
    src, hand = x0.to(DEV), torch.empty_like(y)
    t3, tj = torch.empty(B, 16, dtype=torch.int32, device=DEV), torch.empty(B, 5, dtype=torch.int32, device=DEV)
    boxes = torch.empty(B, 4, dtype=torch.int32, device=DEV)
    slab = torch.empty(B * K.jitter_bps(B, S, BF16, R.S2D), dtype=torch.float64, device=DEV)
    K.three_aug_draw(t3, T.batch_key(5, 1, 2, 7))
    K.three_aug(src, hand, t3, R.S2D)
    K.jitter_draw(tj, jitter_key(5, 1, 2, 7), cfg.color_jitter)
    K.batch_jitter(hand, tj, R.S2D, slab)
    K.erase_draw(boxes, S, erase_key(5, 1, 2, 7), 1.0)
    K.batch_erase(hand, boxes, R.S2D)
    assert torch.equal(_bits(got), _bits(hand)) and bool((got[..., :12] == 0).any())


def test_graph_mode_trains_on_the_augmented_batch(tmp_path, capsys, monkeypatch):
    """MX_GRAPH=1 needs no refusal: two replayed steps end with the eager run's weights. Per training
    step the trainer calls three_aug, then batch_jitter, then batch_erase."""
    from pytorch_distributed_amd import trainer
    from pytorch_distributed_amd.config import config_for
    K = _k()
    models, calls, real_build = [], [], trainer.build_model
    monkeypatch.setattr(trainer, "build_model", lambda *a: models.append(real_build(*a)) or models[-1])
    for name in ("three_aug", "batch_jitter", "batch_erase"):
        real = getattr(K, name)
        monkeypatch.setattr(K, name, lambda *a, _r=real, _n=name, **kw: calls.append(_n) or _r(*a, **kw))
    for sub, env in (("eager", {}), ("graph", {"MX_GRAPH": "1"})):
        trainer.run(config_for("single", env={
            "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
            "MX_BATCH": "8", "MX_IMAGE_SIZE": "64", "MX_DTYPE": "bf16", "MX_LOG_EVERY": "0", "MX_WORKERS": "0",
            "MX_THREE_AUGMENT": "1", "MX_COLOR_JITTER": "0.4", "MX_RANDOM_ERASE": "0.5",
            "MX_SAVE_PATH": str(tmp_path / sub), **env}), "single")
    capsys.readouterr()
    torch.cuda.synchronize()
    assert calls == ["three_aug", "batch_jitter", "batch_erase"] * 4
    eager, graph = models
    assert torch.equal(_bits(eager.flat_params), _bits(graph.flat_params))
    assert torch.equal(_bits(eager.flat_buffers), _bits(graph.flat_buffers))
