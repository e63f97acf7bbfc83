"""Random erasing without a GPU: configuration, BatchEraser on the CPU against tests/erase_refs.py,
the host-side wrapper checks, and the trainer's wiring (off by default, before the mixer)."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import erase_refs as R
from pytorch_distributed_amd import trainer
from pytorch_distributed_amd.config import config_for, parse_cli


# ------------------------------------------------------------------ config
def test_config_parses_the_variable():
    assert config_for("single", env={}).random_erase == 0.0
    assert config_for("ddp", env={"MX_RANDOM_ERASE": "0.25"}).random_erase == 0.25
    assert config_for("single", env={"MX_RANDOM_ERASE": "1"}).random_erase == 1.0
    assert config_for("single", env={}, argv=["--random-erase", "0.5"]).random_erase == 0.5
    assert set(parse_cli(["--random-erase", "1"])) == {"MX_RANDOM_ERASE"}
    for bad in ("-0.1", "1.5", "nan", "inf"):
        with pytest.raises(ValueError, match="MX_RANDOM_ERASE"):
            config_for("single", env={"MX_RANDOM_ERASE": bad})
    assert not config_for("single", env={"MX_RANDOM_ERASE": "1"}).soft_targets     # hard labels stay


# ------------------------------------------------------------------ BatchEraser on the CPU
class _Ctx:
    rank, engine = 0, "torch"


def _eraser(S, p, seed=0, rank=0):
    from pytorch_distributed_amd.erase import BatchEraser
    cfg = config_for("single", env={"MX_IMAGE_SIZE": str(S), "MX_RANDOM_ERASE": str(p), "MX_SEED": str(seed)})
    ctx = _Ctx()
    ctx.rank = rank
    return BatchEraser(cfg, ctx)


@pytest.mark.parametrize("layout,dtype", [(R.NCHW, torch.float32), (R.S2D, torch.float32),
                                          (R.S2D, torch.bfloat16), (R.S2D, torch.float16)])
def test_batch_eraser_cpu_erases_in_place(layout, dtype):
    S, B = 10, 8
    x0 = R.planted_input(layout, dtype, S, B)
    eraser = _eraser(S, 0.5, seed=5, rank=1)
    hit = 0
    for step in range(4):
        x = x0.clone()
        out = eraser(x, 2, step)
        assert out is x                                         # in place, the same tensor
        boxes, accepted, _ = R.draw(5, 1, 2, step, B, S, 0.5)
        assert torch.equal(R.bits(x), R.bits(R.erased(x0, boxes, layout)))
        hit += sum(a >= 0 for a in accepted)
    assert 0 < hit < 4 * B                                      # p = 0.5: some samples, not all
    with pytest.raises(ValueError, match="neither"):
        eraser(torch.zeros(2, 5, 7), 0, 0)
    other = torch.zeros(2, 3, 12, 12) if layout == R.NCHW else torch.zeros(2, 6, 6, 16, dtype=dtype)
    with pytest.raises(ValueError, match="12x12"):
        eraser(other, 0, 0)


def test_wrappers_validate_on_the_host():
    """erase_bounds / batch_erase_check are pure Python: the refusals need no GPU and name the
    argument."""
    from pytorch_distributed_amd.ops import native_ops as K
    assert K.erase_bounds(0.25, R.SCALE, R.RATIO) == (0.25, 0.02, 0.33, math.log(0.3), math.log(3.3))
    for kw, word in ((dict(p=-0.1), "p"), (dict(p=1.5), "p"), (dict(p=float("nan")), "p"),
                     (dict(scale=(0.5, 0.2)), "scale"), (dict(scale=(-0.1, 0.2)), "scale"),
                     (dict(scale=(0.1, float("inf"))), "scale"), (dict(ratio=(3.0, 0.3)), "ratio"),
                     (dict(ratio=(0.0, 1.0)), "ratio"), (dict(ratio=(0.3, float("nan"))), "ratio")):
        a = dict(p=0.5, scale=R.SCALE, ratio=R.RATIO)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            K.erase_bounds(a["p"], a["scale"], a["ratio"])
    s = torch.zeros(2, 4, 4, 16, dtype=torch.bfloat16)
    n = torch.zeros(2, 3, 6, 6)
    t = torch.zeros(2, 4, dtype=torch.int32)
    assert K.batch_erase_check(s, t, K.AUG_S2D) == (2, 8)
    assert K.batch_erase_check(n, t, K.AUG_NCHW) == (2, 6)
    bad = [
        (n, t, K.AUG_S2D),                                   # not s2d
        (s, t, K.AUG_NCHW),
        (n.bfloat16(), t, K.AUG_NCHW),                       # NCHW is f32
        (s.double(), t, K.AUG_S2D),
        (n, t, 2),
        (n, t.long(), K.AUG_NCHW),                           # the table is int32
        (n, torch.zeros(3, 4, dtype=torch.int32), K.AUG_NCHW),
        (n, torch.zeros(2, 3, dtype=torch.int32), K.AUG_NCHW),
        (n.permute(0, 1, 3, 2)[:, :, ::2], t, K.AUG_NCHW),
        (n[:, :, :, ::2].transpose(2, 3)[:, :, :, :3], t, K.AUG_NCHW),
    ]
    for args in bad:
        with pytest.raises(ValueError, match="batch_erase"):
            K.batch_erase_check(*args)
    with pytest.raises(ValueError, match="GPU"):
        K.batch_erase(n, t, K.AUG_NCHW)
    with pytest.raises(ValueError, match="GPU"):
        K.erase_draw(t, 6, 0, 0.5)
    with pytest.raises(ValueError, match="int32"):
        K.erase_draw(t.long(), 6, 0, 0.5)


# ------------------------------------------------------------------ the trainer on the CPU
def _ctx(**env):
    cfg = config_for("single", env={"MX_IMAGE_SIZE": "8", "MX_LOG_EVERY": "0", **env})
    return trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")


def test_off_by_default_owns_nothing():
    ctx = _ctx()
    assert trainer._batch_eraser(ctx) is None and ctx.extra == {}
    ctx = _ctx(MX_RANDOM_ERASE="0")
    assert trainer._batch_eraser(ctx) is None and ctx.extra == {}
    ctx = _ctx(MX_RANDOM_ERASE="0.25")
    e = trainer._batch_eraser(ctx)
    assert e is not None and e.p == 0.25 and trainer._batch_eraser(ctx) is e and set(ctx.extra) == {"eraser"}


class _Loader:
    def __init__(self, n):
        g = torch.Generator().manual_seed(6)
        self.batches = [(torch.randn(4, 3, 8, 8, generator=g) + 5.0, torch.randint(0, 5, (4,), generator=g))
                        for _ in range(n)]
        self.given = [x.clone() for x, _ in self.batches]

    def iter_from(self, k):
        return iter(list(enumerate(self.batches))[k:])


class _Crit(nn.Module):
    def forward(self, out, labels, *soft):
        return nn.functional.cross_entropy(out, labels)


def _train(tmp_path, monkeypatch, **env):
    """Three steps of trainer.train on the CPU with a recording stub in the mixer's place."""
    ctx = _ctx(**env)
    seen = []

    class Mixer:
        def __call__(self, samples, labels, epoch, step):
            seen.append((step, samples.clone()))
            return samples, labels, labels.roll(1, 0), 1.0
    if ctx.cfg.mixup > 0 or ctx.cfg.cutmix > 0:
        ctx.extra["mixer"] = Mixer()
    fed = []
    torch.manual_seed(0)
    model = nn.Sequential(nn.Flatten(), nn.Linear(192, 5))
    model.register_forward_pre_hook(lambda m, args: fed.append(args[0].clone()))
    loader = _Loader(3)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    assert trainer.train(loader, model, _Crit(), opt, None, 0, ctx, 0, 0.0, tmp_path) == 3
    return loader, seen, fed


def test_the_mixer_receives_a_batch_that_already_has_its_zeros(tmp_path, monkeypatch):
    """p = 1 with CutMix on: the stub mixer is handed the erased batch (torchvision's order:
    per-sample transforms, then the mixing), and so is the model."""
    loader, seen, fed = _train(tmp_path, monkeypatch, MX_RANDOM_ERASE="1", MX_CUTMIX="1")
    assert [s for s, _ in seen] == [0, 1, 2]
    for step, got in seen:
        boxes, accepted, _ = R.draw(0, 0, 0, step, 4, 8, 1.0)
        assert all(a >= 0 for a in accepted) and int((boxes[:, 1] > boxes[:, 0]).sum()) > 0
        want = R.erased(loader.given[step], boxes, R.NCHW)
        assert torch.equal(R.bits(got), R.bits(want))
        assert int((got == 0).sum()) > 0 and int((loader.given[step] == 0).sum()) == 0
        assert torch.equal(R.bits(fed[step]), R.bits(want))


def test_without_the_variable_the_batch_is_untouched(tmp_path, monkeypatch):
    loader, seen, fed = _train(tmp_path, monkeypatch)
    assert seen == []
    for step in range(3):
        assert torch.equal(R.bits(fed[step]), R.bits(loader.given[step]))
    loader, _, fed = _train(tmp_path, monkeypatch, MX_RANDOM_ERASE="1")      # hard labels: no mixer
    for step in range(3):
        boxes = R.draw(0, 0, 0, step, 4, 8, 1.0)[0]
        assert torch.equal(R.bits(fed[step]), R.bits(R.erased(loader.given[step], boxes, R.NCHW)))


def test_cpu_entrypoint_runs_with_random_erase_beside_cutmix(tmp_path, capsys, monkeypatch):
    """The single-GPU script's path on the CPU for three steps with MX_RANDOM_ERASE=1 and
    MX_CUTMIX=1: the eraser ran once per training step (and not in validation), the loss is finite."""
    from pytorch_distributed_amd import erase
    cfg = config_for("single", env={
        "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "3", "MX_VAL_STEPS": "1",
        "MX_BATCH": "4", "MX_IMAGE_SIZE": "32", "MX_NUM_CLASSES": "10", "MX_DEVICE": "cpu",
        "MX_WORKERS": "0", "MX_SAVE_PATH": str(tmp_path / "out"), "MX_RANDOM_ERASE": "1", "MX_CUTMIX": "1"})
    draws, real = [], erase.draw_erase
    monkeypatch.setattr(erase, "draw_erase", lambda *a: draws.append(a) or real(*a))
    trainer.run(cfg, "single")
    out = capsys.readouterr().out
    loss = float(out.split("Epoch: 0, Loss: ")[1].split(",")[0])
    assert math.isfinite(loss) and loss > 0
    assert [d[:7] for d in draws] == [(0, 0, 0, s, 4, 32, 1.0) for s in range(3)]
    assert all(np.asarray(real(*d)).any() for d in draws)
