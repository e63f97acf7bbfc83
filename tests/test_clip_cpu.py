"""MX_CLIP_GRAD_NORM without a GPU: parsing and refusals, the captured-step refusals, and the torch
engine's clipped step on the CPU against a hand-written clip-then-step."""
import json

import pytest
import torch
from torch import nn

from pytorch_distributed_amd import trainer
from pytorch_distributed_amd.config import config_for, parse_cli
from pytorch_distributed_amd.runtime.graphs import CLIP_REFUSAL


# ------------------------------------------------------------------ config
def test_config_parses_the_variable():
    assert config_for("single", env={}).clip_grad_norm == 0.0
    assert config_for("ddp", env={"MX_CLIP_GRAD_NORM": "2.5"}).clip_grad_norm == 2.5
    assert config_for("single", env={"MX_CLIP_GRAD_NORM": "0"}).clip_grad_norm == 0.0
    assert config_for("single", env={}, argv=["--clip-grad-norm", "1"]).clip_grad_norm == 1.0
    assert set(parse_cli(["--clip-grad-norm", "0.5"])) == {"MX_CLIP_GRAD_NORM"}
    for bad in ("-1", "-0.001", "nan", "inf", "-inf"):
        with pytest.raises(ValueError, match="MX_CLIP_GRAD_NORM"):
            config_for("single", env={"MX_CLIP_GRAD_NORM": bad})


# ------------------------------------------------------------------ refusals before training
class _FakeDP(nn.Module):
    """Looks like a DataParallel wrapper; asked for an optimizer or a parameter, it fails the test."""

    def make_optimizer(self, **kw):
        raise AssertionError("the refusal comes first")

    def parameters(self, recurse=True):
        raise AssertionError("the refusal comes first")


def test_replicated_steps_refuse_clipping_before_training():
    cfg = config_for("dp", env={"MX_CLIP_GRAD_NORM": "1.0"})
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.bfloat16, engine="native")
    dp = _FakeDP()
    dp.replicas = [object()]
    with pytest.raises(ValueError, match="DataParallel.*MX_CLIP_GRAD_NORM") as ei:
        trainer.build_optimizer(cfg, dp, ctx)
    assert str(ei.value) == CLIP_REFUSAL.format(
        what="DataParallel over several devices (or with PDA_DP_FORCE_REPLAY=1)")
    dp = _FakeDP()
    dp.replicas, dp.force_replay, dp._native = [], True, True
    with pytest.raises(ValueError, match="PDA_DP_FORCE_REPLAY=1"):
        trainer.build_optimizer(cfg, dp, ctx)


def test_dataparallel_factory_refuses_and_one_device_passes_the_value_on():
    from pytorch_distributed_amd.parallel.dp import DataParallel
    dp = DataParallel(nn.Linear(3, 2), device_ids=[])
    dp.replicas = [nn.Linear(3, 2)]
    with pytest.raises(ValueError, match="MX_CLIP_GRAD_NORM"):
        dp.make_optimizer(lr=0.1, clip_grad_norm=1.0)
    dp.replicas = []
    opt = dp.make_optimizer(lr=0.1, momentum=0.9, weight_decay=0.0, clip_grad_norm=1.0)
    assert type(opt) is torch.optim.SGD        # a torch optimizer: the trainer clips before step()


def test_native_optimizer_refuses_bad_values_before_touching_the_model():
    from pytorch_distributed_amd.models.native_train import NativeSGD
    for bad in (-1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            NativeSGD(None, clip_grad_norm=bad)


# ------------------------------------------------------------------ the trainer on the CPU
def _cfg(tmp, **env):
    return config_for("single", env={
        "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
        "MX_BATCH": "4", "MX_IMAGE_SIZE": "32", "MX_NUM_CLASSES": "10", "MX_DEVICE": "cpu",
        "MX_WORKERS": "0", "MX_METRICS": "1", "MX_SAVE_PATH": str(tmp), **env})


def _capture_optimizer(monkeypatch):
    built, real = [], trainer.build_optimizer
    monkeypatch.setattr(trainer, "build_optimizer", lambda *a: built.append(real(*a)) or built[-1])
    return built


def _by_hand(cfg, max_norm):
    """Two steps of the eager branch, the clip written out: per-tensor 2-norms, the norm of those,
    coef = clamp(max_norm / (total + 1e-6), max=1), every gradient times coef, SGD step."""
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")
    model = trainer.build_model(cfg, ctx)
    loader, _, _ = trainer._make_loaders(cfg, ctx, model, cfg.batch_size)
    opt = torch.optim.SGD(model.parameters(), lr=cfg.lr, momentum=cfg.momentum,
                          weight_decay=cfg.weight_decay)
    crit, total = nn.CrossEntropyLoss(), None
    model.train()
    for _, (x, y) in loader.iter_from(0):
        out = model(x)
        opt.zero_grad()
        crit(out, y).backward()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        norms = torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads])
        total = torch.linalg.vector_norm(norms, 2.0)
        if max_norm is not None:
            coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
            for g in grads:
                g.mul_(coef)
        opt.step()
    return [p.detach().clone() for p in model.parameters()], float(total)


def test_cpu_run_clips_as_written_by_hand_and_logs_the_norm(tmp_path, monkeypatch):
    built = _capture_optimizer(monkeypatch)
    cfg = _cfg(tmp_path, MX_CLIP_GRAD_NORM="0.5")
    trainer.run(cfg, "single")
    got = [p.detach() for g in built[0].param_groups for p in g["params"]]
    want, last_norm = _by_hand(cfg, 0.5)
    assert last_norm > 0.5                      # the clip was active
    assert len(got) == len(want) == 62
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    unclipped, _ = _by_hand(cfg, None)
    assert any(not torch.equal(a, b) for a, b in zip(got, unclipped))
    rec = json.loads((tmp_path / "metrics.jsonl").read_text().strip().splitlines()[-1])
    assert rec["grad_norm"] == last_norm and rec["steps"] == 2


def test_without_the_variable_the_metrics_have_no_such_key(tmp_path, monkeypatch):
    built = _capture_optimizer(monkeypatch)
    cfg = _cfg(tmp_path)
    trainer.run(cfg, "single")
    rec = json.loads((tmp_path / "metrics.jsonl").read_text().strip().splitlines()[-1])
    assert "grad_norm" not in rec and "acc1" in rec
    got = [p.detach() for g in built[0].param_groups for p in g["params"]]
    want, _ = _by_hand(cfg, None)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
