"""The weight EMA without a GPU: configuration and refusals, ModelEMA against tests/ema_refs.py, and
the CPU trainer with MX_EMA (validation line, metrics, best.pt, suspend -> resume)."""
import json

import pytest
import torch
from torch import nn

import ema_refs as R
import head_refs as H
from pytorch_distributed_amd import trainer
from pytorch_distributed_amd.config import config_for, parse_cli
from pytorch_distributed_amd.ema import EMA_REFUSAL, ModelEMA, build_ema, ema_weight

F64 = torch.float64


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------ config
def test_config_parses_the_three_variables():
    c = config_for("single", env={})
    assert (c.ema, c.ema_every, c.ema_warmup) == (0.0, 1, True)
    c = config_for("ddp", env={"MX_EMA": "0.999", "MX_EMA_EVERY": "4", "MX_EMA_WARMUP": "0"})
    assert (c.ema, c.ema_every, c.ema_warmup) == (0.999, 4, False)
    c = config_for("single", env={}, argv=["--ema", "0.9", "--ema-every", "2", "--ema-warmup", "1"])
    assert (c.ema, c.ema_every, c.ema_warmup) == (0.9, 2, True)
    assert set(parse_cli(["--ema", "0.5"])) == {"MX_EMA"}
    assert config_for("single", env={"MX_EMA": "0"}).ema == 0.0
    for bad in ("1", "-0.1", "nan", "1.5", "inf"):
        with pytest.raises(ValueError, match="MX_EMA"):
            config_for("single", env={"MX_EMA": bad})
    for bad in ("0", "-2"):
        with pytest.raises(ValueError, match="MX_EMA_EVERY"):
            config_for("single", env={"MX_EMA": "0.9", "MX_EMA_EVERY": bad})


def test_schedule_matches_the_reference():
    for decay in (0.5, 0.9, 0.9999):
        for warmup in (True, False):
            for t in (0, 1, 5, 100, 100_000):
                assert ema_weight(decay, t, warmup) == R.weight(decay, t, warmup)


class _FakeNative(nn.Module):
    def state_dict(self, *a, **k):
        raise AssertionError("the refusal comes first")


def test_captured_steps_refuse_the_ema_before_training():
    """MX_GRAPH=1 on the native engine, DataParallel with replicas or with forced replay: ValueError
    that names the cause and MX_EMA, before the model is asked for anything."""
    cfg = config_for("single", env={"MX_GRAPH": "1", "MX_EMA": "0.9"})
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.bfloat16, engine="native")
    with pytest.raises(ValueError, match="MX_GRAPH=1 cannot run MX_EMA") as ei:
        build_ema(cfg, _FakeNative(), ctx)
    assert str(ei.value) == EMA_REFUSAL.format(what="MX_GRAPH=1")
    cfg = config_for("dp", env={"MX_EMA": "0.9"})
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.bfloat16, engine="native")
    dp = _FakeNative()
    dp.replicas = [object()]
    with pytest.raises(ValueError, match="DataParallel.*MX_EMA"):
        build_ema(cfg, dp, ctx)
    dp = _FakeNative()
    dp.force_replay, dp._native = True, True
    with pytest.raises(ValueError, match="PDA_DP_FORCE_REPLAY=1"):
        build_ema(cfg, dp, ctx)
    # off: nothing is built, nothing refused; on the torch engine MX_GRAPH does not capture
    off = config_for("single", env={"MX_GRAPH": "1"})
    assert build_ema(off, _FakeNative(), ctx) is None
    cfg = config_for("single", env={"MX_GRAPH": "1", "MX_EMA": "0.9", "MX_EMA_EVERY": "3"})
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")
    e = build_ema(cfg, nn.Linear(2, 2), ctx)
    assert type(e) is ModelEMA and (e.decay, e.every, e.warmup) == (0.9, 3, True)


def test_constructor_refuses_bad_arguments():
    m = nn.Linear(2, 2)
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            ModelEMA(m, bad)
    with pytest.raises(ValueError):
        ModelEMA(m, 0.9, every=0)


def test_binding_refuses_host_tensors_and_dtypes():
    """ema_update's Python checks need no GPU: an f16 e, lengths that differ, host buffers."""
    from pytorch_distributed_amd.ops import native_ops as K
    e, p = torch.zeros(8), torch.ones(8)
    with pytest.raises(ValueError, match="f32"):
        K.ema_update([(e.half(), p)], K.EMA_LERP, 0.5)
    with pytest.raises(ValueError, match="8 elements"):
        K.ema_update([(e, p[:4])], K.EMA_LERP, 0.5)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        K.ema_update([(e, p, torch.zeros(8))], K.EMA_SWAP)
    with pytest.raises(ValueError, match="GPU"):
        K.ema_update([(e, p)], K.EMA_LERP, 0.5)
    assert torch.equal(e, torch.zeros(8)) and torch.equal(p, torch.ones(8))
    assert K.ema_weight(0.1) == float(torch.tensor(0.1, dtype=torch.float32))


# ------------------------------------------------------------------ ModelEMA
def _resnet():
    from pytorch_distributed_amd.models import build_model
    torch.manual_seed(0)
    return build_model("resnet18", 10)


def _train_steps(model, ema, n):
    g = H._gen(31)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    snaps = []
    model.train()
    for _ in range(n):
        x, y = torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 10, (4,), generator=g)
        opt.zero_grad()
        nn.functional.cross_entropy(model(x), y).backward()
        opt.step()
        ema.update()
        snaps.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    return snaps


@pytest.mark.parametrize("every,warmup", [(1, True), (2, False)])
def test_model_ema_matches_the_reference(every, warmup):
    """ResNet-18 on the CPU, four SGD steps: every floating tensor within the accumulated
    3 * 2^-24 (|p| + |e|) bound of the float64 recurrence, integer buffers copied at each update."""
    model = _resnet()
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ema = ModelEMA(model, 0.9, every=every, warmup=warmup)
    snaps = _train_steps(model, ema, 4)
    assert ema.steps == 4 and ema.num_updates == 4 // every
    sd = ema.state_dict()
    assert list(sd["model"]) == list(start) and sd["num_updates"] == 4 // every
    moved = 0
    for k, e in sd["model"].items():
        if not e.is_floating_point():
            assert k.endswith("num_batches_tracked") and e.dtype == torch.int64
            assert int(e) == int(snaps[(4 // every) * every - 1][k]) == (4 // every) * every
            continue
        want, bound, n, _ = R.run(start[k], [s[k] for s in snaps], 0.9, every, warmup)
        assert n == ema.num_updates
        err = (e.to(F64) - want).abs()
        assert bool((err <= bound).all()), f"{k}: {float(err.max())} over {float(bound.max())}"
        moved += int(not torch.equal(e, start[k]))
    assert moved > 60      # (the average did follow the weights)


def test_model_ema_swapped_restores_every_bit_and_round_trips():
    model = _resnet()
    ema = ModelEMA(model, 0.9)
    _train_steps(model, ema, 2)
    live = {k: v.detach().clone() for k, v in model.state_dict().items()}
    avg = {k: v.clone() for k, v in ema.state_dict()["model"].items()}
    assert any(not torch.equal(live[k], avg[k]) for k in live)
    with ema.swapped():
        for k, v in model.state_dict().items():
            assert torch.equal(_bits(v), _bits(avg[k])), k
        for k, v in ema.ema.items():
            assert torch.equal(_bits(v), _bits(live[k])), k
    for k, v in model.state_dict().items():
        assert torch.equal(_bits(v), _bits(live[k])), k
    for k, v in ema.ema.items():
        assert torch.equal(_bits(v), _bits(avg[k])), k
    # the state loads strictly into the torchvision-keyed model and into another ModelEMA
    sd = ema.state_dict()
    _resnet().load_state_dict(sd["model"], strict=True)
    other = ModelEMA(_resnet(), 0.5, every=3, warmup=False)
    other.load_state_dict(sd)
    assert (other.decay, other.every, other.warmup, other.num_updates, other.steps) == (0.9, 1, True, 2, 2)
    for k, v in other.ema.items():
        assert torch.equal(_bits(v), _bits(avg[k])), k
    bad = dict(sd, model={k: v for k, v in sd["model"].items() if k != "fc.bias"})
    with pytest.raises(KeyError, match="fc.bias"):
        other.load_state_dict(bad)


# ------------------------------------------------------------------ the trainer on the CPU
def _cfg(tmp, **env):
    return config_for("single", env={
        "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "4", "MX_VAL_STEPS": "1",
        "MX_BATCH": "4", "MX_IMAGE_SIZE": "32", "MX_NUM_CLASSES": "10", "MX_DEVICE": "cpu",
        "MX_WORKERS": "0", "MX_METRICS": "1", "MX_SAVE_PATH": str(tmp), **env})


def _capture_ema(monkeypatch):
    from pytorch_distributed_amd import ema as ema_mod
    built, real = [], ema_mod.build_ema
    monkeypatch.setattr(ema_mod, "build_ema", lambda *a: built.append(real(*a)) or built[-1])
    return built


def test_cpu_run_validates_and_saves_the_average(tmp_path, capsys, monkeypatch):
    built = _capture_ema(monkeypatch)
    trainer.run(_cfg(tmp_path, MX_EMA="0.5"), "single")
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "Epoch: 0, Loss: " in l]
    assert len(lines) == 2 and lines[0].startswith("Epoch: 0") and lines[1].startswith("EMA Epoch: 0")
    rec = json.loads((tmp_path / "metrics.jsonl").read_text().strip().splitlines()[-1])
    assert 0.0 <= rec["ema_acc1"] <= 1.0 and "acc1" in rec
    ema = built[0]
    assert type(ema) is ModelEMA and ema.steps == 4 and ema.num_updates == 4
    best = tmp_path / "best.pt"
    if rec["ema_acc1"] > 0:            # best.pt is written when the accuracy beats 0: the average
        sd = torch.load(best, weights_only=True)
        _resnet().load_state_dict(sd, strict=True)
        for k, v in ema.state_dict()["model"].items():
            assert torch.equal(_bits(sd[k]), _bits(v)), k
    else:
        assert not best.exists()


def test_suspended_and_resumed_run_ends_with_the_same_average(tmp_path, capsys, monkeypatch):
    """MX_EMA=0.5 with MX_EMA_EVERY=1: a run suspended after step 2 and resumed from latest.pt ends
    with the EMA state of the uninterrupted run, bit for bit (counters included)."""
    from pytorch_distributed_amd.utils.suspend import REQUEUE_EXIT_CODE
    built = _capture_ema(monkeypatch)
    trainer.run(_cfg(tmp_path / "whole", MX_EMA="0.5"), "single")
    monkeypatch.setenv("MX_SUSPEND_AT_STEP", "2")
    with pytest.raises(SystemExit) as ei:
        trainer.run(_cfg(tmp_path / "cut", MX_EMA="0.5"), "single")
    assert ei.value.code == REQUEUE_EXIT_CODE
    ck = torch.load(tmp_path / "cut" / "latest.pt", weights_only=True)
    assert ck["step"] == 2 and ck["ema"]["steps"] == 2 and ck["ema"]["num_updates"] == 2
    assert set(ck["ema"]) == {"decay", "every", "warmup", "num_updates", "steps", "model"}
    assert list(ck["ema"]["model"]) == list(ck["model"])
    monkeypatch.delenv("MX_SUSPEND_AT_STEP")
    trainer.run(_cfg(tmp_path / "cut", MX_EMA="0.5"), "single")
    assert "resume: epoch 0 step 2" in capsys.readouterr().out
    whole, cut, resumed = (b.state_dict() for b in built)
    assert (cut["steps"], resumed["steps"], whole["steps"]) == (2, 4, 4)
    assert resumed["num_updates"] == whole["num_updates"] == 4
    for k, v in whole["model"].items():
        assert torch.equal(_bits(resumed["model"][k]), _bits(v)), k
    assert any(not torch.equal(cut["model"][k], v) for k, v in whole["model"].items())


def test_checkpoint_without_the_key_starts_the_average_from_the_loaded_weights(tmp_path, monkeypatch):
    built = _capture_ema(monkeypatch)
    monkeypatch.setenv("MX_SUSPEND_AT_STEP", "2")
    with pytest.raises(SystemExit):
        trainer.run(_cfg(tmp_path), "single")          # no MX_EMA: today's checkpoint
    ck = torch.load(tmp_path / "latest.pt", weights_only=True)
    assert "ema" not in ck and not built
    monkeypatch.setenv("MX_SUSPEND_AT_STEP", "1")      # stop again right after the next step
    with pytest.raises(SystemExit):
        trainer.run(_cfg(tmp_path, MX_EMA="0.5", MX_EMA_EVERY="2"), "single")
    ema = built[0]
    assert ema.steps == 1 and ema.num_updates == 0     # (every = 2: no update yet)
    for k, v in ema.state_dict()["model"].items():
        assert torch.equal(_bits(v), _bits(ck["model"][k])), k


def test_without_the_variable_nothing_changes(tmp_path, capsys, monkeypatch):
    """MX_EMA unset: latest.pt has exactly the keys it had, no EMA line is printed, the metrics
    record has no ema_acc1 and save_latest writes "ema" only when given."""
    from pytorch_distributed_amd.utils.checkpoint import save_latest
    built = _capture_ema(monkeypatch)
    monkeypatch.setenv("MX_SUSPEND_AT_STEP", "2")
    with pytest.raises(SystemExit):
        trainer.run(_cfg(tmp_path / "a"), "single")
    ck = torch.load(tmp_path / "a" / "latest.pt", weights_only=True)
    assert set(ck) == {"model", "optimizer", "scheduler", "acc", "epoch", "step"}
    monkeypatch.delenv("MX_SUSPEND_AT_STEP")
    trainer.run(_cfg(tmp_path / "a"), "single")
    out = capsys.readouterr().out
    assert "EMA" not in out and out.count("Epoch: 0, Loss: ") == 1 and not built
    rec = json.loads((tmp_path / "a" / "metrics.jsonl").read_text().strip().splitlines()[-1])
    assert set(rec) - {"ts"} == {"epoch", "steps", "epoch_s", "acc1", "images", "gpu_mem_gb", "gpu_util_pct",
                                 "gpu_util_method", "engine", "dtype"}
    p = save_latest(tmp_path / "b", {}, {}, {}, 0.0, 0, 0)
    assert set(torch.load(p, weights_only=True)) == set(ck)
    p = save_latest(tmp_path / "b", {}, {}, {}, 0.0, 0, 0, ema_sd={"steps": 3})
    assert torch.load(p, weights_only=True)["ema"] == {"steps": 3}
