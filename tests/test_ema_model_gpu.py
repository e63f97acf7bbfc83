"""NativeEMA at the model level (native ResNet-18, 32 px, batch 8): the average against the float64
recurrence of tests/ema_refs.py fed per-step snapshots, the exchange for validation, the state dict,
AMP overflow steps, and one entrypoint run with MX_EMA.

Bound: 3 * 2^-24 * (|p| + |e_old|) per applied update (tests/ema_refs.py), accumulated over the
updates. Everything else is compared bit for bit.
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import ema_refs as R
import head_refs as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
STEPS = 5


def _native(dtype=torch.bfloat16, image=32):
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.models.native import NativeResNet
    torch.manual_seed(0)
    return NativeResNet(build_model("resnet18"), device=DEV, dtype=dtype, image_size=image)


def _batch(nm, image=32, B=8):
    from pytorch_distributed_amd.data import SyntheticImageNet
    return nm.input_generator(SyntheticImageNet("train", image_size=image))(torch.arange(B))


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _model_state(nm, opt=None):
    ts = [nm.flat_params, nm.flat_bufstore, nm.flat_shadow, nm.stem_packed]
    return [_bits(t) for t in ts + ([opt.flat_mom] if opt is not None else [])]


def _train(ema_args=None, steps=STEPS):
    """`steps` training steps as the trainer's eager branch runs them, with an EMA update after each
    optimizer step. Returns (model, optimizer, ema, start (params, buffers), per-step snapshots)."""
    from pytorch_distributed_amd.ema import NativeEMA
    nm = _native()
    opt, crit = nm.make_optimizer(lr=0.05, momentum=0.9, weight_decay=1e-4), nm.make_criterion()
    x, y = _batch(nm)
    ema = NativeEMA(nm, *ema_args) if ema_args is not None else None
    start = (nm.flat_params.cpu(), nm.flat_buffers.cpu(), nm.flat_nbt.cpu())
    snaps = []
    nm.train()
    for _ in range(steps):
        out = nm(x)
        opt.zero_grad()
        crit(out, y).backward()
        opt.step()
        if ema is not None:
            allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
            torch.cuda.set_sync_debug_mode("error")
            try:
                ema.update()        # no host synchronisation ...
            finally:
                torch.cuda.set_sync_debug_mode(0)
            assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocs   # ... no allocation
        torch.cuda.synchronize()
        snaps.append((nm.flat_params.cpu(), nm.flat_buffers.cpu(), nm.flat_nbt.cpu()))
    return nm, opt, ema, start, snaps


@functools.lru_cache(maxsize=None)
def _baseline():
    nm, opt, _, _, snaps = _train(None)
    return _model_state(nm, opt), snaps


@pytest.mark.parametrize("every,warmup", [(1, True), (1, False), (2, True), (2, False)])
def test_average_matches_the_reference_and_leaves_training_alone(every, warmup):
    nm, opt, ema, start, snaps = _train((0.9, every, warmup))
    assert ema.steps == STEPS and ema.num_updates == STEPS // every
    # construction copied the model: the reference starts from the same bits
    for i, (name, got) in enumerate((("params", ema.ema_params), ("buffers", ema.ema_buffers))):
        want, bound, n, last = R.run(start[i], [s[i] for s in snaps], 0.9, every, warmup)
        assert n == ema.num_updates
        err = (got.cpu().to(F64) - want).abs()
        worst = float((err - bound).max())
        assert worst <= 0, f"{name}: {worst} over the accumulated bound"
        assert not torch.equal(got.cpu(), start[i]), name
    assert torch.equal(ema.ema_nbt.cpu(), snaps[last][2]) and int(ema.ema_nbt[0]) == last + 1
    # the live training state is that of the same run without an EMA object, bit for bit
    base_state, base_snaps = _baseline()
    for a, b in zip(_model_state(nm, opt), base_state):
        assert torch.equal(a, b), "the EMA changed the training run"
    assert torch.equal(_bits(snaps[-1][1]), _bits(base_snaps[-1][1]))


def test_swapped_computes_with_the_average_and_restores_every_bit():
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.models.native import NativeResNet
    nm, opt, ema, _, _ = _train((0.9, 1, True), steps=3)
    x, _ = _batch(nm)
    sd = {k: v.clone() for k, v in ema.state_dict()["model"].items()}
    build_model("resnet18").load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    fresh = NativeResNet(build_model("resnet18"), device=DEV, dtype=torch.bfloat16, image_size=32)
    fresh.load_state_dict(sd, strict=True)
    fresh.eval()
    want = fresh(x).clone()
    nm.eval()
    live_logits = nm(x).clone()
    before_model, before_ema = _model_state(nm), [_bits(ema.ema_params), _bits(ema.ema_bufstore)]
    with ema.swapped():
        assert torch.equal(_bits(nm.flat_params), before_ema[0])
        assert torch.equal(_bits(nm.flat_bufstore), before_ema[1])
        assert torch.equal(_bits(ema.ema_params), before_model[0])
        assert bool(H.cast_matches(nm.flat_shadow, nm.flat_params).all())
        assert torch.equal(_bits(nm.stem_packed), _bits(fresh.stem_packed))
        for k, v in nm.state_dict().items():      # what the trainer saves as best.pt
            assert torch.equal(_bits(v), _bits(sd[k])), k
        got = nm(x).clone()
    assert torch.equal(_bits(got), _bits(want)), "swapped logits != a fresh model loaded from the EMA state"
    assert not torch.equal(got, live_logits)
    for a, b in zip(_model_state(nm), before_model):
        assert torch.equal(a, b), "the model is not back after swapped()"
    for a, b in zip([_bits(ema.ema_params), _bits(ema.ema_bufstore)], before_ema):
        assert torch.equal(a, b), "the EMA is not back after swapped()"
    assert torch.equal(_bits(nm(x)), _bits(live_logits))
    with pytest.raises(RuntimeError, match="boom"):   # an exception inside still exchanges back
        with ema.swapped():
            raise RuntimeError("boom")
    for a, b in zip(_model_state(nm), before_model):
        assert torch.equal(a, b)


def test_exact_fp32_engine_swaps_without_a_shadow():
    from pytorch_distributed_amd.ema import NativeEMA
    nm = _native(torch.float32)
    ema = NativeEMA(nm, 0.5)
    assert torch.equal(_bits(ema.ema_params), _bits(nm.flat_params))
    nm.flat_params.mul_(1.5)
    nm.refresh_shadow()
    ema.update()
    torch.cuda.synchronize()
    before = _model_state(nm)
    with ema.swapped():
        assert not torch.equal(_bits(nm.flat_params), before[0])
    for a, b in zip(_model_state(nm), before):
        assert torch.equal(a, b)


def test_state_dict_round_trip_is_bit_exact(tmp_path):
    from pytorch_distributed_amd.ema import ModelEMA, NativeEMA
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.utils.checkpoint import save_atomic
    nm, opt, ema, _, _ = _train((0.9, 2, False), steps=3)
    sd = ema.state_dict()
    assert {k: sd[k] for k in ("decay", "every", "warmup", "num_updates", "steps")} == {
        "decay": 0.9, "every": 2, "warmup": False, "num_updates": 1, "steps": 3}
    assert list(sd["model"]) == list(nm.state_dict())
    assert sd["model"]["conv1.weight"].shape == (64, 3, 7, 7)
    assert sd["model"]["bn1.num_batches_tracked"].dtype == torch.int64
    save_atomic({"ema": sd}, tmp_path / "ema.pt")
    loaded = torch.load(tmp_path / "ema.pt", weights_only=True)["ema"]
    other_model = _native()
    other_model.flat_params.add_(1.0)          # (another model: everything must come from the state)
    other_model.flat_buffers.add_(1.0)
    other = NativeEMA(other_model, 0.5)
    other.load_state_dict(loaded)
    assert (other.decay, other.every, other.warmup, other.num_updates, other.steps) == (0.9, 2, False, 1, 3)
    for k, v in other.state_dict()["model"].items():
        assert torch.equal(_bits(v), _bits(sd["model"][k])), k
    assert torch.equal(_bits(other.ema_bufstore), _bits(ema.ema_bufstore))
    tm = ModelEMA(build_model("resnet18"), 0.5)
    tm.load_state_dict(loaded)
    assert tm.num_updates == 1 and tm.every == 2
    for k, v in tm.state_dict()["model"].items():
        assert torch.equal(_bits(v), _bits(sd["model"][k])), k
    # and back: the torch EMA's state into the native one
    other.ema_params.zero_()
    other.load_state_dict(tm.state_dict())
    for k, v in other.state_dict()["model"].items():
        assert torch.equal(_bits(v), _bits(sd["model"][k])), k


def test_amp_overflow_step_still_updates_the_average():
    """fp16 with loss scaling: a step whose gradient overflowed leaves p unchanged, and the update
    after it still runs: num_updates advances and e moves towards the unchanged p."""
    from pytorch_distributed_amd.amp import LossScaler
    from pytorch_distributed_amd.ema import NativeEMA
    nm = _native(torch.float16)
    opt, crit = nm.make_optimizer(lr=0.05), nm.make_criterion()
    x, y = _batch(nm)
    scaler = LossScaler(init_scale=1024.0, growth_interval=1000)
    ema = NativeEMA(nm, 0.9, 1, False)

    def step(poison):
        scaler.scale(crit(nm(x), y)).backward()
        if poison:
            nm.flat_grad[nm.fc_b_off + 1] = float("inf")
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        ema.update()
        torch.cuda.synchronize()

    step(False)
    assert scaler.found_inf.item() == 0.0 and ema.num_updates == 1
    p1, e1 = nm.flat_params.cpu(), ema.ema_params.cpu()
    assert not torch.equal(p1, e1)
    step(True)
    assert scaler.found_inf.item() == 1.0 and scaler.get_scale() == 512.0
    assert torch.equal(_bits(nm.flat_params), _bits(p1)), "an overflowing step must leave p unchanged"
    assert ema.num_updates == 2 and ema.steps == 2
    e2 = ema.ema_params.cpu()
    err = (e2.to(F64) - R.lerp64(e1, p1, R.weight(0.9, 1, False))).abs()
    assert float((err - R.lerp_bound(e1, p1)).max()) <= 0
    assert not torch.equal(e2, e1)


def test_captured_dp_step_is_refused_and_one_device_runs(monkeypatch):
    from pytorch_distributed_amd import trainer
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.ema import NativeEMA, build_ema
    from pytorch_distributed_amd.parallel.dp import DataParallel
    nm = _native()
    cfg = config_for("dp", env={"MX_EMA": "0.9"})
    ctx = trainer.Context(cfg=cfg, device=DEV, dtype=torch.bfloat16, engine="native")
    monkeypatch.setenv("PDA_DP_FORCE_REPLAY", "1")
    with pytest.raises(ValueError, match="DataParallel.*MX_EMA"):
        build_ema(cfg, DataParallel(nm, device_ids=[0]), ctx)
    monkeypatch.setenv("PDA_DP_FORCE_REPLAY", "0")
    ema = build_ema(cfg, DataParallel(nm, device_ids=[0]), ctx)
    assert type(ema) is NativeEMA and ema.model is nm


def test_entrypoint_with_ema(tmp_path):
    """resnet_single_gpu.py with MX_EMA=0.9: the second validation line, ema_acc1 in the metrics, and
    a best.pt that loads into the torchvision-keyed model."""
    from pytorch_distributed_amd.models import build_model
    e = dict(os.environ)
    e.update({"MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "3", "MX_VAL_STEPS": "4",
              "MX_BATCH": "8", "MX_IMAGE_SIZE": "32", "MX_DTYPE": "bf16", "MX_METRICS": "1",
              "MX_NUM_CLASSES": "10", "MX_LR": "0.01", "PYTHONPATH": ROOT, "MX_EMA": "0.9"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "resnet_single_gpu.py")], cwd=tmp_path,
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if "Epoch: 0, Loss: " in l]
    assert len(lines) == 2 and lines[0].startswith("Epoch: 0") and lines[1].startswith("EMA Epoch: 0")
    out = tmp_path / "output" / "resnet_single"
    rec = json.loads((out / "metrics.jsonl").read_text().strip().splitlines()[-1])
    assert rec["engine"] == "native" and 0.0 < rec["ema_acc1"] <= 1.0
    sd = torch.load(out / "best.pt", weights_only=True)
    build_model("resnet18", 10).load_state_dict(sd, strict=True)
    assert f"New Best Acc: {100 * rec['ema_acc1']:.2f}%!" in r.stdout
