"""Random erasing through the single-GPU entrypoint's path (``trainer.run(cfg, "single")``, what
resnet_single_gpu.py calls) on the native engine: ResNet-18, batch 8, 64 px, bf16, three steps."""
import math

import pytest
import torch

import erase_refs as R
from pytorch_distributed_amd import trainer
from pytorch_distributed_amd.config import config_for

pytestmark = pytest.mark.gpu

MIX = {"MX_MIXUP": "0.2", "MX_CUTMIX": "1.0"}


def _cfg(tmp, **env):
    return config_for("single", env={
        "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "3", "MX_VAL_STEPS": "1",
        "MX_BATCH": "8", "MX_IMAGE_SIZE": "64", "MX_DTYPE": "bf16", "MX_LOG_EVERY": "0",
        "MX_WORKERS": "0", "MX_SAVE_PATH": str(tmp), **env})


def _capture(monkeypatch):
    """The models trainer.run builds, and the eraser's launches (seen through native_ops)."""
    from pytorch_distributed_amd.ops import native_ops as K
    models, erases, real_build, real_erase = [], [], trainer.build_model, K.batch_erase
    monkeypatch.setattr(trainer, "build_model", lambda *a: models.append(real_build(*a)) or models[-1])
    monkeypatch.setattr(K, "batch_erase", lambda x, t, l: erases.append((tuple(x.shape), x.dtype, l))
                        or real_erase(x, t, l))
    return models, erases


def _run(cfg, capsys):
    trainer.run(cfg, "single")
    out = capsys.readouterr().out
    loss = float(out.split("Epoch: 0, Loss: ")[1].split(",")[0])
    assert math.isfinite(loss) and loss > 0
    return out


def _state(m):
    torch.cuda.synchronize()
    return R.bits(m.flat_params), R.bits(m.flat_buffers)


@pytest.mark.parametrize("env", [{}, MIX], ids=["alone", "with-mixup-cutmix"])
def test_entrypoint_runs_and_repeats_bit_for_bit(env, tmp_path, capsys, monkeypatch):
    """MX_RANDOM_ERASE=1, alone and beside MX_MIXUP / MX_CUTMIX: the validation loss is finite, the
    erase kernel ran once per training step on the engine's s2d bf16 batch, two identical runs end
    with bit-identical weights and BatchNorm statistics, and a run without the variable does not."""
    models, erases = _capture(monkeypatch)
    for sub in ("a", "b"):
        _run(_cfg(tmp_path / sub, MX_RANDOM_ERASE="1", **env), capsys)
    assert models[0].__class__.__name__ == "NativeResNet"
    assert erases == [((8, 32, 32, 16), torch.bfloat16, 0)] * 6
    a, b = _state(models[0]), _state(models[1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _run(_cfg(tmp_path / "off", **env), capsys)
    assert len(erases) == 6
    assert not torch.equal(a[0], _state(models[2])[0])


def test_suspended_and_resumed_run_ends_with_the_same_weights(tmp_path, capsys, monkeypatch):
    """A run suspended after step 2 and resumed from latest.pt draws step 2's boxes again (the key
    is (seed, rank, epoch, step, position)) and ends with the uninterrupted run's weights."""
    from pytorch_distributed_amd.utils.suspend import REQUEUE_EXIT_CODE
    models, erases = _capture(monkeypatch)
    _run(_cfg(tmp_path / "whole", MX_RANDOM_ERASE="1"), capsys)
    monkeypatch.setenv("MX_SUSPEND_AT_STEP", "2")
    with pytest.raises(SystemExit) as ei:
        trainer.run(_cfg(tmp_path / "cut", MX_RANDOM_ERASE="1"), "single")
    assert ei.value.code == REQUEUE_EXIT_CODE
    monkeypatch.delenv("MX_SUSPEND_AT_STEP")
    assert len(erases) == 5
    out = _run(_cfg(tmp_path / "cut", MX_RANDOM_ERASE="1"), capsys)
    assert "resume: epoch 0 step 2" in out and len(erases) == 6
    whole, cut, resumed = (_state(m) for m in models)
    assert torch.equal(whole[0], resumed[0]) and torch.equal(whole[1], resumed[1])
    assert not torch.equal(whole[0], cut[0])


def test_graph_mode_trains_on_the_erased_batch(tmp_path, capsys, monkeypatch):
    """MX_GRAPH=1 needs no refusal: the captured step copies the batch it is handed, after the erase
    and on the same stream, so three replayed steps end with the eager run's weights."""
    models, erases = _capture(monkeypatch)
    _run(_cfg(tmp_path / "eager", MX_RANDOM_ERASE="1"), capsys)
    _run(_cfg(tmp_path / "graph", MX_RANDOM_ERASE="1", MX_GRAPH="1"), capsys)
    assert len(erases) == 6
    eager, graph = _state(models[0]), _state(models[1])
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
