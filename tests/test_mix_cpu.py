"""Label smoothing / mixup / CutMix without a GPU: configuration, the refusals, BatchMixer and
SoftCrossEntropy on the CPU against tests/mix_refs.py, and the CPU trainer."""
import math

import pytest
import torch
from torch import nn

import head_refs as H
import mix_refs as R
from pytorch_distributed_amd import trainer
from pytorch_distributed_amd.config import config_for, parse_cli

F64 = torch.float64
U24 = 2.0 ** -24


# ------------------------------------------------------------------ config
def test_config_parses_the_three_variables():
    c = config_for("single", env={})
    assert (c.label_smoothing, c.mixup, c.cutmix) == (0.0, 0.0, 0.0) and not c.soft_targets
    c = config_for("ddp", env={"MX_LABEL_SMOOTHING": "0.1", "MX_MIXUP": "0.2", "MX_CUTMIX": "1.0"})
    assert (c.label_smoothing, c.mixup, c.cutmix) == (0.1, 0.2, 1.0) and c.soft_targets
    c = config_for("single", env={}, argv=["--label-smoothing", "0.05", "--mixup", "0.4", "--cutmix", "0.5"])
    assert (c.label_smoothing, c.mixup, c.cutmix) == (0.05, 0.4, 0.5)
    assert set(parse_cli(["--cutmix", "1"])) == {"MX_CUTMIX"}
    for var in ("MX_LABEL_SMOOTHING", "MX_MIXUP", "MX_CUTMIX"):
        assert config_for("single", env={var: "0.5"}).soft_targets
        for bad in ("-0.1", "nan", "inf", "-inf"):
            with pytest.raises(ValueError, match=var):
                config_for("single", env={var: bad})
    for bad in ("1", "1.5"):
        with pytest.raises(ValueError, match="MX_LABEL_SMOOTHING"):
            config_for("single", env={"MX_LABEL_SMOOTHING": bad})
    assert config_for("single", env={"MX_MIXUP": "2.5"}).mixup == 2.5       # an alpha may exceed 1


class _FakeNative(nn.Module):
    def make_criterion(self, **kw):
        raise AssertionError("the refusal comes first")


def test_captured_steps_refuse_soft_targets_before_training():
    """MX_GRAPH=1 on the native engine, and DataParallel with replicas, with any of the three
    variables: ValueError from build_criterion, before the model is asked for anything."""
    for var in ("MX_LABEL_SMOOTHING", "MX_MIXUP", "MX_CUTMIX"):
        cfg = config_for("single", env={"MX_GRAPH": "1", var: "0.1"})
        ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.bfloat16, engine="native")
        with pytest.raises(ValueError, match="MX_GRAPH.*MX_LABEL_SMOOTHING"):
            trainer.build_criterion(ctx, _FakeNative())
        cfg = config_for("dp", env={var: "0.1"})
        ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.bfloat16, engine="native")
        dp = _FakeNative()
        dp.replicas = [object()]
        with pytest.raises(ValueError, match="DataParallel"):
            trainer.build_criterion(ctx, dp)
    # MX_GRAPH=1 without them still builds
    cfg = config_for("single", env={"MX_GRAPH": "1"})
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")
    assert type(trainer.build_criterion(ctx, nn.Linear(2, 2))) is nn.CrossEntropyLoss


def test_build_criterion_per_engine():
    from pytorch_distributed_amd.mix import SoftCrossEntropy
    m = nn.Linear(2, 2)
    mk = lambda **env: trainer.Context(cfg=config_for("single", env=env), device=torch.device("cpu"),
                                       dtype=torch.float32, engine="torch")
    assert type(trainer.build_criterion(mk(), m)) is nn.CrossEntropyLoss
    for env in ({"MX_LABEL_SMOOTHING": "0.1"}, {"MX_MIXUP": "0.2"}, {"MX_CUTMIX": "1"}):
        c = trainer.build_criterion(mk(**env), m)
        assert type(c) is SoftCrossEntropy
        assert c.label_smoothing == float(env.get("MX_LABEL_SMOOTHING", 0))

    class Crit:
        soft_targets = True

        def __init__(self, kw):
            self.kw = kw

    class Native(nn.Module):
        def make_criterion(self, **kw):
            return Crit(kw)
    assert trainer.build_criterion(mk(), Native()).kw == {}                   # today's call
    assert trainer.build_criterion(mk(MX_MIXUP="0.2"), Native()).kw == {}
    assert trainer.build_criterion(mk(MX_LABEL_SMOOTHING="0.1"), Native()).kw == {"label_smoothing": 0.1}

    # the real DataParallel around a torch module (no replicas): its factory's hard-label loss is
    # kept without the variables and replaced by SoftCrossEntropy with any of them
    from pytorch_distributed_amd.parallel.dp import DataParallel
    dp = DataParallel(m)
    assert type(trainer.build_criterion(mk(), dp)) is nn.CrossEntropyLoss
    for env in ({"MX_LABEL_SMOOTHING": "0.1"}, {"MX_MIXUP": "0.2"}, {"MX_CUTMIX": "1"}):
        c = trainer.build_criterion(mk(**env), dp)
        assert type(c) is SoftCrossEntropy
        assert c.label_smoothing == float(env.get("MX_LABEL_SMOOTHING", 0))


# ------------------------------------------------------------------ BatchMixer on the CPU
class _Ctx:
    rank, engine = 0, "torch"


def _mixer(S, mixup, cutmix, seed=0):
    from pytorch_distributed_amd.mix import BatchMixer
    cfg = config_for("single", env={"MX_IMAGE_SIZE": str(S), "MX_MIXUP": str(mixup),
                                    "MX_CUTMIX": str(cutmix), "MX_SEED": str(seed)})
    return BatchMixer(cfg, _Ctx())


@pytest.mark.parametrize("layout,dtype", [(R.NCHW, torch.float32), (R.S2D, torch.float32),
                                          (R.S2D, torch.bfloat16)])
def test_batch_mixer_cpu_matches_the_reference(layout, dtype):
    from pytorch_distributed_amd.mix import CUTMIX, MIXUP, draw_mix
    S, B = 10, 5
    g = H._gen(4)
    img = torch.randn(B, 3, S, S, generator=g).to(dtype)
    x = R.s2d_from_nchw(img) if layout == R.S2D else img
    labels = torch.arange(B) * 3
    x0 = x.clone()
    mixer = _mixer(S, 0.4, 1.0)
    seen, buf = set(), None
    for step in range(12):
        mode, lam, box = draw_mix(0, 0, 2, step, S, 0.4, 1.0)
        out, la, lb, lam_got = mixer(x, labels, 2, step)
        assert lam_got == lam and torch.equal(la, labels) and torch.equal(lb, labels.roll(1, 0))
        assert torch.equal(x, x0) and out.dtype == dtype and out.shape == x.shape
        buf = buf if buf is not None else out.data_ptr()
        assert out.data_ptr() == buf                    # one persistent buffer
        ref = R.batch_mix_ref(x, layout, mode, lam, box)
        if mode == CUTMIX:
            assert H.same_bits(out, ref)
        else:
            lam32, oml32 = R.f32_weights(lam)
            part = x.roll(1, 0).to(F64)
            extra = 3 * U24 * ((lam32 * x.to(F64)).abs() + (oml32 * part).abs())
            ok, worst = H.within_ulp(out, ref, dtype, extra=extra)
            assert bool(ok.all()), worst
        seen.add(mode)
    assert seen == {MIXUP, CUTMIX}
    out2 = mixer(x[:3].contiguous(), labels[:3], 2, 0)[0]          # another shape: a new buffer
    assert out2.shape[0] == 3
    with pytest.raises(ValueError):
        mixer(torch.zeros(2, 5, 7), labels[:2], 0, 0)
    off = _mixer(S, 0.0, 0.0)
    assert off(x, labels, 0, 0) == (x, labels, None, 1.0)


# ------------------------------------------------------------------ criteria on the CPU
@pytest.mark.parametrize("eps,lam", [(0.0, 1.0), (0.1, 1.0), (0.0, 0.3), (0.1, 0.3), (0.1, 0.0)])
def test_soft_cross_entropy_matches_the_reference(eps, lam):
    from pytorch_distributed_amd.mix import SoftCrossEntropy
    from pytorch_distributed_amd.models.native import NativeCrossEntropy
    g = H._gen(5)
    x = (torch.randn(7, 13, generator=g, dtype=F64) * 3).requires_grad_(True)
    a = torch.randint(0, 13, (7,), generator=g)
    b = a.roll(1, 0)
    rows, grad = R.xent_soft_ref(x.detach(), a, b, lam, eps)
    loss = SoftCrossEntropy(eps)(x, a, b, lam)
    loss.backward()
    torch.testing.assert_close(loss.detach(), rows.mean(), rtol=0, atol=1e-12)
    torch.testing.assert_close(x.grad, grad / 7, rtol=0, atol=1e-12)
    # hard labels only (validate's call): the same smoothing, no mixing
    rows_h, _ = R.xent_soft_ref(x.detach(), a, None, 1.0, eps)
    torch.testing.assert_close(SoftCrossEntropy(eps)(x.detach(), a), rows_h.mean(), rtol=0, atol=1e-12)
    # the native criterion without a model / on CPU logits falls back to the same arithmetic (f32)
    x32 = x.detach().float()
    nat = NativeCrossEntropy(None, label_smoothing=eps)
    r32, _ = R.xent_soft_ref(x32.to(F64), a, b, lam, eps)
    torch.testing.assert_close(nat(x32, a, b, lam).to(F64), r32.mean(), rtol=1e-5, atol=1e-5)
    r32h, _ = R.xent_soft_ref(x32.to(F64), a, None, 1.0, eps)
    torch.testing.assert_close(nat(x32, a).to(F64), r32h.mean(), rtol=1e-5, atol=1e-5)


def test_criteria_refuse_bad_smoothing():
    from pytorch_distributed_amd.mix import SoftCrossEntropy
    from pytorch_distributed_amd.models.native import NativeCrossEntropy
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            SoftCrossEntropy(bad)
        with pytest.raises(ValueError):
            NativeCrossEntropy(None, label_smoothing=bad)


def test_wrappers_validate_on_the_host():
    """xent_soft_check / batch_mix_check are pure Python: the refusals need no GPU."""
    from pytorch_distributed_amd.ops import native_ops as K
    x, lab = torch.zeros(4, 10), torch.zeros(4, dtype=torch.int64)
    assert K.xent_soft_check(x, lab, lab.clone(), 0.3, 0.1) == (4, 10)
    for kw in (dict(eps=1.0), dict(eps=-0.1), dict(lam=1.5), dict(lam=-0.1), dict(lam=float("nan")),
               dict(labels_b=torch.zeros(3, dtype=torch.int64)),
               dict(labels_b=torch.zeros(4, dtype=torch.int32))):
        a = dict(labels_b=None, lam=1.0, eps=0.0)
        a.update(kw)
        with pytest.raises(ValueError):
            K.xent_soft_check(x, lab, a["labels_b"], a["lam"], a["eps"])
    s = torch.zeros(2, 4, 4, 16, dtype=torch.bfloat16)
    assert K.batch_mix_check(s, torch.zeros_like(s), K.AUG_S2D, K.MIX_CUTMIX, 0.5, (0, 8, 1, 3)) == \
        (2, 8, (0, 8, 1, 3))
    n = torch.zeros(2, 3, 6, 6)
    assert K.batch_mix_check(n, torch.zeros_like(n), K.AUG_NCHW, K.MIX_MIXUP, 0.5)[:2] == (2, 6)
    bad = [
        (s, s, K.AUG_S2D, K.MIX_MIXUP, 0.5, None),                                 # aliasing
        (s, torch.zeros_like(s), K.AUG_S2D, K.MIX_CUTMIX, 0.5, (0, 9, 0, 8)),       # box past S
        (s, torch.zeros_like(s), K.AUG_S2D, K.MIX_CUTMIX, 0.5, (3, 2, 0, 8)),       # y1 > y2
        (s, torch.zeros_like(s), K.AUG_S2D, K.MIX_CUTMIX, 0.5, None),
        (s, torch.zeros_like(s), K.AUG_S2D, K.MIX_MIXUP, 1.5, None),
        (s, torch.zeros_like(s).float(), K.AUG_S2D, K.MIX_MIXUP, 0.5, None),        # dtype differs
        (n.bfloat16(), n.bfloat16() + 0, K.AUG_NCHW, K.MIX_MIXUP, 0.5, None),       # NCHW is f32
        (n, torch.zeros_like(n), K.AUG_S2D, K.MIX_MIXUP, 0.5, None),                # not s2d
        (n, torch.zeros_like(n), 2, K.MIX_MIXUP, 0.5, None),
        (n, torch.zeros_like(n), K.AUG_NCHW, 2, 0.5, None),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            K.batch_mix_check(*args)
    with pytest.raises(ValueError, match="GPU"):
        K.batch_mix(n, torch.zeros_like(n), K.AUG_NCHW, K.MIX_MIXUP, 0.5)


# ------------------------------------------------------------------ the trainer on the CPU
ALL3 = {"MX_LABEL_SMOOTHING": "0.1", "MX_MIXUP": "0.2", "MX_CUTMIX": "1.0"}


@pytest.mark.parametrize("mode,env", [("single", ALL3), ("dp", ALL3), ("dp", {"MX_LABEL_SMOOTHING": "0.1"}),
                                      ("dp", {"MX_MIXUP": "0.2"})],
                         ids=["single-all", "dp-all", "dp-smoothing", "dp-mixup"])
def test_cpu_run_with_the_variables(mode, env, tmp_path, capsys, monkeypatch):
    """Two steps of trainer.run on the CPU, through the single-GPU script's path and through the
    real DataParallel wrapper (one device, torch module): the run read the variables (the config
    says so, the criterion is SoftCrossEntropy with that smoothing and got four arguments at each
    training step and two in validation, draw_mix ran once per step when a mixing variable is
    set), and the validation loss is finite (its size says nothing: after two steps at lr 0.1 the
    eval-mode BatchNorm of the plain run is as far off)."""
    from pytorch_distributed_amd import mix
    cfg = config_for(mode, env={
        "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
        "MX_BATCH": "4", "MX_IMAGE_SIZE": "32", "MX_NUM_CLASSES": "10", "MX_DEVICE": "cpu",
        "MX_WORKERS": "0", "MX_SAVE_PATH": str(tmp_path / "out"), **env})
    assert cfg.soft_targets
    draws, crits, calls = [], [], []
    real_draw, real_build = mix.draw_mix, trainer.build_criterion
    monkeypatch.setattr(mix, "draw_mix", lambda *a: draws.append(a) or real_draw(*a))

    def build(ctx, model):
        c = real_build(ctx, model)
        c.register_forward_pre_hook(lambda m, args: calls.append(len(args)))
        crits.append(c)
        return c
    monkeypatch.setattr(trainer, "build_criterion", build)
    trainer.run(cfg, mode)
    out = capsys.readouterr().out
    loss = float(out.split("Epoch: 0, Loss: ")[1].split(",")[0])
    assert math.isfinite(loss) and loss > 0
    assert len(crits) == 1 and type(crits[0]) is mix.SoftCrossEntropy
    assert crits[0].label_smoothing == float(env.get("MX_LABEL_SMOOTHING", 0))
    assert calls == [4, 4, 2]
    mixing = "MX_MIXUP" in env or "MX_CUTMIX" in env
    assert [d[3] for d in draws] == ([0, 1] if mixing else [])         # (seed, rank, epoch, step, ...)


class _Loader:
    def __init__(self, n):
        g = H._gen(6)
        self.batches = [(torch.randn(4, 3, 8, 8, generator=g), torch.randint(0, 5, (4,), generator=g))
                        for _ in range(n)]

    def iter_from(self, k):
        return iter(list(enumerate(self.batches))[k:])


class _Recorder(nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, *args):
        self.calls.append(args)
        return nn.functional.cross_entropy(args[0], args[1])


def _train_once(tmp_path, **env):
    cfg = config_for("single", env={"MX_IMAGE_SIZE": "8", "MX_LOG_EVERY": "0", **env})
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")
    torch.manual_seed(0)
    model = nn.Sequential(nn.Flatten(), nn.Linear(192, 5))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    rec = _Recorder()
    loader = _Loader(3)
    n = trainer.train(loader, model, rec, opt, None, 0, ctx, 0, 0.0, tmp_path)
    assert n == 3 and len(rec.calls) == 3
    return rec.calls, loader.batches


def test_train_loop_calls_the_criterion_as_before_without_the_variables(tmp_path):
    calls, batches = _train_once(tmp_path)
    for args, (x, y) in zip(calls, batches):
        assert len(args) == 2 and torch.equal(args[1], y)


def test_train_loop_mixes_and_passes_both_label_sets(tmp_path):
    from pytorch_distributed_amd.mix import draw_mix
    calls, batches = _train_once(tmp_path, MX_MIXUP="0.2", MX_CUTMIX="1.0")
    for step, (args, (x, y)) in enumerate(zip(calls, batches)):
        _, lam, _ = draw_mix(0, 0, 0, step, 8, 0.2, 1.0)
        assert len(args) == 4 and torch.equal(args[1], y) and torch.equal(args[2], y.roll(1, 0))
        assert args[3] == lam
    calls, _ = _train_once(tmp_path, MX_LABEL_SMOOTHING="0.1")
    assert all(len(a) == 4 and a[2] is None and a[3] == 1.0 for a in calls)
