"""Parameter groups, configuration and refusals of the grouped optimizer that need no GPU, the
host-side table check of the segmented kernels, and one CLI run on the CPU with every knob set."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from pytorch_distributed_amd.config import config_for, parse_cli
from pytorch_distributed_amd.models import build_model
from pytorch_distributed_amd.optim import LARS, build_param_groups, normalize_param_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=False, lars=0.0, lars_eps=1e-8,
                dampening=0.0)


# ------------------------------------------------------------------ build_param_groups
@pytest.mark.parametrize("arch,mats,vecs", [("resnet18", 21, 41), ("resnet50", 54, 107)])
def test_param_group_census(arch, mats, vecs):
    """ResNet-18: 20 conv weights + the fc weight have dim() >= 2; 20 BatchNorm weight / bias pairs +
    the fc bias are 1-D. ResNet-50: 53 + 1 and 2 * 53 + 1."""
    m = build_model(arch)
    n = len(list(m.parameters()))
    assert n == mats + vecs
    one = build_param_groups(m, 1e-4)
    assert len(one) == 1 and len(one[0]["params"]) == n and one[0]["weight_decay"] == 1e-4
    assert "lars" not in one[0]
    g = build_param_groups(m, 1e-4, no_bn_decay=True)
    assert [len(x["params"]) for x in g] == [mats, vecs]
    assert all(p.dim() >= 2 for p in g[0]["params"]) and all(p.dim() == 1 for p in g[1]["params"])
    assert g[0]["weight_decay"] == 1e-4 and g[1]["weight_decay"] == 0.0
    g = build_param_groups(m, 1e-4, no_bn_decay=False, lars=0.001)
    assert [len(x["params"]) for x in g] == [mats, vecs]
    assert (g[0]["lars"], g[1]["lars"]) == (0.001, 0.0)          # the usual exclusion
    assert g[0]["weight_decay"] == g[1]["weight_decay"] == 1e-4
    g = build_param_groups(m, 1e-4, no_bn_decay=True, lars=0.001)
    assert (g[1]["weight_decay"], g[1]["lars"]) == (0.0, 0.0)
    ids = [id(p) for x in g for p in x["params"]]
    assert sorted(ids) == sorted(id(p) for p in m.parameters()) and len(set(ids)) == n
    with pytest.raises(ValueError):
        build_param_groups(m, 1e-4, lars=-0.001)
    # torch accepts the groups as they are (custom keys ride along)
    torch.optim.SGD(g, lr=0.1, momentum=0.9, nesterov=True)
    LARS(g, lr=0.1, momentum=0.9, nesterov=True)


# ------------------------------------------------------------------ config
def test_config_parses_the_optimizer_variables():
    c = config_for("single", env={})
    assert (c.nesterov, c.no_bn_decay, c.lars) == (False, False, 0.0)
    c = config_for("single", env={"MX_NESTEROV": "1", "MX_NO_BN_DECAY": "true", "MX_LARS": "0.001"})
    assert (c.nesterov, c.no_bn_decay, c.lars) == (True, True, 0.001)
    c = config_for("ddp", env={"MX_NESTEROV": "0", "MX_NO_BN_DECAY": "false"})
    assert (c.nesterov, c.no_bn_decay) == (False, False)
    c = config_for("ddp", env={}, argv=["--nesterov", "1", "--no-bn-decay", "1", "--lars", "0.002"])
    assert (c.nesterov, c.no_bn_decay, c.lars) == (True, True, 0.002)
    assert set(parse_cli(["--lars", "0.5"])) == {"MX_LARS"}
    for bad in ("-0.001", "nan", "inf"):
        with pytest.raises(ValueError, match="MX_LARS"):
            config_for("single", env={"MX_LARS": bad})


def test_trainer_builds_what_it_built_before_without_the_variables():
    from pytorch_distributed_amd import trainer
    m = build_model("resnet18", 10)
    ctx = trainer.Context(cfg=config_for("single", env={}), device=torch.device("cpu"),
                          dtype=torch.float32, engine="torch")
    opt = trainer.build_optimizer(ctx.cfg, m, ctx)
    assert type(opt) is torch.optim.SGD and len(opt.param_groups) == 1
    assert not opt.param_groups[0]["nesterov"] and opt.param_groups[0]["weight_decay"] == 1e-4
    cfg = config_for("single", env={"MX_NO_BN_DECAY": "1", "MX_NESTEROV": "1"})
    opt = trainer.build_optimizer(cfg, m, ctx)
    assert type(opt) is torch.optim.SGD and [len(g["params"]) for g in opt.param_groups] == [21, 41]
    assert all(g["nesterov"] for g in opt.param_groups) and opt.param_groups[1]["weight_decay"] == 0
    cfg = config_for("single", env={"MX_LARS": "0.001"})
    opt = trainer.build_optimizer(cfg, m, ctx)
    assert type(opt) is LARS and [g["lars"] for g in opt.param_groups] == [0.001, 0.0]


def test_trainer_refuses_groups_with_graph_capture_before_training():
    """MX_GRAPH=1 with any of the variables on the native engine: ValueError from build_optimizer,
    naming MX_GRAPH / DataParallel, before the model is asked for anything."""
    from pytorch_distributed_amd import trainer

    class FakeNative(torch.nn.Module):
        def make_optimizer(self, **kw):
            raise AssertionError("the refusal comes first")

    for var in ("MX_NESTEROV", "MX_NO_BN_DECAY", "MX_LARS"):
        cfg = config_for("single", env={"MX_GRAPH": "1", var: "0.5" if var == "MX_LARS" else "1"})
        ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.bfloat16, engine="native")
        with pytest.raises(ValueError, match="MX_GRAPH.*DataParallel|DataParallel.*MX_GRAPH"):
            trainer.build_optimizer(cfg, FakeNative(), ctx)


# ------------------------------------------------------------------ group refusals (NativeSGD's)
def test_group_refusals():
    m = build_model("resnet18", 10)
    ps = list(m.parameters())
    other = torch.nn.Parameter(torch.zeros(3))
    ok = normalize_param_groups(ps, [{"params": ps[:3], "lr": 0.5}, {"params": ps[5:6], "lars": 0.01}],
                                DEFAULTS)
    assert [len(g["params"]) for g in ok] == [3, 1]          # the rest is frozen
    assert ok[0]["lr"] == 0.5 and ok[0]["momentum"] == 0.9 and ok[1]["lars"] == 0.01
    assert ok[0]["lars"] == 0.0 and ok[0]["lars_eps"] == 1e-8
    assert len(normalize_param_groups(ps, None, DEFAULTS)[0]["params"]) == len(ps)
    bad = [
        [{"params": [other]}],                                        # not the model's
        [{"params": ps[:2]}, {"params": ps[1:3]}],                    # in two groups
        [{"params": [ps[0], ps[0]]}],
        [{"params": ps[:2], "learning_rate": 0.1}],                   # unknown key
        [{"params": ps[:2], "lr": -0.1}],
        [{"params": ps[:2], "momentum": -0.9}],
        [{"params": ps[:2], "weight_decay": -1e-4}],
        [{"params": ps[:2], "lars": -0.001}],
        [{"params": ps[:2], "lars_eps": -1e-8}],
        [{"params": ps[:2], "nesterov": True, "momentum": 0.0}],      # torch's rule
        [{"params": ps[:2], "dampening": 0.1}],
        [{"lr": 0.1}],
    ]
    for groups in bad:
        with pytest.raises(ValueError):
            normalize_param_groups(ps, groups, DEFAULTS)
    with pytest.raises(ValueError):
        normalize_param_groups(ps, None, {**DEFAULTS, "nesterov": True, "momentum": 0.0})
    with pytest.raises(ValueError):
        normalize_param_groups(ps, None, {**DEFAULTS, "lr": -1.0})
    with pytest.raises(ValueError):
        LARS(ps, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        LARS(ps, lr=0.1, lars=-1.0)


def test_native_sgd_knows_which_arguments_need_segments():
    from pytorch_distributed_amd.models.native import NativeSGD
    assert not NativeSGD.wants_segments(lr=0.1, momentum=0.9, weight_decay=1e-4)
    assert NativeSGD.wants_segments(nesterov=True)
    assert NativeSGD.wants_segments(lars=0.001)
    assert NativeSGD.wants_segments(param_groups=[])


# ------------------------------------------------------------------ host-side table check
def test_segment_tables_and_their_host_check():
    """seg_tables cuts segments into SEG_CHUNK-element blocks; pda_seg_check (what the launchers run
    before every launch) accepts them and names each defect by its own code."""
    from pytorch_distributed_amd.ops import ext, native_ops as K
    L = ext.load(required=True)
    assert L.pda_seg_chunk() == K.SEG_CHUNK and K.SEG_CHUNK % 4 == 0
    assert C.sizeof(K.SegRow) == 48 and C.sizeof(K.BlkRow) == 16

    def tables(segs, hyper=None):
        t, nb = K.seg_tables(segs, hyper or [dict(lr=0.1)] * len(segs), device=None)   # host rows only
        assert nb == t.nblocks == sum(-(-n // K.SEG_CHUNK) for _, n in segs) and t.nseg == len(segs)
        return t

    def chk(t, n):
        return L.pda_seg_check(t.seg_host, t.nseg, t.blk_host, t.nblocks, n)

    S = K.SEG_CHUNK
    t = tables([(0, 5), (8, S + 1), (3 * S, 3 * S + 5)])
    assert [(b.first, b.seg, b.count) for b in t.blk_host] == [
        (0, 0, 5), (8, 1, S), (8 + S, 1, 1), (3 * S, 2, S), (4 * S, 2, S), (5 * S, 2, S), (6 * S, 2, 5)]
    assert [(s.blk0, s.nblk) for s in t.seg_host] == [(0, 1), (1, 2), (3, 4)]
    assert chk(t, 6 * S + 5) == 0 and chk(t, 10 ** 7) == 0
    assert chk(t, 6 * S + 4) == -3                                   # past n
    assert chk(tables([(2, 4)]), 100) == -2                          # offset % 4
    assert chk(tables([(0, 8), (4, 8)]), 100) == -4                  # overlap
    assert chk(tables([(16, 8), (0, 17)]), 100) == -4
    assert chk(tables([(0, 8)], [dict(lr=-1.0)]), 100) == -5
    assert chk(tables([(0, 8)], [dict(lr=0.1, lars=float("nan"))]), 100) == -5
    skipped = (K.BlkRow * (t.nblocks - 1))(*[b for i, b in enumerate(t.blk_host) if i != 4])
    assert chk(K.SegTables(t.seg_host, skipped, None), 10 ** 7) == -6
    with pytest.raises(ValueError, match="GPU"):
        K.sgd_seg(torch.zeros(8), torch.zeros(8), torch.zeros(8), None, t, False)
    t.blk_host[1].count = S - 4                                       # a hole inside a segment
    assert chk(t, 10 ** 7) == -6
    with pytest.raises(ValueError):
        K.seg_tables([(0, 8)], [])
    with pytest.raises(ValueError):
        K.seg_tables([(0, 8)], [dict(lr=0.1, beta=0.9)])


# ------------------------------------------------------------------ CLI
def _cli(tmp_path, sub, **kw):
    d = tmp_path / sub
    d.mkdir()
    e = dict(os.environ)
    e.update({"MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
              "MX_BATCH": "4", "MX_IMAGE_SIZE": "32", "MX_NUM_CLASSES": "10", "MX_DEVICE": "cpu",
              "PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2"})
    e.update(kw)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "resnet_single_gpu.py")], cwd=d, env=e,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Epoch: 0, Loss: ")]
    assert len(lines) == 1 and "cost time per epoch: " in r.stdout, r.stdout
    return lines[0]


def test_cli_cpu_knobs_reach_the_optimizer(tmp_path):
    """resnet18, two steps on the CPU with MX_NO_BN_DECAY, MX_NESTEROV and MX_LARS set: exits 0 with
    the usual log lines, and the validation loss after the two steps differs from the run without
    them (same seed, same data): the knobs reach the optimizer."""
    plain = _cli(tmp_path, "plain")
    knobs = _cli(tmp_path, "knobs", MX_NO_BN_DECAY="1", MX_NESTEROV="1", MX_LARS="0.001")
    assert plain != knobs, (plain, knobs)
