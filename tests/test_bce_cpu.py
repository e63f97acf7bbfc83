"""The sigmoid loss without a GPU: mix.soft_bce / SoftBCE against tests/bce_refs.py and torch,
MX_LOSS / MX_BCE_TARGET_THRESH / MX_BCE_SUM parsing and refusals, and build_criterion."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bce_refs as R
from pytorch_distributed_amd import trainer
from pytorch_distributed_amd.config import config_for
from pytorch_distributed_amd.mix import SoftBCE, SoftCrossEntropy, soft_bce


@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_soft_bce_matches_the_reference(case, sum_classes):
    """float64 in and out, the same definition twice: 1e-12 (values up to K = 37, 1e-16 an operation)."""
    _, eps, second, lam, thresh = case
    g = torch.Generator().manual_seed(3)
    a, b = R.labels_for(5, 37, second, g)
    x = R.logits_for(5, 37, a, b, g, R.F64).requires_grad_()
    rows, t, d = R.bce_soft_ref(x.detach(), a, b, lam, eps, thresh, sum_classes)
    loss = soft_bce(x, a, b, lam, eps, thresh, sum_classes)
    loss.backward()
    torch.testing.assert_close(loss.detach(), rows.mean(), rtol=0, atol=1e-12)
    torch.testing.assert_close(x.grad, d, rtol=0, atol=1e-12)
    if case[0] == "hard" and not sum_classes:      # float32 hard labels: torch's BCE on one-hot targets
        x32 = x.detach().float()
        assert torch.equal(SoftBCE()(x32, a), F.binary_cross_entropy_with_logits(x32, F.one_hot(a, 37).float()))
    if case[0] == "thresh-equal":
        assert bool((t[torch.arange(5), a] == 0).all()) and bool((t[torch.arange(5), b] == 1).all())


def test_config_parses_and_refuses():
    c = config_for("single", env={})
    assert (c.loss, c.bce_target_thresh, c.bce_sum) == ("ce", None, False) and not c.soft_targets
    c = config_for("ddp", env={"MX_LOSS": "bce", "MX_BCE_TARGET_THRESH": "0.2", "MX_BCE_SUM": "1"})
    assert (c.loss, c.bce_target_thresh, c.bce_sum) == ("bce", 0.2, True) and c.soft_targets
    assert config_for("single", env={}, argv=["--loss", "bce", "--bce-target-thresh", "0"]).bce_target_thresh == 0.0
    thresh = [({"MX_LOSS": "bce", "MX_BCE_TARGET_THRESH": v}, "MX_BCE_TARGET_THRESH") for v in ("1", "-0.1", "nan")]
    for env, var in thresh + [({"MX_LOSS": "focal"}, "MX_LOSS"), ({"MX_BCE_TARGET_THRESH": "0.2"}, "MX_LOSS=bce"),
                              ({"MX_BCE_SUM": "1"}, "MX_LOSS=bce")]:
        with pytest.raises(ValueError, match=var):
            config_for("single", env=env)


_Native = type("_Native", (nn.Module,), {"make_criterion": lambda self, **kw: kw})   # hands back its arguments


def _ctx(engine="torch", script="single", **env):
    return trainer.Context(config_for(script, env=env), torch.device("cpu"), torch.float32, engine)


def test_build_criterion_trains_on_bce_validates_on_ce_and_refuses_captured_steps():
    m, ctx = nn.Linear(2, 2), _ctx(MX_LOSS="bce", MX_LABEL_SMOOTHING="0.1", MX_BCE_TARGET_THRESH="0.2")
    c, v = trainer.build_criterion(ctx, m), trainer.build_criterion(ctx, m, train=False)
    assert type(c) is SoftBCE and (c.label_smoothing, c.target_thresh, c.sum_classes) == (0.1, 0.2, False)
    assert type(v) is SoftCrossEntropy and v.label_smoothing == 0.1
    assert trainer.build_criterion(_ctx(MX_LOSS="bce", MX_BCE_SUM="1"), _Native()) == dict(
        label_smoothing=0.0, loss="bce", target_thresh=None, sum_classes=True)
    assert trainer.build_criterion(_ctx(), _Native()) == {}
    dp = _Native()
    dp.replicas = [object()]                                 # (MX_GRAPH=1: tests/test_bce_train_gpu.py)
    with pytest.raises(ValueError, match="DataParallel.*PDA_DP_FORCE_REPLAY=1.*MX_LOSS=bce"):
        trainer.build_criterion(_ctx("native", "dp", MX_LOSS="bce"), dp)
