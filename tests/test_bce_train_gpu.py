"""NativeBCE through the native engine (ResNet-18, 32 px, batch 8) against tests/bce_refs.py on the
model's own logits; the AMP overflow skip; the captured-step refusal."""
import pytest
import torch
import torch.nn.functional as F

import bce_refs as R
import head_refs as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S, B = 32, 8


def _model(dtype):
    from pytorch_distributed_amd.data import SyntheticImageNet
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.models.native import NativeResNet
    torch.manual_seed(0)
    nm = NativeResNet(build_model("resnet18"), device=DEV, dtype=dtype, image_size=S)
    x, y = nm.input_generator(SyntheticImageNet("train", image_size=S))(torch.arange(B))
    return nm.train(), x, y


def test_loss_and_bias_gradient_follow_the_float64_bce_of_the_logits():
    """bf16, smoothing 0.1, two label sets, lam 0.4. Loss: the f32 bar of test_bce_gpu.py. The fc bias
    gradient is the column sum of the bf16 dlog left in _pending_dlog16: B addends, each within 1 bf16
    ulp of the rounded reference (ulp at the column's largest entry), plus the f32 accumulation."""
    nm, x, y = _model(torch.bfloat16)
    yb, lam, crit = y.roll(1, 0), 0.4, nm.make_criterion(label_smoothing=0.1, loss="bce")
    assert type(crit).__name__ == "NativeBCE" and crit.soft_targets
    logits = nm(x)
    loss = crit(logits, y, yb, lam)
    loss.backward()
    z = logits.detach()
    rows, t, d = R.bce_soft_ref(z.cpu(), y.cpu(), yb.cpu(), R.f32(lam), R.f32(0.1))
    want = float(rows.mean())
    yard = abs(float(F.binary_cross_entropy_with_logits(z.contiguous(), t.float().to(DEV))) - want)
    print(f"loss {loss.item():.7f}: off by {abs(loss.item() - want):.3g}, torch f32 by {yard:.3g}")
    assert abs(loss.item() - want) <= 4 * yard + float(H.ulp_out(rows.mean(), torch.float32))
    got = nm.flat_grad[nm.fc_b_off:nm.fc_b_off + nm.num_classes].cpu().double()
    d16 = d.to(torch.bfloat16).double()
    bound = B * H.ulp_out(d.abs().max(0).values, torch.bfloat16) + B * 2.0 ** -24 * d16.abs().sum(0)
    assert float(got.abs().max()) > 0 and bool(((got - d16.sum(0)).abs() <= bound).all())


@pytest.mark.parametrize("scale,moves", [(2.0 ** 40, False), (2.0 ** 10, True)])
def test_amp_step_skips_on_overflow(scale, moves):
    """fp16: at scale 2^40 dlog (order 2^40 / (B*K)) overflows and the step is skipped; at 2^10 not."""
    from pytorch_distributed_amd.amp import LossScaler
    nm, x, y = _model(torch.float16)
    opt, crit = nm.make_optimizer(lr=0.1), nm.make_criterion(label_smoothing=0.1, loss="bce", target_thresh=0.05)
    scaler, before = LossScaler(init_scale=scale), nm.flat_params.clone()
    scaler.scale(crit(nm(x), y, y.roll(1, 0), 0.4)).backward()
    scaler.step(opt), scaler.update()
    assert torch.equal(nm.flat_params, before) != moves and bool(nm.flat_params.isfinite().all())
    assert scaler.get_scale() == (scale if moves else scale / 2)


def test_captured_step_refuses_bce_before_any_launch():
    """MX_GRAPH=1: refused before the model is touched (there is none), so before any launch."""
    from pytorch_distributed_amd import config, trainer
    ctx = trainer.Context(config.config_for("single", env={"MX_LOSS": "bce", "MX_GRAPH": "1"}), DEV, torch.bfloat16, "native")
    with pytest.raises(ValueError, match="MX_GRAPH.*MX_LOSS=bce"):
        trainer.build_criterion(ctx, None)
