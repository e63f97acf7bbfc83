"""Label smoothing, mixup and CutMix through the native engine: ResNet-18 at 32 px, batch 8 (the
model of tests/test_optim_gpu.py) against the torch fp32 model on the same weights and the same
mixed batch; the AMP path; and the default path left bit-identical."""
import copy

import pytest
import torch

import head_refs as H
import mix_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S, B = 32, 8


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _pair(dtype=torch.bfloat16):
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.models.native import NativeResNet
    torch.manual_seed(0)
    ref = build_model("resnet18")
    tm = copy.deepcopy(ref).to(DEV)
    return tm, NativeResNet(ref, device=DEV, dtype=dtype, image_size=S)


def _batch(nm):
    from pytorch_distributed_amd.data import SyntheticImageNet
    return nm.input_generator(SyntheticImageNet("train", image_size=S))(torch.arange(B))


@pytest.mark.parametrize("mode", ["mixup", "cutmix"])
def test_native_step_matches_fp32_on_the_same_mixed_batch(mode):
    """Smoothing 0.1 plus a fixed mixup draw (lam 0.3) / a fixed CutMix box: the batch is mixed by
    batch_mix in the engine's s2d bf16 layout, and the torch fp32 model and torch's bf16 autocast
    get the same mixed pixels as NCHW with SoftCrossEntropy. Bounds of
    tests/test_native_model_gpu.py::test_forward_backward_matches_reference for the same model:
    |loss - fp32| < 2 * |bf16 autocast - fp32| + 0.02, and every fc gradient's relative error
    <= 1.5 * autocast's + 0.02."""
    from pytorch_distributed_amd.mix import SoftCrossEntropy
    from pytorch_distributed_amd.ops import native_ops as K
    tm, nm = _pair()
    tb = copy.deepcopy(tm)
    x, y = _batch(nm)
    if mode == "mixup":
        kind, lam, box = K.MIX_MIXUP, 0.3, None
    else:
        kind, box = K.MIX_CUTMIX, (4, 20, 9, 30)
        lam = 1.0 - (20 - 4) * (30 - 9) / (S * S)
    mixed = torch.empty_like(x)
    K.batch_mix(x, mixed, K.AUG_S2D, kind, lam, box)
    torch.cuda.synchronize()
    assert _mixed_ok(mixed, x.cpu(), kind, lam, box)
    yb = y.roll(1, 0)
    xt = R.nchw_from_s2d(mixed.cpu()).float().to(DEV)        # the same pixels, exactly
    tm.train(), tb.train(), nm.train()
    soft = SoftCrossEntropy(0.1)
    loss_t = soft(tm(xt), y, yb, lam)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb = tb(xt)
    loss_b = soft(lb.float(), y, yb, lam)
    crit = nm.make_criterion(label_smoothing=0.1)
    loss_n = crit(nm(mixed), y, yb, lam)
    d_n, d_b = abs(loss_n.item() - loss_t.item()), abs(loss_b.item() - loss_t.item())
    print(f"{mode}: loss fp32 {loss_t.item():.6f}, native off by {d_n:.3g}, bf16 autocast by {d_b:.3g}")
    assert d_n < 2 * d_b + 0.02
    loss_t.backward(), loss_b.backward(), loss_n.backward()
    torch.cuda.synchronize()
    tp, bp = dict(tm.named_parameters()), dict(tb.named_parameters())
    seen = 0
    for name, p in nm.named_parameters():
        if not name.startswith("fc."):
            continue
        e, eb = rel_err(p.grad, tp[name].grad), rel_err(bp[name].grad, tp[name].grad)
        print(f"{mode}: {name} grad rel err native {e:.3g}, bf16 autocast {eb:.3g}")
        assert e <= 1.5 * eb + 0.02, (name, e, eb)
        seen += 1
    assert seen == 2
    # the hard-label loss on the same logits is another number: the soft target reached the kernel
    with torch.no_grad():
        hard = nm.make_criterion()(nm(mixed), y)
    assert abs(hard.item() - loss_n.item()) > 1e-4


def _mixed_ok(got, x, kind, lam, box):
    """The batch is the mixed one, by the checks of tests/test_batch_mix_gpu.py: CutMix bit-equal,
    mixup within ulp_out + 3 * 2^-24 * (|lam*a| + |(1-lam)*b|)."""
    got = got.cpu()
    ref = R.batch_mix_ref(x, R.S2D, kind, lam, box)
    if kind == R.CUTMIX:
        return H.same_bits(got, ref)
    lam32, oml32 = R.f32_weights(lam)
    extra = 3 * 2.0 ** -24 * ((lam32 * x.double()).abs() + (oml32 * x.roll(1, 0).double()).abs())
    return bool(H.within_ulp(got, ref, got.dtype, extra=extra)[0].all())


def test_amp_scaled_backward_is_the_unscaled_one_times_the_scale():
    """scaler.scale(loss).backward() through xent_soft's device scale, against loss.backward() on
    the same model and batch: bf16, scale 1024. A power-of-two scale commutes with every rounding
    of the backward pass (bf16 and f32 share their exponent range; nothing under- or overflows), so
    the scaled gradients are the unscaled ones times 1024 up to f32 summation order: relative
    error <= 1e-6 over the whole flat gradient and over the fc gradients."""
    from pytorch_distributed_amd.amp import LossScaler
    _, nm = _pair()
    x, y = _batch(nm)
    yb, lam = y.roll(1, 0), 0.3
    crit = nm.make_criterion(label_smoothing=0.1)
    nm.train()
    crit(nm(x), y, yb, lam).backward()
    torch.cuda.synchronize()
    plain = nm.flat_grad.clone()
    assert bool(plain.isfinite().all()) and float(plain.abs().max()) > 0
    nm.zero_grad_flat()
    scaler = LossScaler(init_scale=1024.0, growth_interval=1000)
    scaler.scale(crit(nm(x), y, yb, lam)).backward()
    torch.cuda.synchronize()
    scaled = nm.flat_grad.clone()
    assert rel_err(scaled, plain * 1024.0) <= 1e-6
    fc = slice(nm.fc_w_off, nm.fc_w_off + nm.num_classes * nm.feat_dim)
    assert rel_err(scaled[fc], plain[fc] * 1024.0) <= 1e-6


def test_amp_fp16_fc_gradients_follow_the_loss_scale():
    """The path the AMP script runs: an fp16 model and LossScaler's default scale 2^16 through
    _XentSoftFn.backward (xent_soft's gdev). The fc gradients come straight from the fp16 dlog, so
    they are checked: scaled / 2^16 against the unscaled backward. Both paths round an entry of dlog
    alike (a power-of-two scale commutes with the rounding) unless the unscaled entry is subnormal
    in fp16, where it is off by at most 2^-25, against label entries of order 0.1 / B; norm-wise
    that is orders below one fp16 spacing, 2^-10, which is the (loose) bound. A gradient that
    missed the scale would be off by a factor 65536."""
    from pytorch_distributed_amd.amp import LossScaler
    _, nm = _pair(torch.float16)
    x, y = _batch(nm)
    yb, lam = y.roll(1, 0), 0.3
    crit = nm.make_criterion(label_smoothing=0.1)
    nm.train()
    crit(nm(x), y, yb, lam).backward()
    torch.cuda.synchronize()
    plain = nm.flat_grad.clone()
    nm.zero_grad_flat()
    scaler = LossScaler()
    scaler.scale(crit(nm(x), y, yb, lam)).backward()
    torch.cuda.synchronize()
    assert scaler.get_scale() == 65536.0
    scaled = nm.flat_grad.clone()
    for name, sl in (("fc.weight", slice(nm.fc_w_off, nm.fc_w_off + nm.num_classes * nm.feat_dim)),
                     ("fc.bias", slice(nm.fc_b_off, nm.fc_b_off + nm.num_classes))):
        assert bool(plain[sl].isfinite().all()) and float(plain[sl].abs().max()) > 0, name
        e = rel_err(scaled[sl] / 65536.0, plain[sl])
        print(f"fp16 AMP {name}: scaled / 2^16 vs unscaled, relative error {e:.3g}")
        assert e <= 2.0 ** -10, (name, e)


def test_default_path_is_bit_identical_to_the_direct_xent_step(monkeypatch):
    """All three off: two eager steps through make_criterion() (the trainer's calls) leave weights
    and momentum bit-identical to two steps that call K.xent directly
    (runtime.graphs.native_train_step, the code path before label smoothing existed)."""
    from pytorch_distributed_amd.models.native import NativeCrossEntropy
    from pytorch_distributed_amd.runtime.graphs import native_train_step
    from pytorch_distributed_amd.ops import native_ops as K
    _, a = _pair()
    _, b = _pair()
    assert torch.equal(a.flat_params, b.flat_params)
    oa, ob = a.make_optimizer(lr=0.1), b.make_optimizer(lr=0.1)
    crit = a.make_criterion()
    assert type(crit) is NativeCrossEntropy and crit.label_smoothing == 0.0
    calls = []
    real = K.xent_soft
    monkeypatch.setattr(K, "xent_soft", lambda *p, **k: calls.append(1) or real(*p, **k))
    a.train(), b.train()
    for i in range(2):
        x, y = _batch(a)
        oa.zero_grad()
        loss_a = crit(a(x), y)
        loss_a.backward()
        oa.step()
        loss_b = native_train_step(b, ob, x, y)
        torch.cuda.synchronize()
        assert torch.equal(loss_a.detach(), loss_b)
    assert not calls, "the default criterion must stay on xent_kernel"
    assert torch.equal(a.flat_params, b.flat_params) and torch.equal(oa.flat_mom, ob.flat_mom)
    assert not torch.equal(a.flat_params, _pair()[1].flat_params)
