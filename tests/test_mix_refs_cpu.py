"""The references of tests/mix_refs.py against torch, and the properties of draw_mix (no GPU)."""
import math

import pytest
import torch
import torch.nn.functional as F

import head_refs as H
import mix_refs as R

F64 = torch.float64


def _case(B=6, K=11, seed=0):
    g = H._gen(seed)
    x = torch.randn(B, K, generator=g, dtype=F64) * 3
    a = torch.randint(0, K, (B,), generator=g)
    return x, a, a.roll(1, 0)


def test_xent_soft_ref_reduces_to_the_hard_label_reference():
    x, a, _ = _case()
    rows, grad = R.xent_soft_ref(x, a, None, 1.0, 0.0)
    rows_h, grad_h = H.xent_ref(x, a)
    torch.testing.assert_close(rows, rows_h, rtol=0, atol=1e-13)
    torch.testing.assert_close(grad, grad_h, rtol=0, atol=1e-15)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_xent_soft_ref_matches_torch_and_its_autograd(eps, lam):
    x, a, b = _case(seed=1)
    x.requires_grad_(True)
    want = (lam * F.cross_entropy(x, a, label_smoothing=eps, reduction="none")
            + (1 - lam) * F.cross_entropy(x, b, label_smoothing=eps, reduction="none"))
    want.sum().backward()
    rows, grad = R.xent_soft_ref(x.detach(), a, b, lam, eps)
    torch.testing.assert_close(rows, want.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(grad, x.grad, rtol=0, atol=1e-12)
    # b = None means b = a
    r2, g2 = R.xent_soft_ref(x.detach(), a, None, lam, eps)
    r3, g3 = R.xent_soft_ref(x.detach(), a, a, lam, eps)
    assert torch.equal(r2, r3) and torch.equal(g2, g3)


def test_s2d_relayout_follows_the_stem_formula():
    """X'[b][i][j][(p*2+q)*3+c] == x[b][c][2i+p][2j+q] element by element, padding slots 0, and the
    inverse restores the image."""
    g = H._gen(2)
    x = torch.randn(2, 3, 6, 6, generator=g)
    s = R.s2d_from_nchw(x)
    assert s.shape == (2, 3, 3, 16) and bool((s[..., 12:] == 0).all())
    for b in range(2):
        for i in range(3):
            for j in range(3):
                for k in range(12):
                    pq, c = divmod(k, 3)
                    assert s[b, i, j, k] == x[b, c, 2 * i + (pq >> 1), 2 * j + (pq & 1)]
    assert torch.equal(R.nchw_from_s2d(s), x)


@pytest.mark.parametrize("mode,lam,box", [(R.MIXUP, 0.3, None), (R.MIXUP, 1.0, None), (R.MIXUP, 0.0, None),
                                          (R.CUTMIX, 0.5, (1, 4, 3, 5)), (R.CUTMIX, 0.5, (0, 6, 0, 6)),
                                          (R.CUTMIX, 0.5, (2, 2, 0, 6))])
def test_batch_mix_ref_s2d_is_the_relaid_nchw_result(mode, lam, box):
    g = H._gen(3)
    x = torch.randn(3, 3, 6, 6, generator=g)
    n = R.batch_mix_ref(x, R.NCHW, mode, lam, box)
    s = R.batch_mix_ref(R.s2d_from_nchw(x), R.S2D, mode, lam, box)
    assert torch.equal(s, R.s2d_from_nchw(n))
    # against a direct statement of the operation
    part = x.roll(1, 0)
    if mode == R.MIXUP:
        lam32, oml32 = R.f32_weights(lam)
        assert torch.equal(n, lam32 * x.to(F64) + oml32 * part.to(F64))
        if lam == 1.0:
            assert torch.equal(n, x.to(F64))
        if lam == 0.0:
            assert torch.equal(n, part.to(F64))
    else:
        y1, y2, x1, x2 = box
        want = x.clone()
        want[:, :, y1:y2, x1:x2] = part[:, :, y1:y2, x1:x2]
        assert torch.equal(n, want)
    one = torch.randn(1, 3, 4, 4, generator=g)          # B = 1: mixed with itself
    assert torch.equal(R.batch_mix_ref(one, R.NCHW, R.CUTMIX, 0.5, (0, 2, 0, 2)), one)


def test_f32_weights_are_float32_values():
    lam32, oml32 = R.f32_weights(0.3)
    assert lam32 == float(torch.tensor(0.3, dtype=torch.float32)) and lam32 != 0.3
    assert oml32 == float(torch.tensor(1.0) - torch.tensor(0.3))
    assert R.f32_weights(1.0) == (1.0, 0.0) and R.f32_weights(0.0) == (0.0, 1.0)
    from pytorch_distributed_amd.ops.native_ops import mix_weights
    for lam in (0.0, 1.0, 0.3, 0.5, 1e-9, 0.999999):
        assert mix_weights(lam) == R.f32_weights(lam)


# ------------------------------------------------------------------ draw_mix
def _draw(*a, **k):
    from pytorch_distributed_amd.mix import draw_mix
    return draw_mix(*a, **k)


def test_draw_mix_is_a_pure_function_of_its_arguments():
    base = _draw(0, 0, 0, 0, 224, 0.2, 1.0)
    assert base == _draw(0, 0, 0, 0, 224, 0.2, 1.0)
    seen = {base}
    for args in ((0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 0)):
        seen.add(_draw(*args, 224, 0.2, 1.0))
    assert len(seen) == 5                      # rank, epoch, step and seed each change the draw
    # a resumed run draws what the uninterrupted run drew at that step
    assert [_draw(3, 2, 1, s, 64, 0.2, 1.0) for s in range(5, 9)] == \
           [_draw(3, 2, 1, s, 64, 0.2, 1.0) for s in range(9)][5:]


def test_draw_mix_ranges_box_and_switches():
    from pytorch_distributed_amd.mix import CUTMIX, MIXUP
    assert _draw(0, 0, 0, 0, 32, 0.0, 0.0) == (None, 1.0, None)
    for S in (4, 32, 224):
        for step in range(300):
            mode, lam, box = _draw(1, 0, 0, step, S, 0.0, 1.0)
            assert mode == CUTMIX and 0.0 <= lam <= 1.0
            y1, y2, x1, x2 = box
            assert 0 <= y1 <= y2 <= S and 0 <= x1 <= x2 <= S
            assert lam == 1.0 - (x2 - x1) * (y2 - y1) / (S * S)      # exactly
            mode, lam, box = _draw(1, 0, 0, step, S, 0.4, 0.0)
            assert mode == MIXUP and box is None and 0.0 <= lam <= 1.0
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            _draw(0, 0, 0, 0, 32, bad, 1.0)


@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_draw_mix_statistics(alpha):
    """Over n = 4000 steps: the mixup lam has mean 1/2 within 5 standard errors (Beta(a, a) has
    variance 1 / (4 (2a + 1))); with both modes on, each mode's share is within 5 standard errors
    (sqrt(1/4 / n)) of 1/2."""
    from pytorch_distributed_amd.mix import CUTMIX, MIXUP
    n = 4000
    lams = [_draw(7, 0, 0, s, 224, alpha, 0.0)[1] for s in range(n)]
    se = math.sqrt(1.0 / (4 * (2 * alpha + 1)) / n)
    assert abs(sum(lams) / n - 0.5) <= 5 * se
    modes = [_draw(7, 0, 1, s, 224, alpha, 1.0)[0] for s in range(n)]
    assert set(modes) == {MIXUP, CUTMIX}
    assert abs(modes.count(CUTMIX) / n - 0.5) <= 5 * math.sqrt(0.25 / n)
