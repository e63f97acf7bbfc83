"""The EMA references of tests/ema_refs.py against the closed form for a constant p and against
torch.optim.swa_utils.AveragedModel."""
import numpy as np
import pytest
import torch

import ema_refs as R
import head_refs as H

F64 = torch.float64


@pytest.mark.parametrize("warmup", [True, False])
def test_schedule(warmup):
    for t in (0, 1, 8, 80, 10_000):
        w = R.weight(0.99, t, warmup)
        assert w == float(np.float32(w)) and 0 < w < 1
        d = min(0.99, (1 + t) / (10 + t)) if warmup else 0.99
        assert abs(w - (1 - d)) <= 2.0 ** -24
    assert R.weight(0.99, 0, True) == float(np.float32(0.9))          # (1 + 0) / (10 + 0) = 0.1
    assert R.weight(0.99, 10_000, True) == R.weight(0.99, 0, False)   # the decay takes over


@pytest.mark.parametrize("every,warmup", [(1, True), (1, False), (3, True)])
def test_recurrence_matches_the_closed_form_for_constant_p(every, warmup):
    g = H._gen(21)
    e0, p = torch.randn(257, generator=g), torch.randn(257, generator=g)
    steps = 12
    e, bound, n, last = R.run(e0, [p] * steps, 0.9, every, warmup)
    assert n == steps // every and last == (steps // every) * every - 1
    want = R.closed_form(e0, p, [R.weight(0.9, t, warmup) for t in range(n)])
    torch.testing.assert_close(e, want, rtol=1e-13, atol=1e-13)
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-4


def test_recurrence_matches_averaged_model():
    """Without warmup: AveragedModel copies the model at its first update and then averages with
    lerp(e, p, 1 - decay) -- the recurrence from e_0 = p_0 over p_1.. in float64. The reference's
    float32 w is off the double 1 - decay by at most 2^-25 relative, so after n updates the two
    differ by at most n 2^-24 max|p - e|."""
    try:
        from torch.optim import swa_utils as swa
    except ImportError:          # a torch without it: the same average, written by hand
        swa = None
    g = H._gen(22)
    lin = torch.nn.Linear(7, 5).to(F64)
    ps = [torch.randn(5, 7, generator=g, dtype=F64) for _ in range(6)]

    def averaged(**kw):
        if swa is None:
            e = ps[0].clone()
            for p in ps[1:]:
                e = kw["avg_fn"](e, p, 0)
            return e
        avg = swa.AveragedModel(lin, **kw)
        for p in ps:
            with torch.no_grad():
                lin.weight.copy_(p)
            avg.update_parameters(lin)
        return avg.module.weight.detach()

    e, _, n, _ = R.run(ps[0], ps[1:], 0.9, 1, warmup=False)
    assert n == 5
    if swa is not None and hasattr(swa, "get_ema_multi_avg_fn"):
        got = averaged(multi_avg_fn=swa.get_ema_multi_avg_fn(0.9))
    else:
        got = averaged(avg_fn=lambda e_, p_, n_: e_.lerp(p_, 1 - 0.9))
    spread = max(float((p - ps[0]).abs().max()) for p in ps) * 2
    torch.testing.assert_close(got, e, rtol=0, atol=n * 2.0 ** -24 * spread)
    # and the same w through a hand-written avg_fn: the same float64 expression, the same bits
    w = R.weight(0.9, 0, False)
    assert torch.equal(averaged(avg_fn=lambda e_, p_, n_: e_ + w * (p_ - e_)), e)


def test_swap_and_copy():
    e, p = torch.arange(4.0), -torch.arange(4.0)
    assert all(torch.equal(a, b) for a, b in zip(R.swap(e, p), (p, e)))
    assert all(torch.equal(a, b) for a, b in zip(R.copy(e, p), (p, p)))
