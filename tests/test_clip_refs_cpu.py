"""tests/clip_refs.py against torch on the CPU: ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.SGD`` / ``pytorch_distributed_amd.optim.LARS`` on float64 tensors.

Bounds. The norm: torch takes the norm of the per-tensor norms, the reference one sum of squares --
a handful of float64 roundings apart (rtol 1e-14). The coefficient: bit-equal to the float32
formula evaluated with torch's own float32 ops. The clipped step: torch, on float64 tensors,
evaluates the coefficient in float64, the reference (as the kernel) in float32 from the
float32-rounded norm -- three float32 roundings, 3 * 2^-24 < 2e-7 relative on the gradient term,
so the weights agree to rtol 1e-6 of values of order 1 (atol 1e-7 for those near 0).
"""
import math

import numpy as np
import pytest
import torch

import clip_refs as CR
import optim_refs as R

F64 = torch.float64
SIZES = (1, 3, 4, 5, 17, 129, 1001)


def _tensors(seed=5, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g, dtype=F64) for n in SIZES]
    gs = [torch.randn(n, generator=g, dtype=F64) * scale for n in SIZES]
    return ps, gs


def _torch_coef32(norm, max_norm):
    n = torch.tensor(float(norm), dtype=torch.float32)
    c = torch.clamp(torch.tensor(float(max_norm), dtype=torch.float32) / (n + 1e-6), max=1.0)
    assert c.dtype == torch.float32
    return c


def _bits32(v):
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


def test_norm_matches_torch_float64():
    ps, gs = _tensors()
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    for p, g in zip(params, gs):
        p.grad = g.clone()
    total = float(torch.nn.utils.clip_grad_norm_(params, 1e9))
    flat, segs = torch.cat(gs), R.param_segments(gs)
    assert CR.norm64(flat, segs) == pytest.approx(total, rel=1e-14, abs=0)
    # a range left out does not count
    assert CR.norm64(flat, segs[1:]) == pytest.approx(
        float(torch.cat(gs[1:]).pow(2).sum().sqrt()), rel=1e-14, abs=0)
    assert float(CR.norm32(flat, segs, 0.5)) == float(np.float32(0.5 * CR.norm64(flat, segs)))


@pytest.mark.parametrize("case", ["below", "at", "above", "far_above", "nan", "inf", "zero"])
def test_coefficient_is_the_float32_formula_bit_for_bit(case):
    max_norm = 2.5
    norm = {"below": 1.75, "at": 2.5, "above": 2.5000002, "far_above": 1234.5678, "nan": math.nan,
            "inf": math.inf, "zero": 0.0}[case]
    c = CR.coef32(norm, max_norm)
    assert isinstance(c, np.float32)
    want = _torch_coef32(norm, max_norm)
    assert _bits32(c) == _bits32(want.item()) or (math.isnan(c) and bool(want.isnan()))
    if case in ("below", "zero"):
        assert float(c) == 1.0
    if case in ("above", "far_above"):
        assert 0.0 < float(c) < 1.0
    if case == "nan":
        assert math.isnan(float(c))          # torch's clamp propagates NaN; fminf would give 1
    if case == "inf":
        assert float(c) == 0.0


def test_scale_of_non_finite_gradients_and_skipped_steps():
    g = torch.ones(8)
    segs = [(0, 8)]
    g[3] = math.inf
    assert float(CR.norm32(g, segs)) == math.inf and float(CR.scale32(g, segs, 1.0, 0.5)) == 0.0
    g[3] = math.nan
    assert math.isnan(float(CR.norm32(g, segs))) and math.isnan(float(CR.scale32(g, segs, 1.0)))
    assert float(CR.scale32(g, segs, 1.0, 0.25, found_inf=True)) == 0.25


HYPERS = {
    "sgd": dict(lr=0.1, momentum=0.9, weight_decay=1e-4),
    "nesterov": dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True),
    "lars": dict(lr=0.1, momentum=0.9, weight_decay=1e-4, lars=0.02),
}


@pytest.mark.parametrize("name", list(HYPERS))
@pytest.mark.parametrize("max_norm", [0.5, 1e6], ids=["clipping", "not_clipping"])
def test_clipped_step_matches_torch(name, max_norm):
    """Three steps on the same gradient: clip_grad_norm_ then the torch optimizer, float64."""
    from pytorch_distributed_amd.optim import LARS
    h = HYPERS[name]
    ps, gs = _tensors(seed=6)
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = LARS(params, **h) if "lars" in h else torch.optim.SGD(params, **h)
    flat_p, flat_g, segs = torch.cat(ps), torch.cat(gs), R.param_segments(ps)
    if max_norm < 1:
        assert CR.norm64(flat_g, segs) > 10 * max_norm
    # the reference takes and returns float32 roundings; feed it float32-exact inputs
    flat_p32, flat_g32 = flat_p.to(torch.float32), flat_g.to(torch.float32)
    with torch.no_grad():
        for p, (off, n) in zip(params, segs):
            p.copy_(flat_p32[off:off + n])
    ref = CR.clipped_sgd_ref(flat_p32, flat_g32, segs, [h] * len(segs), 3, max_norm)
    for it in range(3):
        for p, (off, n) in zip(params, segs):
            p.grad = flat_g32[off:off + n].to(F64).clone()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        got = torch.cat([p.detach() for p in params])
        torch.testing.assert_close(ref[it][0].to(F64), got, rtol=1e-6, atol=1e-7)
    assert not torch.equal(got, flat_p32.to(F64))
