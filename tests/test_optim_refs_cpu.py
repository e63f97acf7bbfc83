"""The float64 reference of the segmented optimizer (tests/optim_refs.py) against torch.optim.SGD, and
the pure-torch LARS optimizer against that reference."""
import pytest
import torch

import optim_refs as R

SHAPES = [(7,), (3, 5), (4, 2, 3, 3), (1,), (130,)]


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return ([torch.randn(s, generator=g) for s in SHAPES], [torch.randn(s, generator=g) for s in SHAPES])


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _run_torch(opt_fn, ps, gs, groups_of, steps=3):
    """Three steps of a torch optimizer over clones of ``ps`` with the fixed gradients ``gs``;
    ``groups_of``: [(indices, group settings)]. Returns flat p after each step and the optimizer."""
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    groups = [{"params": [params[i] for i in idx], **h} for idx, h in groups_of]
    opt = opt_fn(groups)
    out = []
    for _ in range(steps):
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.step()
        out.append(_flat([p.detach() for p in params]))
    return out, opt, params


def _hyper(groups_of, n, **defaults):
    hy = [None] * n
    for idx, h in groups_of:
        for i in idx:
            hy[i] = {**defaults, **h}
    return hy


CASES = {
    "plain": dict(momentum=0.9, weight_decay=1e-4, nesterov=False),
    "nesterov": dict(momentum=0.9, weight_decay=1e-4, nesterov=True),
    "no_momentum": dict(momentum=0.0, weight_decay=1e-4, nesterov=False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_matches_torch_sgd(case):
    """Plain, Nesterov and momentum-free SGD, each with a second group of its own weight decay and
    learning rate: three steps, rtol = atol = 1e-6 for p and for the momentum buffers."""
    ps, gs = _tensors(1)
    d = CASES[case]
    groups_of = [([0, 2, 4], {}), ([1, 3], {"weight_decay": 0.0, "lr": 0.03})]
    got, opt, params = _run_torch(lambda g: torch.optim.SGD(g, lr=0.1, **d), ps, gs, groups_of)
    segs = R.param_segments(ps)
    ref = R.seg_sgd_ref(_flat(ps), _flat(gs), segs, _hyper(groups_of, len(ps), lr=0.1, **d), 3)
    for it in range(3):
        torch.testing.assert_close(got[it].to(R.F64), ref[it][0].to(R.F64), rtol=1e-6, atol=1e-6)
    if d["momentum"]:
        bufs = _flat([opt.state[p]["momentum_buffer"] for p in params])
        torch.testing.assert_close(bufs.to(R.F64), ref[2][1].to(R.F64), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("nesterov", [False, True], ids=["heavy_ball", "nesterov"])
def test_lars_matches_reference(nesterov):
    """optim.LARS against the reference: a trust group with weight decay, one without, and a group
    without a trust ratio; one tensor with an all-zero gradient and one with all-zero weights, where
    the ratio is 1. Three steps, rtol = atol = 1e-6 (LARS takes its norms in float64 and rounds the
    ratio to float32 once, like the reference)."""
    from pytorch_distributed_amd.optim import LARS
    ps, gs = _tensors(2)
    gs[2] = torch.zeros_like(gs[2])      # |g| = 0
    ps[1] = torch.zeros_like(ps[1])      # |w| = 0
    groups_of = [([0, 2], {"lars": 0.02}),
                 ([1, 4], {"lars": 0.05, "weight_decay": 0.0, "lr": 0.5}),
                 ([3], {"weight_decay": 0.0})]
    d = dict(momentum=0.9, weight_decay=1e-2, nesterov=nesterov)
    got, opt, params = _run_torch(lambda g: LARS(g, lr=0.1, **d), ps, gs, groups_of)
    hy = _hyper(groups_of, len(ps), lr=0.1, **d)
    segs = R.param_segments(ps)
    assert R.trust_ratio(ps[2].to(R.F64), gs[2].to(R.F64), hy[2]) == 1.0
    assert R.trust_ratio(ps[1].to(R.F64), gs[1].to(R.F64), hy[1]) == 1.0
    assert R.trust_ratio(ps[0].to(R.F64), gs[0].to(R.F64), hy[0]) != 1.0
    ref = R.seg_sgd_ref(_flat(ps), _flat(gs), segs, hy, 3)
    for it in range(3):
        torch.testing.assert_close(got[it].to(R.F64), ref[it][0].to(R.F64), rtol=1e-6, atol=1e-6)
    bufs = _flat([opt.state[p]["momentum_buffer"] for p in params])
    torch.testing.assert_close(bufs.to(R.F64), ref[2][1].to(R.F64), rtol=1e-6, atol=1e-6)


def test_lars_without_trust_is_torch_sgd_bit_for_bit():
    """lars = 0: the same float32 operations as torch.optim.SGD, Nesterov included."""
    from pytorch_distributed_amd.optim import LARS
    ps, gs = _tensors(3)
    groups_of = [([0, 1, 2], {}), ([3, 4], {"weight_decay": 0.0})]
    for nesterov in (False, True):
        d = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=nesterov)
        a, _, _ = _run_torch(lambda g: torch.optim.SGD(g, **d), ps, gs, groups_of)
        b, _, _ = _run_torch(lambda g: LARS(g, **d), ps, gs, groups_of)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
