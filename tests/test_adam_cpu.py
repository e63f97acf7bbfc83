"""AdamW / LAMB without a GPU: the float64 reference of tests/adam_refs.py against torch.optim.AdamW,
optim.LAMB against the reference, the LAMB split of build_param_groups, and the MX_* refusals."""
import pytest
import torch

import adam_refs as R
import head_refs as H
from optim_refs import param_segments
from pytorch_distributed_amd.config import config_for
from pytorch_distributed_amd.optim import LAMB, build_param_groups

F64 = torch.float64
HYPER = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
         dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]


def _run(make_opt, dtype, hyper):
    """Three steps of ``make_opt(groups)`` over four tensors in two groups, and of the reference."""
    g = H._gen(5)
    ps, gs = ([torch.randn(s, generator=g) for s in [(5,), (4, 3), (2, 3, 3, 3), (1,)]] for _ in "pg")
    params = [torch.nn.Parameter(p.to(dtype, copy=True)) for p in ps]
    opt = make_opt([{"params": params[:2], **hyper[0]}, {"params": params[2:], **hyper[1]}])
    got = R.torch_steps(opt, params, [x.to(dtype) for x in gs], 3)
    flat = lambda ts: torch.cat([t.flatten() for t in ts])
    return got, R.adam_ref(flat(ps), flat(gs), param_segments(ps), [hyper[0]] * 2 + [hyper[1]] * 2, 3)


def test_reference_is_torch_adamw_in_float64():
    """float32 data in float64 tensors through torch.optim.AdamW; assert_close's float64 defaults."""
    got, ref = _run(lambda gr: torch.optim.AdamW(gr, foreach=False), F64, HYPER)
    for it, q in [(i, j) for i in range(3) for j in range(3)]:
        torch.testing.assert_close(ref[it][q].to(F64), got[it][q])


@pytest.mark.parametrize("lamb", [False, True])
def test_lamb_matches_the_reference(lamb):
    """A handful of f32 operations per element, each within 2^-24 relative: rtol 1e-6; elements
    near zero carry the rounding of steps of size lr ~1e-3: atol 1e-7."""
    got, ref = _run(LAMB, torch.float32, [{**h, "lamb": lamb} for h in HYPER])
    for it in range(3):
        torch.testing.assert_close(got[it][0], ref[it][0], rtol=1e-6, atol=1e-7)


def test_build_param_groups_lamb_split():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, bias=False), torch.nn.BatchNorm2d(4),
                              torch.nn.Flatten(), torch.nn.Linear(4, 2))
    g_m, g_v = build_param_groups(net, 1e-2, no_bn_decay=True, lamb=True)
    assert [p.dim() for p in g_m["params"]] == [4, 2] and [p.dim() for p in g_v["params"]] == [1, 1, 1]
    assert (g_m["lamb"], g_v["lamb"], g_m["weight_decay"], g_v["weight_decay"]) == (True, False, 1e-2, 0.0)
    assert build_param_groups(net, 1e-2, lamb=True)[1]["weight_decay"] == 1e-2
    assert "lamb" not in build_param_groups(net, 1e-2)[0]
    with pytest.raises(ValueError):
        build_param_groups(net, 1e-2, lars=0.01, lamb=True)


def test_config_reads_and_refuses():
    cfg = config_for("single", env={"MX_OPT": "lamb", "MX_BETAS": "0.8,0.99", "MX_OPT_EPS": "1e-6",
                                    "MX_WEIGHT_DECAY": "0.02", "MX_NO_BN_DECAY": "1",
                                    "MX_CLIP_GRAD_NORM": "1"})
    assert (cfg.opt, cfg.betas, cfg.opt_eps, cfg.weight_decay) == ("lamb", (0.8, 0.99), 1e-6, 0.02)
    d = config_for("single", env={})
    assert (d.opt, d.betas, d.opt_eps, d.weight_decay) == ("sgd", (0.9, 0.999), 1e-8, 1e-4)
    for env in ({"MX_OPT": "adam"}, {"MX_BETAS": "0.9,1.0"}, {"MX_BETAS": "-0.1,0.9"},
                {"MX_BETAS": "0.9"}, {"MX_OPT_EPS": "-1e-8"}, {"MX_OPT_EPS": "nan"},
                {"MX_WEIGHT_DECAY": "-1"}, {"MX_WEIGHT_DECAY": "inf"},
                {"MX_OPT": "adamw", "MX_NESTEROV": "1"}, {"MX_OPT": "lamb", "MX_LARS": "0.001"}):
        with pytest.raises(ValueError):
            config_for("single", env=env)
