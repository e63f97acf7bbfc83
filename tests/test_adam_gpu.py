"""AdamW / LAMB on the GPU: adam_tick, adamw_seg, lamb_moments and lamb_apply (csrc/adam.hip) against
the float64 reference of tests/adam_refs.py, their guard bands, the overflow skip and determinism,
the launchers' refusals, and NativeAdamW at the model level.

The bound. Errors are counted in float32 ulps of the reference value -- for p, of the larger of the
reference p before and after the step: a step that nearly cancels p leaves the rounding of its
larger operand, in every implementation. E is the largest such error, per quantity (p, m, v) over
every element and step, of the same steps in plain f32 torch on the CPU (torch.optim.AdamW(
foreach=False), optim.LAMB). Every element of the kernel's p, m and v lies within 2 E + 1 ulp: FMA
contraction and another operation order cost at most one more rounding per operation. Against an
E taken as the largest absolute error this is tighter for all but the largest elements and looser
for those: E is earned near zero (8 to 10 ulp for p, profiles/adam.md) and granted to all.
"""
import copy
import functools

import pytest
import torch

import adam_refs as R
import head_refs as H
from pytorch_distributed_amd.config import config_for
from pytorch_distributed_amd.models import build_model
from pytorch_distributed_amd.ops import native_ops as K
from pytorch_distributed_amd.optim import LAMB, build_param_groups
from pytorch_distributed_amd.runtime.graphs import GraphedNativeStep
from pytorch_distributed_amd.trainer import Context, build_optimizer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
SHADOWS = {"none": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def _groups(mode):
    """A, B: different betas, B without weight decay; C never has LAMB on ('lamb' mixes both kinds)."""
    on = mode == "lamb"
    return {"A": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, lamb=on),
            "B": dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, lamb=on),
            "C": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, lamb=False)}


@functools.lru_cache(maxsize=None)
def _inputs(mode):
    """Segments in one flat buffer, gaps of at least 4 elements (NaN in p) around each; 'frozen' lies
    in the buffer and in no table. Returns (p, g, live segments, their hyper, inside, {kind: segment})."""
    S = K.SEG_CHUNK
    spec = [(1, "A", ""), (2, "B", ""), (3, "C", ""), (4, "A", ""), (5, "B", ""), (7, "C", ""),
            (10, None, "frozen"), (S - 1, "B", ""), (S, "A", ""), (S + 1, "C", ""),
            (6, "B", "zero_g"), (9, "A", "zero_w"), (8, "A", "tiny_g"), (3 * S + 5, "A", "")]
    gen = H._gen(21)
    off, rows = 4, []
    for size, grp, kind in spec:
        rows.append((off, size, grp, kind))
        off = (off + size + 3) // 4 * 4 + 4
    p, g = torch.full((off,), float("nan")), torch.full((off,), 12345.0)
    inside = torch.zeros(off, dtype=torch.bool)
    for o, size, grp, kind in rows:
        p[o:o + size] = 0.0 if kind == "zero_w" else torch.randn(size, generator=gen)
        g[o:o + size] = torch.randn(size, generator=gen) * {"zero_g": 0.0, "tiny_g": 1e-20}.get(kind, 1.0)
        inside[o:o + size] = grp is not None
    live = [(o, s) for o, s, grp, _ in rows if grp]
    hyper = [_groups(mode)[grp] for _, _, grp, _ in rows if grp]
    return p, g, live, hyper, inside, {kind: (o, s) for o, s, _, kind in rows if kind}


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _run(mode, shadow, inv, repeat=0):
    """CPU copies of (p, m, v, shadow, bias, step, g): at the start, after three steps, a launch with
    found_inf = 1 and a fourth step. Gaps and the frozen range hold NaN in p, m, v and the shadow."""
    p0, g0, live, hyper, inside, kinds = _inputs(mode)
    nan = torch.full_like(p0, float("nan"))
    p, g, m = p0.to(DEV), g0.to(DEV), torch.where(inside, torch.zeros_like(p0), nan).to(DEV)
    v = m.clone()
    sh = nan.to(DEV, SHADOWS[shadow]) if SHADOWS[shadow] else None
    t = K.adam_tables(live, hyper, DEV)
    inv = torch.tensor([inv], device=DEV) if inv is not None else None
    snap = lambda: tuple(None if x is None else x.cpu() for x in (p, m, v, sh, t.bias, t.step, g))
    snaps = [snap()]
    for skip in (0.0, 0.0, 0.0, 1.0, 0.0):
        found = torch.full((1,), skip, device=DEV)
        K.adam_tick(t, found)
        if mode == "lamb":
            K.lamb_moments(p, g, m, v, t, inv_scale=inv, found_inf=found)
            K.lamb_apply(p, m, v, sh, t, found_inf=found)
        else:
            K.adamw_seg(p, g, m, v, sh, t, inv_scale=inv, found_inf=found)
        torch.cuda.synchronize()
        snaps.append(snap())
    return snaps


def _cpu_steps(mode, p0, g, live, hyper, steps):
    """The yardstick: plain f32 torch on the CPU, one parameter (and group) per segment."""
    params = [torch.nn.Parameter(p0[o:o + s].clone()) for o, s in live]
    groups = [{"params": [q], **h} for q, h in zip(params, hyper)]
    opt = LAMB(groups) if mode == "lamb" else torch.optim.AdamW(groups, foreach=False)
    return R.torch_steps(opt, params, [g[o:o + s] for o, s in live], steps)


def _assert_within(got, ref, cpu, live, p0):
    """The module's bound. got / ref: flat (p, m, v) per step; cpu: the segments' elements, joined."""
    idx = torch.cat([torch.arange(o, o + s) for o, s in live])
    for q, name in enumerate(("p", "m", "v")):
        E = worst = 0.0
        for it, r in enumerate(ref):
            a = r[q][idx].abs()
            if q == 0:
                a = torch.maximum(a, (ref[it - 1][0] if it else p0)[idx].abs())
            ulp = (torch.nextafter(a, a + 1) - a).to(F64)
            E = max(E, float(((cpu[it][q] - r[q][idx]).to(F64).abs() / ulp).max()))
            worst = max(worst, float(((got[it][q][idx] - r[q][idx]).to(F64).abs() / ulp).max()))
        assert worst <= 2 * E + 1, f"{name}: the kernel is {worst:.2f} ulp off, the CPU run E = {E:.2f}"


@functools.lru_cache(maxsize=None)
def _refs(mode, inv):
    p0, g0, live, hyper, inside, kinds = _inputs(mode)
    p0, s = torch.nan_to_num(p0), inv or 1.0      # (inv = 0.25: g0 * s is exact in f32)
    return R.adam_ref(p0, g0, live, hyper, 4, s), _cpu_steps(mode, p0, g0 * s, live, hyper, 4)


CASES = [(m, s, i) for m in ("adamw", "lamb") for s in SHADOWS for i in (None, 0.25)]


@pytest.mark.parametrize("mode,shadow,inv", CASES, ids=[f"{m}-{s}-{i}" for m, s, i in CASES])
def test_kernels_match_float64_reference(mode, shadow, inv):
    """Sizes 1..7, SEG_CHUNK - 1 / SEG_CHUNK / SEG_CHUNK + 1 and 3 * SEG_CHUNK + 5; a zero gradient
    without weight decay (u = 0: r = 1, p stays), zero weights (r = 1, p moves), gradients ~1e-20
    (eps rules the denominator). Steps 1-3, and step 4 after the skipped launch (t = 4). Outside the
    segments p, m, v and the shadow keep every bit, the gradient is never written, and the found_inf
    launch changes nothing, the bias table and the step counter included."""
    p0, g0, live, hyper, inside, kinds = _inputs(mode)
    snaps = _run(mode, shadow, inv)
    _assert_within([snaps[i][:3] for i in (1, 2, 3, 5)], *_refs(mode, inv), live, torch.nan_to_num(p0))
    assert [int(snaps[i][5]) for i in range(6)] == [0, 1, 2, 3, 3, 4]
    (o, s), (ow, sw) = kinds["zero_g"], kinds["zero_w"]
    assert torch.equal(snaps[3][0][o:o + s], snaps[0][0][o:o + s])
    assert bool((snaps[1][0][ow:ow + sw] != 0).all()) and int((~inside).sum()) >= 4 * 14 + 10
    for it in range(1, 6):
        assert torch.equal(_bits(snaps[it][6]), _bits(snaps[0][6])), f"gradient written, launch {it}"
        for name, a, b in zip(("p", "m", "v", "shadow"), snaps[it], snaps[0]):
            if a is not None:
                bad = ((_bits(a) != _bits(b)) & ~inside).nonzero().flatten()[:8].tolist()
                assert not bad, f"{name} written outside the segments at {bad} (launch {it})"
        if shadow != "none":      # the shadow is torch's cast of the kernel's own stored p
            assert bool(H.cast_matches(snaps[it][3][inside], snaps[it][0][inside]).all())
    for a, b in zip(snaps[4][:6], snaps[3][:6]):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), "found_inf = 1 must leave everything unchanged"
    assert not torch.equal(_bits(snaps[3][0]), _bits(snaps[2][0]))     # (the clean steps do move p)
    if shadow == "bf16" and inv is None:      # a second run from the same inputs: bit-equal
        for a, b in zip(snaps[1:], _run(mode, shadow, inv, repeat=1)[1:]):
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[:5], b[:5]))


def test_refusals_launch_nothing():
    """b1 = 1, a negative lr, a NaN eps, a LAMB segment with no slab: ValueError, nothing launched."""
    (p, g), (m, v) = torch.randn(2, 64, device=DEV), torch.zeros(2, 64, device=DEV)
    before = [x.clone() for x in (p, m, v)]
    good = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for bad in (dict(betas=(1.0, 0.999)), dict(lr=-1e-3), dict(eps=float("nan")), dict(lamb=True)):
        t = K.adam_tables([(0, 40)], [{**good, **bad}], DEV)
        t.slab = None
        launches = [lambda: K.adamw_seg(p, g, m, v, None, t), lambda: K.lamb_moments(p, g, m, v, t),
                    lambda: K.lamb_apply(p, m, v, None, t)]
        for launch in launches + ([] if "lamb" in bad else [lambda: K.adam_tick(t)]):
            with pytest.raises(ValueError, match="LAMB on" if "lamb" in bad else None):
                launch()
        assert int(t.step) == 0
    for a, b in zip(before, (p, m, v)):
        assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ model level
def _native(dtype=torch.bfloat16, image=32):
    from pytorch_distributed_amd.models.native import NativeResNet
    torch.manual_seed(0)
    return NativeResNet(build_model("resnet18"), device=DEV, dtype=dtype, image_size=image)


def _batch(nm, image=32, B=8):
    from pytorch_distributed_amd.data import SyntheticImageNet
    return nm.input_generator(SyntheticImageNet("train", image_size=image))(torch.arange(B))


def _make(nm, mode, **kw):
    groups = build_param_groups(nm, 1e-2, no_bn_decay=True, lamb=mode == "lamb")
    return nm.make_optimizer(opt=mode, lr=1e-3, weight_decay=1e-2, param_groups=groups, **kw)


@pytest.mark.parametrize("mode", ["adamw", "lamb"])
def test_model_steps_state_round_trip_and_graph_refusal(mode):
    """ResNet-18 (32 px, batch 8, bf16), no-BN-decay groups: two steps against the CPU optimizer under
    the module's bound; state_dict() through torch.optim.AdamW into a fresh NativeAdamW: bit-equal."""
    nm = _native()
    opt = _make(nm, mode)
    x, y = _batch(nm)
    nm.make_criterion()(nm(x), y).backward()
    torch.cuda.synchronize()
    base, p0, g0 = nm.flat_params.data_ptr(), nm.flat_params.cpu(), nm.flat_grad.cpu()
    live = [((q.data_ptr() - base) // 4, q.numel()) for gr in opt.param_groups for q in gr["params"]]
    hyper = [{k: gr[k] for k in _groups(mode)["A"]} for gr in opt.param_groups for _ in gr["params"]]

    def step(o):
        nm._grads_zero = False          # the same flat gradient again (zero_grad was not called)
        o.step()
        torch.cuda.synchronize()
        return [t.clone() for t in (nm.flat_params, o.exp_avg, o.exp_avg_sq, nm.flat_shadow)]

    got = [[t.cpu() for t in step(opt)[:3]] for _ in range(2)]
    _assert_within(got, R.adam_ref(p0, g0, live, hyper, 2), _cpu_steps(mode, p0, g0, live, hyper, 2), live, p0)
    inside = torch.zeros(nm.numel, dtype=torch.bool)
    inside[torch.cat([torch.arange(o, o + s) for o, s in live])] = True
    assert bool(H.cast_matches(nm.flat_shadow.cpu()[inside], got[1][0][inside]).all())
    assert torch.equal(_bits(got[1][0])[~inside], _bits(p0)[~inside])
    sd = copy.deepcopy(opt.state_dict())      # (torch's load keeps the tensors)
    assert {float(s["step"]) for s in sd["state"].values()} == {2.0} and len(sd["state"]) == 62
    topt = torch.optim.AdamW([{**gr, "params": list(gr["params"])} for gr in opt.param_groups])
    topt.load_state_dict(sd)
    p2, s2 = nm.flat_params.clone(), nm.flat_shadow.clone()
    want = step(opt)
    with torch.no_grad():
        nm.flat_params.copy_(p2), nm.flat_shadow.copy_(s2)
    fresh = _make(nm, mode)
    fresh.load_state_dict(topt.state_dict())
    assert int(fresh._tables.step) == 2 and [gr["lamb"] for gr in fresh.param_groups] == [mode == "lamb", False]
    for w, g in zip(want, step(fresh)):
        assert torch.equal(_bits(w), _bits(g))
    # MX_OPT with MX_GRAPH=1: the segmented optimizer's refusal, before training starts
    cfg = config_for("single", env={"MX_OPT": mode, "MX_GRAPH": "1", "MX_LR": "0.001"})
    with pytest.raises(ValueError, match="MX_GRAPH=1 cannot run the segmented optimizer"):
        build_optimizer(cfg, nm, Context(cfg, DEV, torch.bfloat16, "native"))
    built = build_optimizer(cfg.replace(graph=False), nm, Context(cfg, DEV, torch.bfloat16, "native"))
    assert type(built).__name__ == "NativeAdamW" and built.param_groups[0]["lr"] == 0.001
    with pytest.raises(ValueError, match="MX_GRAPH"):
        GraphedNativeStep(nm, built, None, 8)


def test_amp_overflow_skips_the_step_and_its_count():
    """fp16 + clipping: a clean step_amp moves the weights; an injected inf changes nothing. No sync."""
    from pytorch_distributed_amd.amp import LossScaler
    nm = _native(torch.float16)
    opt = _make(nm, "lamb", clip_grad_norm=1.0)
    crit, (x, y) = nm.make_criterion(), _batch(nm)
    scaler = LossScaler(init_scale=1024.0, growth_interval=1000)
    for poison in (False, True):
        before = [t.clone() for t in (nm.flat_params, opt.exp_avg, opt.exp_avg_sq, nm.flat_shadow)]
        scaler.scale(crit(nm(x), y)).backward()
        if poison:
            nm.flat_grad[nm.fc_b_off + 1] = float("inf")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt), scaler.update(), opt.zero_grad()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        same = [torch.equal(_bits(a), _bits(b)) for a, b in
                zip(before, (nm.flat_params, opt.exp_avg, opt.exp_avg_sq, nm.flat_shadow))]
        assert same == [poison] * 4 and scaler.found_inf.item() == float(poison)
        assert {float(s["step"]) for s in opt.state_dict()["state"].values()} == {1.0}
    assert scaler.get_scale() == 512.0 and float(opt.grad_norm) > 0
