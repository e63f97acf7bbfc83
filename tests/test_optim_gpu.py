"""The segmented optimizer on the GPU: seg_norms / sgd_seg (csrc/optim.hip) against the float64
reference of tests/optim_refs.py, their guard bands and determinism, the table refusals, and
NativeSGD with parameter groups, Nesterov momentum and LARS at the model level.

Bounds: p and buf within rtol = atol = 1e-6 of the float64 reference, the bound sgd_flat is held to
(tests/test_head_kernels_gpu.py); the trust ratio, from double sums, is off by at most one float32
rounding. The 16-bit shadow bit-equals torch's cast of the stored p. Everything outside the
segments is compared bit for bit.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import head_refs as H
import optim_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
SHADOWS = {"none": None, "bf16": torch.bfloat16, "fp16": torch.float16}


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


# ------------------------------------------------------------------ the kernel-level layout
GROUPS = {
    "A": dict(lr=0.1, momentum=0.0, weight_decay=1e-4),                                # no momentum
    "B": dict(lr=0.05, momentum=0.9, weight_decay=0.0, nesterov=True),                 # no wd, Nesterov
    "C": dict(lr=0.1, momentum=0.9, weight_decay=1e-4, lars=0.02),                     # trust, wd
    "D": dict(lr=0.2, momentum=0.9, weight_decay=0.0, lars=0.05, nesterov=True, lars_eps=1e-6),
}


@functools.lru_cache(maxsize=None)
def _layout():
    """Segments (size, group, kind) laid into one flat buffer with gaps of at least 4 elements
    between them, in front of the first and behind the last; 'frozen' lies in the buffer and in no
    table. Returns (n, [(off, size, group, kind)])."""
    S = _k().SEG_CHUNK
    spec = [(1, "C", ""), (2, "D", ""), (3, "A", ""), (4, "B", ""), (5, "C", ""), (7, "D", ""),
            (10, None, "frozen"), (S - 1, "B", ""), (S, "A", ""), (S + 1, "D", ""),
            (6, "C", "zero_g"), (9, "D", "zero_w"), (3 * S + 5, "C", ""), (2 * S + 3, "B", "")]
    off, segs = 4, []
    for size, grp, kind in spec:
        segs.append((off, size, grp, kind))
        off = (off + size + 3) // 4 * 4 + 4
    return off, segs


def _inputs():
    n, segs = _layout()
    g = H._gen(11)
    p = torch.full((n,), float("nan"))
    gr = torch.full((n,), 12345.0)
    for off, size, grp, kind in segs:
        p[off:off + size] = 0.0 if kind == "zero_w" else torch.randn(size, generator=g)
        gr[off:off + size] = 0.0 if kind == "zero_g" else torch.randn(size, generator=g)
    live = [(o, s) for o, s, grp, _ in segs if grp is not None]
    hyper = [dict(GROUPS[grp]) for _, _, grp, _ in segs if grp is not None]
    inside = torch.zeros(n, dtype=torch.bool)
    for o, s in live:
        inside[o:o + s] = True
    return n, p, gr, live, hyper, inside


def _canary(n, dtype):
    if dtype == torch.float32:
        return torch.full((n,), 0x7FC0BEEF, dtype=torch.int64).to(torch.int32).view(torch.float32)
    bits = 0x7FC5 if dtype == torch.bfloat16 else 0x7E05
    return torch.full((n,), bits, dtype=torch.int16).view(dtype)


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _run(shadow_name, inv, repeat=0):
    """Three steps of seg_norms + sgd_seg from the fixed inputs; CPU copies of (p, buf, shadow)
    after every step, then a fourth launch with found_inf = 1 (its copies last)."""
    K = _k()
    sdt = SHADOWS[shadow_name]
    n, p0, g0, live, hyper, inside = _inputs()
    # canaries: gaps (and the frozen segment's momentum and shadow) hold NaN patterns; the frozen
    # segment's p holds finite data; the segments' momentum starts as NaN too (a first step must
    # not read it) and their shadow as the canary
    p = torch.where(inside | ~p0.isnan(), p0, _canary(n, torch.float32)).to(DEV)
    gr = g0.to(DEV)
    buf = _canary(n, torch.float32).to(DEV)
    sh = _canary(n, sdt).to(DEV) if sdt is not None else None
    tables, nblk = K.seg_tables(live, hyper, DEV)
    assert nblk == sum(-(-s // K.SEG_CHUNK) for _, s in live)
    inv_d = torch.tensor([inv], device=DEV) if inv is not None else None
    zero = torch.zeros(1, device=DEV) if inv is not None else None
    snaps = [tuple(t.cpu() if t is not None else None for t in (p, buf, sh, gr))]
    for it in range(3):
        K.seg_norms(p, gr, tables)
        K.sgd_seg(p, gr, buf, sh, tables, initialized=it > 0, inv_scale=inv_d, found_inf=zero)
        torch.cuda.synchronize()
        snaps.append(tuple(t.cpu() if t is not None else None for t in (p, buf, sh, gr)))
    K.seg_norms(p, gr, tables)
    K.sgd_seg(p, gr, buf, sh, tables, initialized=True, inv_scale=inv_d,
              found_inf=torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    snaps.append(tuple(t.cpu() if t is not None else None for t in (p, buf, sh, gr)))
    return snaps


@functools.lru_cache(maxsize=None)
def _reference(inv):
    n, p0, g0, live, hyper, inside = _inputs()
    return R.seg_sgd_ref(torch.nan_to_num(p0), g0, live, hyper, 3, inv if inv is not None else 1.0)


CASES = [(s, i) for s in SHADOWS for i in (None, 0.25)]
IDS = [f"{s}-{'inv' if i else 'noinv'}" for s, i in CASES]


@pytest.mark.parametrize("shadow,inv", CASES, ids=IDS)
def test_kernel_matches_float64_reference(shadow, inv):
    """Sizes 1..7, SEG_CHUNK - 1 / SEG_CHUNK / SEG_CHUNK + 1, 3 * SEG_CHUNK + 5 and 2 * SEG_CHUNK + 3
    over four groups (momentum 0; weight decay 0 with Nesterov; trust with weight decay; trust
    without, with Nesterov), a trust segment with an all-zero gradient and one with all-zero
    weights: three steps, the first over a NaN momentum buffer."""
    n, p0, g0, live, hyper, inside = _inputs()
    snaps, ref = _run(shadow, inv), _reference(inv)
    for it in range(3):
        p, buf, sh, _ = snaps[it + 1]
        for off, size in live:
            sl = slice(off, off + size)
            tag = f"step {it}, segment at {off} of {size}"
            assert bool(p[sl].isfinite().all()) and bool(buf[sl].isfinite().all()), tag
            torch.testing.assert_close(p[sl].to(F64), ref[it][0][sl].to(F64), rtol=1e-6, atol=1e-6,
                                       msg=lambda m, tag=tag: f"p, {tag}: {m}")
            torch.testing.assert_close(buf[sl].to(F64), ref[it][1][sl].to(F64), rtol=1e-6, atol=1e-6,
                                       msg=lambda m, tag=tag: f"buf, {tag}: {m}")
            if sh is not None:      # the shadow is torch's cast of the kernel's own stored p
                assert bool(H.cast_matches(sh[sl], p[sl]).all()), tag
    # the degenerate trust segments took q = 1 and moved: zero gradient by its weight decay, zero
    # weights by their gradient (the reference agrees above; this pins that they are not skipped)
    kinds = {kind: (off, size) for off, size, _, kind in _layout()[1] if kind in ("zero_g", "zero_w")}
    assert len(kinds) == 2
    for off, size in kinds.values():
        assert not torch.equal(snaps[1][0][off:off + size], snaps[0][0][off:off + size])


@pytest.mark.parametrize("shadow,inv", CASES, ids=IDS)
def test_guard_bands_and_overflow_skip(shadow, inv):
    """Every element in no segment -- the gaps, and a frozen segment that lies in the buffer but in
    no table -- keeps its bits in p, buf and the shadow through all launches, the gradient keeps
    all of its bits, and a launch with found_inf = 1 changes nothing at all."""
    n, p0, g0, live, hyper, inside = _inputs()
    snaps = _run(shadow, inv)
    first = snaps[0]
    assert int((~inside).sum()) >= 4 * (len(live) + 2)
    for it in range(1, 5):
        p, buf, sh, gr = snaps[it]
        assert torch.equal(_bits(gr), _bits(first[3])), f"gradient written at launch {it}"
        for name, a, b in (("p", p, first[0]), ("buf", buf, first[1]), ("shadow", sh, first[2])):
            if a is None:
                continue
            bad = ((_bits(a) != _bits(b)) & ~inside).nonzero().flatten()[:8].tolist()
            assert not bad, f"{name} written outside the segments at {bad} (launch {it})"
    for a, b in zip(snaps[4][:3], snaps[3][:3]):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), "found_inf = 1 must leave everything unchanged"
    assert not torch.equal(_bits(snaps[3][0]), _bits(snaps[2][0]))     # (the clean steps do move p)


def test_three_steps_repeat_bit_for_bit():
    """The same three steps from the same inputs, LARS groups included: bit-equal p and buf."""
    a, b = _run("bf16", None), _run("bf16", None, repeat=1)
    assert a is not b
    for it in range(1, 4):
        for x, y in zip(a[it][:3], b[it][:3]):
            assert torch.equal(_bits(x), _bits(y)), f"step {it - 1} differs between two runs"


def test_table_refusals_launch_nothing():
    """An offset that is no multiple of 4, a segment past n, overlapping segments and a block table
    that skips a chunk: ValueError from both launchers, and p, buf and the shadow keep their bits."""
    K = _k()
    S = K.SEG_CHUNK
    n = 4 * S
    g = H._gen(12)
    p, gr = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    buf, sh = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=torch.bfloat16)
    before = [t.clone() for t in (p, buf, sh)]
    h = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, lars=0.01)
    good, _ = K.seg_tables([(0, 2 * S + 5)], [h], DEV)
    skipped = (K.BlkRow * 2)(good.blk_host[0], good.blk_host[2])
    bad = {"offset": K.seg_tables([(6, 8)], [h], DEV)[0],
           "past n": K.seg_tables([(n - 8, 12)], [h], DEV)[0],
           "overlap": K.seg_tables([(0, 16), (8, 16)], [h, h], DEV)[0],
           "skipped chunk": K.SegTables(good.seg_host, skipped, DEV)}
    for name, t in bad.items():
        with pytest.raises(ValueError):
            K.seg_norms(p, gr, t)
        t.slab = torch.zeros(64, dtype=torch.float64, device=DEV)
        with pytest.raises(ValueError):
            K.sgd_seg(p, gr, buf, sh, t, initialized=False)
        torch.cuda.synchronize()
        for a, b in zip(before, (p, buf, sh)):
            assert torch.equal(_bits(a), _bits(b)), name
    with pytest.raises(ValueError):          # buffers of another length than p
        K.sgd_seg(p, gr[:-4], buf, sh, good, initialized=False)
    with pytest.raises(ValueError):          # a trust coefficient and no norms
        K.sgd_seg(p, gr, buf, sh, K.seg_tables([(0, 8)], [h], DEV)[0], initialized=False)
    K.seg_norms(p, gr, good)                 # (the good table does launch)
    K.sgd_seg(p, gr, buf, sh, good, initialized=False)
    torch.cuda.synchronize()
    assert not torch.equal(p[:2 * S + 5], before[0][:2 * S + 5])
    assert torch.equal(_bits(p[2 * S + 5:]), _bits(before[0][2 * S + 5:]))


# ------------------------------------------------------------------ model level
def _native(dtype=torch.bfloat16, image=32):
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.models.native import NativeResNet
    torch.manual_seed(0)
    return NativeResNet(build_model("resnet18"), device=DEV, dtype=dtype, image_size=image)


def _batch(nm, image=32, B=8):
    from pytorch_distributed_amd.data import SyntheticImageNet
    return nm.input_generator(SyntheticImageNet("train", image_size=image))(torch.arange(B))


def _segments_of(nm, opt):
    base = nm.flat_params.data_ptr()
    segs, hyper = [], []
    for g in opt.param_groups:
        for p in g["params"]:
            segs.append(((p.data_ptr() - base) // 4, p.numel()))
            hyper.append({k: g[k] for k in ("lr", "momentum", "weight_decay", "nesterov", "lars",
                                            "lars_eps")})
    return segs, hyper


def test_model_groups_nesterov_lars_and_frozen_layer():
    """Native ResNet-18 (32 px, batch 8, bf16): one forward / backward, then three optimizer steps
    on that flat gradient with no_bn_decay + Nesterov + lars = 0.001 groups and layer1 left out of
    every group. Against the float64 reference at rtol = atol = 1e-6; layer1 (and every padding
    element) keeps its bits in the master weights, the momentum and the shadow."""
    from pytorch_distributed_amd.models.native import NativeSGD
    from pytorch_distributed_amd.optim import build_param_groups
    nm = _native()
    assert NativeSGD(nm).segmented is False
    frozen = {id(p) for p in nm.layer1.parameters()}
    assert len(frozen) == 12
    groups = build_param_groups(nm, 1e-4, no_bn_decay=True, lars=0.001)
    assert [len(g["params"]) for g in groups] == [21, 41]
    for g in groups:
        g["params"] = [p for p in g["params"] if id(p) not in frozen]
    opt = nm.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True, param_groups=groups)
    assert opt.segmented is True and sum(len(g["params"]) for g in opt.param_groups) == 62 - 12
    with pytest.raises(ValueError):
        opt.add_param_group({"params": list(nm.layer1.parameters())})
    x, y = _batch(nm)
    nm.make_criterion()(nm(x), y).backward()
    torch.cuda.synchronize()
    segs, hyper = _segments_of(nm, opt)
    assert (nm.fc_w_off, nm.num_classes * nm.feat_dim) in segs         # not the padded rows
    p0, g0, s0 = nm.flat_params.cpu(), nm.flat_grad.cpu(), nm.flat_shadow.cpu()
    assert bool(g0.isfinite().all()) and float(g0.abs().max()) > 0
    ref = R.seg_sgd_ref(p0, g0, segs, hyper, 3)
    inside = torch.zeros(nm.numel, dtype=torch.bool)
    for o, s in segs:
        inside[o:o + s] = True
    assert int((~inside).sum()) >= sum(p.numel() for p in nm.layer1.parameters())
    for it in range(3):
        nm._grads_zero = False          # the same flat gradient again (zero_grad was not called)
        opt.step()
        torch.cuda.synchronize()
        p, buf, sh = nm.flat_params.cpu(), opt.flat_mom.cpu(), nm.flat_shadow.cpu()
        torch.testing.assert_close(p[inside].to(F64), ref[it][0][inside].to(F64), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(buf[inside].to(F64), ref[it][1][inside].to(F64), rtol=1e-6,
                                   atol=1e-6)
        assert bool(H.cast_matches(sh[inside], p[inside]).all())
        assert torch.equal(_bits(p)[~inside], _bits(p0)[~inside])
        assert torch.equal(_bits(sh)[~inside], _bits(s0)[~inside])
        assert int(torch.count_nonzero(buf[~inside])) == 0
    assert not torch.equal(p[inside], p0[inside])
    # StepLR edits group["lr"]: the next step uploads the table again and uses it
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [0.05, 0.05]
    nm._grads_zero = False
    opt.step()
    torch.cuda.synchronize()
    hyper2 = [{**h, "lr": 0.05} for h in hyper]
    # one more reference step from the reference's own state, at the new rate
    ref4 = _continue_ref(ref[2], g0, segs, hyper2)
    torch.testing.assert_close(nm.flat_params.cpu()[inside].to(F64), ref4[inside].to(F64), rtol=1e-6,
                               atol=1e-6)


def _continue_ref(last, g, segs, hyper):
    """One more float64 step from a reference state (p32, buf32, _) that is already initialised."""
    p64, buf = last[0].to(F64).clone(), last[1].to(F64).clone()
    g64 = g.to(F64)
    for (off, n), h in zip(segs, hyper):
        sl = slice(off, off + n)
        q = R.trust_ratio(p64[sl], g64[sl], h)
        d = q * (g64[sl] + h["weight_decay"] * p64[sl])
        b = h["momentum"] * buf[sl] + d
        step = d + h["momentum"] * b if h["nesterov"] else b
        p64[sl] = p64[sl] - h["lr"] * step
    return p64.to(torch.float32)


def test_state_dict_round_trip_with_torch_sgd():
    """Three groups: the native state loads into a torch.optim.SGD with the same grouping over
    clones of the parameters (custom keys ride along), and torch's state loads back; the momentum
    buffers are equal both ways."""
    nm = _native()
    ps = list(nm.parameters())
    mk = lambda q: [{"params": q[:20], "lr": 0.05}, {"params": q[20:40], "weight_decay": 0.0},
                    {"params": q[40:], "lars": 0.001, "lars_eps": 1e-7}]
    opt = nm.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True, param_groups=mk(ps))
    x, y = _batch(nm)
    nm.make_criterion()(nm(x), y).backward()
    opt.step()
    torch.cuda.synchronize()
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 3 and len(sd["state"]) == 62
    assert sd["param_groups"][2]["lars"] == 0.001 and sd["param_groups"][2]["lars_eps"] == 1e-7
    assert [g["params"] for g in sd["param_groups"]] == [list(range(20)), list(range(20, 40)),
                                                         list(range(40, 62))]
    clones = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    topt = torch.optim.SGD(mk(clones), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == 0.05 and topt.param_groups[2]["lars"] == 0.001
    for p, c in zip(ps, clones):
        assert torch.equal(topt.state[c]["momentum_buffer"], opt.state[p]["momentum_buffer"])
    # torch -> native: different buffers, hyper-parameters from the checkpoint
    for c in clones:
        topt.state[c]["momentum_buffer"].mul_(3.0).add_(1.0)
    topt.param_groups[1]["lr"] = 0.025
    nm2 = _native()
    ps2 = list(nm2.parameters())
    opt2 = nm2.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True,
                              param_groups=mk(ps2))
    opt2.load_state_dict(topt.state_dict())
    assert opt2._initialized and opt2.param_groups[1]["lr"] == 0.025
    assert opt2.param_groups[2]["lars"] == 0.001 and opt2.param_groups[0]["lars"] == 0.0
    for p, c in zip(ps2, clones):
        assert torch.equal(opt2.state[p]["momentum_buffer"], topt.state[c]["momentum_buffer"])
        assert opt2.state[p]["momentum_buffer"].data_ptr() == opt2._views[p].data_ptr()
    # a plain torch SGD checkpoint (no lars keys) keeps the groups' defaults
    plain = torch.optim.SGD(mk(clones)[:2] + [{"params": clones[40:]}], lr=0.1, momentum=0.9)
    opt2.load_state_dict(plain.state_dict())
    assert all("lars" in g and "lars_eps" in g for g in opt2.param_groups)
    opt2.load_state_dict(opt.state_dict())
    assert torch.equal(opt2.flat_mom, opt.flat_mom)


def test_amp_overflow_skips_every_group():
    """fp16 ResNet-18 with grouped Nesterov + LARS: a clean step_amp moves the weights; with an inf
    injected into the flat gradient the step leaves p, momentum and shadow bit-unchanged and halves
    the scale -- with no host synchronisation in either."""
    from pytorch_distributed_amd.amp import LossScaler
    from pytorch_distributed_amd.optim import build_param_groups
    nm = _native(torch.float16)
    opt = nm.make_optimizer(lr=0.1, nesterov=True,
                            param_groups=build_param_groups(nm, 1e-4, no_bn_decay=True, lars=0.001))
    crit = nm.make_criterion()
    x, y = _batch(nm)
    scaler = LossScaler(init_scale=1024.0, growth_interval=1000)
    p0 = nm.flat_params.clone()

    def step(poison):
        scaler.scale(crit(nm(x), y)).backward()
        if poison:
            nm.flat_grad[nm.fc_b_off + 1] = float("inf")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaler.step(opt)
            scaler.update()
            opt.zero_grad()
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()

    step(False)
    assert scaler.found_inf.item() == 0.0 and scaler.get_scale() == 1024.0
    assert not torch.equal(nm.flat_params, p0) and bool(nm.flat_params.isfinite().all())
    before = [t.clone() for t in (nm.flat_params, opt.flat_mom, nm.flat_shadow)]
    assert int(torch.count_nonzero(before[1])) > 0
    step(True)
    assert scaler.found_inf.item() == 1.0 and scaler.get_scale() == 512.0
    for a, b in zip(before, (nm.flat_params, opt.flat_mom, nm.flat_shadow)):
        assert torch.equal(_bits(a), _bits(b)), "an overflowing step must skip every group"


def test_captured_steps_refuse_the_segmented_optimizer(monkeypatch):
    """GraphedNativeStep and the DataParallel replica-graph path (PDA_DP_FORCE_REPLAY=1) raise
    ValueError naming MX_GRAPH / DataParallel; nothing is captured. One device without replay works."""
    from pytorch_distributed_amd.parallel.dp import DataParallel
    from pytorch_distributed_amd.runtime.graphs import GraphedNativeStep
    nm = _native()
    opt = nm.make_optimizer(nesterov=True)
    assert opt.segmented
    with pytest.raises(ValueError, match="MX_GRAPH"):
        GraphedNativeStep(nm, opt, None, 8)
    GraphedNativeStep(nm, nm.make_optimizer(), None, 8)          # the one-group optimizer is taken
    monkeypatch.setenv("PDA_DP_FORCE_REPLAY", "1")
    dp = DataParallel(nm, device_ids=[0])
    with pytest.raises(ValueError, match="DataParallel"):
        dp.make_optimizer(lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match="DataParallel"):
        dp.make_optimizer(lr=0.1, param_groups=[{"params": list(nm.parameters())}])
    x, y = _batch(nm)
    with pytest.raises(ValueError, match="DataParallel"):
        dp.train_step_chunks([x], [y], opt)
    assert getattr(dp, "_graphs", None) is None
    assert not dp.make_optimizer(lr=0.1).segmented
    monkeypatch.setenv("PDA_DP_FORCE_REPLAY", "0")
    dp1 = DataParallel(nm, device_ids=[0])
    opt1 = dp1.make_optimizer(lr=0.1, nesterov=True)
    assert opt1.segmented
    p0 = nm.flat_params.clone()
    loss = dp1.train_step_chunks([x], [y], opt1)
    torch.cuda.synchronize()
    assert bool(loss.isfinite()) and not torch.equal(nm.flat_params, p0)


def test_native_cli_run_with_every_knob(tmp_path):
    """resnet_single_gpu.py on the native engine with MX_NO_BN_DECAY, MX_NESTEROV and MX_LARS:
    exits 0 with the usual log lines."""
    e = dict(os.environ)
    e.update({"MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1",
              "MX_BATCH": "8", "MX_IMAGE_SIZE": "32", "MX_DTYPE": "bf16", "MX_METRICS": "1",
              "MX_LOG_EVERY": "1", "PYTHONPATH": ROOT, "MX_NO_BN_DECAY": "1", "MX_NESTEROV": "1",
              "MX_LARS": "0.001"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "resnet_single_gpu.py")], cwd=tmp_path,
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "epoch: 0, step: 0" in r.stdout and "epoch: 0, step: 1" in r.stdout
    assert "Epoch: 0, Loss: " in r.stdout and "Acc1: " in r.stdout and "Acc5: " in r.stdout
    assert "cost time per epoch: " in r.stdout
    loss = float(r.stdout.split("Epoch: 0, Loss: ")[1].split(",")[0])
    assert loss == loss and loss < 1e4
    assert '"engine": "native"' in (tmp_path / "output/resnet_single/metrics.jsonl").read_text()
