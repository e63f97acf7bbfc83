"""NativeSGD(clip_grad_norm=...) at the model level: native ResNet-18, 32 px, batch 8.

Bounds: the clipped update within rtol = atol = 1e-6 of the float64 reference of tests/clip_refs.py
(the bound tests/test_optim_gpu.py holds the unclipped update to), ``optimizer.grad_norm`` within
one float32 ulp of the float64 norm of the captured gradient (tests/test_clip_gpu.py derives it);
everything else -- threshold above the norm, resume, graph replay, two DDP ranks -- bit for bit.
The reference update is torch's: d = coef * g + wd * p (the weight decay is not clipped).
"""
import copy
import os
import socket

import numpy as np
import pytest
import torch

import clip_refs as CR
import optim_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
HYPER = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)


def _native(dtype=torch.bfloat16, image=32):
    from pytorch_distributed_amd.models import build_model
    from pytorch_distributed_amd.models.native import NativeResNet
    torch.manual_seed(0)
    return NativeResNet(build_model("resnet18"), device=DEV, dtype=dtype, image_size=image)


def _batch(nm, first=0, image=32, B=8):
    from pytorch_distributed_amd.data import SyntheticImageNet
    return nm.input_generator(SyntheticImageNet("train", image_size=image))(torch.arange(B) + first)


def _segments_of(nm, opt):
    base = nm.flat_params.data_ptr()
    return [((p.data_ptr() - base) // 4, p.numel()) for g in opt.param_groups for p in g["params"]]


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _steps(nm, opt, n, first=0):
    crit = nm.make_criterion()
    for i in range(n):
        x, y = _batch(nm, 8 * (first + i))
        crit(nm(x), y).backward()
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()


@pytest.mark.parametrize("segmented", [False, True], ids=["flat", "segmented"])
def test_clipped_first_step_matches_the_reference(segmented):
    """A threshold at a quarter of the first gradient's norm; the segmented variant freezes layer1
    (in no group: neither in the norm nor in the update) and runs Nesterov momentum."""
    nm = _native()
    x, y = _batch(nm)
    nm.make_criterion()(nm(x), y).backward()
    torch.cuda.synchronize()
    p0, g0 = nm.flat_params.cpu(), nm.flat_grad.cpu()
    kw = dict(HYPER)
    if segmented:
        frozen = {id(p) for p in nm.layer1.parameters()}
        kw.update(nesterov=True,
                  param_groups=[{"params": [p for p in nm.parameters() if id(p) not in frozen]}])
    segs = _segments_of(nm, nm.make_optimizer(**kw))
    norm = CR.norm64(g0, segs)
    every = _segments_of(nm, nm.make_optimizer(**HYPER))
    assert norm > 0 and (norm < CR.norm64(g0, every) if segmented else segs == every)
    max_norm = 0.25 * norm
    opt = nm.make_optimizer(clip_grad_norm=max_norm, **kw)
    assert opt.segmented is segmented and opt.clip_grad_norm == max_norm
    opt.step()
    torch.cuda.synchronize()
    got_norm = opt.grad_norm.item()
    print(f"grad_norm {got_norm!r}, float64 norm {norm!r}, scale {opt._clip_out[1].item()!r}")
    assert opt.grad_norm.shape == (1,) and _ulps(got_norm, np.float32(norm)) <= 1
    hyper = [{k: v for k, v in kw.items() if k != "param_groups"}] * len(segs)
    ref = CR.clipped_sgd_ref(p0, g0, segs, hyper, 1, max_norm)[0]
    assert 0.2 < float(CR.scale32(g0, segs, max_norm)) < 0.3
    inside = torch.zeros(nm.numel, dtype=torch.bool)
    for o, s in segs:
        inside[o:o + s] = True
    p, buf = nm.flat_params.cpu(), opt.flat_mom.cpu()
    torch.testing.assert_close(p[inside].to(F64), ref[0][inside].to(F64), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(buf[inside].to(F64), ref[1][inside].to(F64), rtol=1e-6, atol=1e-6)
    assert torch.equal(_bits(p)[~inside], _bits(p0)[~inside])
    assert int(torch.count_nonzero(buf[~inside])) == 0
    # and it is not the unclipped update
    plain = R.seg_sgd_ref(p0, g0, segs, hyper, 1)[0][0]
    assert float((p[inside] - plain[inside]).abs().max()) > 1e-4


def test_threshold_above_the_norm_changes_no_bit():
    runs = []
    for clip in (0.0, 1e9):
        nm = _native()
        opt = nm.make_optimizer(clip_grad_norm=clip, **HYPER)
        _steps(nm, opt, 3)
        runs.append((nm.flat_params.clone(), opt.flat_mom.clone(), nm.flat_shadow.clone()))
        if clip:
            assert 0 < opt.grad_norm.item() < 1e9 and opt._clip_out[1].item() == 1.0
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


def test_off_owns_nothing_and_launches_nothing(monkeypatch):
    from pytorch_distributed_amd.models import native_train
    calls = []
    real = native_train.K.grad_clip
    monkeypatch.setattr(native_train.K, "grad_clip", lambda *a, **k: calls.append(1) or real(*a, **k))
    nm = _native()
    opt = nm.make_optimizer(**HYPER)
    assert opt.clip_grad_norm == 0.0 and opt.grad_norm is None
    assert not [k for k in vars(opt) if k.startswith("_clip")]
    _steps(nm, opt, 1)
    assert calls == []
    on = nm.make_optimizer(clip_grad_norm=1.0, **HYPER)
    _steps(nm, on, 2)
    assert calls == [1, 1]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_grad_norm"):
            nm.make_optimizer(clip_grad_norm=bad)


def test_amp_overflow_is_skipped_with_no_host_sync():
    """fp16: a clean clipped step_amp moves the weights and publishes the UNSCALED norm; with an inf
    in the flat gradient the step leaves weights, momentum and shadow untouched and halves the
    scale -- no host synchronisation in either."""
    from pytorch_distributed_amd.amp import LossScaler
    nm = _native(torch.float16)
    opt = nm.make_optimizer(clip_grad_norm=0.5, **HYPER)
    crit = nm.make_criterion()
    x, y = _batch(nm)
    scaler = LossScaler(init_scale=1024.0, growth_interval=1000)
    p0 = nm.flat_params.clone()
    segs = _segments_of(nm, opt)
    grads = []

    def step(poison):
        scaler.scale(crit(nm(x), y)).backward()
        if poison:
            nm.flat_grad[nm.fc_b_off + 1] = float("inf")
        torch.cuda.synchronize()
        grads.append(nm.flat_grad.cpu())
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
    want = CR.norm32(grads[0], segs, 1.0 / 1024.0)
    assert want > 0.5 and _ulps(opt.grad_norm.item(), want) <= 1
    assert opt._clip_out[1].item() == float(np.float32(1.0 / 1024.0) * CR.coef32(opt.grad_norm.item(), 0.5))
    before = [t.clone() for t in (nm.flat_params, opt.flat_mom, nm.flat_shadow)]
    assert int(torch.count_nonzero(before[1])) > 0
    step(True)
    assert scaler.found_inf.item() == 1.0 and scaler.get_scale() == 512.0
    assert opt._clip_out[1].item() == 1.0 / 1024.0          # a skipped step: the bare 1/scale
    for a, b in zip(before, (nm.flat_params, opt.flat_mom, nm.flat_shadow)):
        assert torch.equal(_bits(a), _bits(b)), "an overflowing step must be skipped"


def test_resume_needs_no_clip_state():
    """Two steps, save model and optimizer, two more; a fresh pair loaded from the save and run for
    those two steps ends bit-equal: the clip holds no state of its own."""
    nm = _native()
    opt = nm.make_optimizer(clip_grad_norm=0.3, **HYPER)
    _steps(nm, opt, 2)
    saved = copy.deepcopy((nm.state_dict(), opt.state_dict()))
    assert not [k for k in saved[1]["param_groups"][0] if "clip" in k]
    _steps(nm, opt, 2, first=2)
    assert opt.grad_norm.item() > 0.3
    nm2 = _native()
    opt2 = nm2.make_optimizer(clip_grad_norm=0.3, **HYPER)
    nm2.load_state_dict(saved[0])
    opt2.load_state_dict(saved[1])
    _steps(nm2, opt2, 2, first=2)
    for a, b in ((nm.flat_params, nm2.flat_params), (opt.flat_mom, opt2.flat_mom),
                 (nm.flat_buffers, nm2.flat_buffers), (opt.grad_norm, opt2.grad_norm)):
        assert torch.equal(_bits(a), _bits(b))


def _trainer(graph):
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.runtime.graphs import GraphedNativeStep, single_queue_graphs
    tr = NativeTrainer("resnet18", 8, torch.bfloat16, DEV, image_size=32, graph=False)
    tr.opt = tr.model.make_optimizer(clip_grad_norm=0.1, **HYPER)
    if graph and single_queue_graphs():        # (NativeTrainer's own condition for graph=True)
        tr.graphed = GraphedNativeStep(tr.model, tr.opt, tr.gen, tr.batch, tr.scaler, DEV)
    losses = []
    for i in range(3):
        tr.step(i)
        losses.append(tr.last_loss())
    torch.cuda.synchronize()
    return tr, losses


def test_graph_replay_matches_eager():
    """The pattern of tests/test_graph_gpu.py: three replayed steps against three eager ones."""
    te, le = _trainer(False)
    tg, lg = _trainer(True)
    assert tg.graphed.captures == 1
    assert le == lg, (le, lg)
    assert te.opt.grad_norm.item() > 0.1                    # the clip is active
    for a, b in ((te.model.flat_params, tg.model.flat_params), (te.opt.flat_mom, tg.opt.flat_mom),
                 (te.model.flat_buffers, tg.model.flat_buffers), (te.opt.grad_norm, tg.opt.grad_norm)):
        assert torch.equal(_bits(a), _bits(b))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["PDA_COMM"] = "torch"
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", world_size=world, rank=rank)
    torch.cuda.set_device(0)
    from pytorch_distributed_amd.bench_step import tensor_checksum
    from pytorch_distributed_amd.parallel import DistributedDataParallel
    nm = _native()
    ddp = DistributedDataParallel(nm, bucket_cap_mb=4.0)
    opt = nm.make_optimizer(clip_grad_norm=0.2, **HYPER)
    crit = nm.make_criterion()
    for i in range(2):
        x, y = _batch(nm, 8 * (i * world + rank))
        opt.zero_grad()
        crit(ddp(x), y).backward()
        opt.step()
    torch.cuda.synchronize()
    q.put((rank, tensor_checksum([nm.flat_params, opt.flat_mom]).cpu().tolist(),
           int(_bits(opt.grad_norm)[0]), opt.grad_norm.item()))
    dist.destroy_process_group()


def test_ddp_two_ranks_clip_identically():
    """Two ranks on one GPU (gloo, as tests/test_ddp_gpu.py): each clips its own copy of the
    all-reduced gradient; checksums and grad_norm bits agree."""
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_ddp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(world))
    for p in ps:
        p.join(120)
        assert p.exitcode == 0
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2], res
    assert res[0][3] > 0.2                                   # the clip was active
