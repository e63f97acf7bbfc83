"""Shared training driver for the four entrypoints (reference L5).

Each reference script re-implements the same ``train`` / ``validate`` /
``main`` skeleton (``resnet_single_gpu.py:17-134``, ``resnet_dp.py:14-129``,
``restnet_ddp.py:19-150``, ``resnet_ddp_apex.py:19-155``); the per-script deltas
are listed in SURVEY §2.2. They are expressed here as :class:`RunConfig` fields
and the ``mode`` argument (``single`` / ``dp`` / ``ddp`` / ``ddp_amp``).

Behaviour kept byte-compatible with the reference: hyper-parameters, the
epoch loop (train -> ``scheduler.step()`` -> validate, timed as one span), the four
stdout line formats, ``latest.pt``/``best.pt`` schemas and paths. Reference
bugs fixed deliberately: Q1/Q2 (bad save/suspend calls), Q3
(python-int counters in single-GPU validate), Q5 (rank-0-only suspend poll ->
collective decision), Q6/Q7 (print/return on global rank 0 with all-reduced
counters), Q8 (per-step ``empty_cache`` opt-in via ``MX_EMPTY_CACHE=step``), Q9
(GradScaler state saved under ``'scaler'``), Q10 (resume seeks instead of
re-reading skipped batches).
"""
from __future__ import annotations

import contextlib
import os
import time
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Optional

import torch
from torch import nn

from .config import RunConfig
from .data import DistributedSampler, SyntheticImageNet
from .utils.checkpoint import load_latest, save_best, save_latest
from .utils.metrics import MetricsLog, gpu_mem_gb
from .utils.suspend import SuspendMonitor, go_suspend

__all__ = ["Context", "train", "validate", "run", "resolve_device", "resolve_dtype",
           "load_model_state"]


@dataclass
class Context:
    cfg: RunConfig
    device: torch.device
    dtype: torch.dtype
    engine: str                       # "native" | "torch"
    rank: int = 0
    world: int = 1
    local_rank: int = 0
    distributed: bool = False
    suspend: Optional[SuspendMonitor] = None
    scaler: Any = None
    metrics: Optional[MetricsLog] = None
    extra: dict = field(default_factory=dict)

    @property
    def is_main(self) -> bool:
        return self.rank == 0


def resolve_device(cfg: RunConfig, local_rank: int = 0) -> torch.device:
    if cfg.device == "cpu" or (cfg.device == "auto" and not torch.cuda.is_available()):
        return torch.device("cpu")
    if not torch.cuda.is_available():
        raise RuntimeError("MX_DEVICE=cuda but no GPU is visible")
    torch.cuda.set_device(local_rank)
    return torch.device("cuda", local_rank)


def resolve_dtype(cfg: RunConfig, device: torch.device) -> torch.dtype:
    """``auto`` = the reference script's precision: fp32 for the single / DP / DDP scripts
    (``resnet_single_gpu.py:27-31``, ``resnet_dp.py:21-25``, ``restnet_ddp.py:26-30`` run
    without autocast), fp16 for the AMP script (its SCRIPT_DEFAULTS). bf16 is opt-in
    (``MX_DTYPE=bf16``)."""
    d = cfg.dtype
    if d == "auto":
        d = "fp32"
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[d]


def resolve_engine(cfg: RunConfig, device: torch.device, dtype: torch.dtype) -> str:
    if cfg.engine in ("native", "torch"):
        return cfg.engine
    if device.type != "cuda":
        return "torch"
    from .models import native
    return "native" if native.supports(cfg.arch, dtype) else "torch"


def _autocast(ctx: Context):
    if ctx.engine == "torch" and ctx.dtype != torch.float32:
        return torch.autocast(device_type=ctx.device.type, dtype=ctx.dtype)
    return torch.autocast(device_type=ctx.device.type, enabled=False)


def _unwrap(model: nn.Module) -> nn.Module:
    return getattr(model, "module", model)


def load_model_state(model: nn.Module, state_dict) -> None:
    """Resume-time model load (reference ``restnet_ddp.py:127-132`` loads into the unwrapped
    module). DataParallel must load through the wrapper, which re-copies the weights into every
    replica -- loading only ``.module`` would leave replicas 1..N-1 on their old weights."""
    (model if hasattr(model, "replicas") else _unwrap(model)).load_state_dict(state_dict)


def _sync_step(ctx: Context) -> None:
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()
        if ctx.cfg.empty_cache == "step":
            torch.cuda.empty_cache()


def _graphed_step(model, optimizer, ctx: Context):
    """``MX_GRAPH=1`` (single process, native engine, one GPU): the whole training step --
    forward, loss, backward, fused SGD (+ AMP scale update) -- replayed from ONE HIP graph per step
    (:class:`~pytorch_distributed_amd.runtime.graphs.GraphedNativeStep`; re-captured when the LR
    scheduler changes the learning rate, a ragged last batch runs eagerly). Kept on the context so
    one capture serves every epoch."""
    if not ctx.cfg.graph or ctx.distributed or ctx.device.type != "cuda" or ctx.engine != "native":
        return None
    if not hasattr(model, "native_forward") or hasattr(model, "replicas"):
        return None
    from .runtime.graphs import graphs_unsafe_warning, single_queue_graphs
    if not single_queue_graphs():
        graphs_unsafe_warning("MX_GRAPH=1")
        return None
    g = ctx.extra.get("graphed")
    if g is None:
        from .runtime.graphs import GraphedNativeStep
        g = GraphedNativeStep(model, optimizer, None, ctx.cfg.batch_size, ctx.scaler, ctx.device)
        ctx.extra["graphed"] = g
    return g


def _batch_mixer(ctx: Context):
    """``MX_MIXUP`` / ``MX_CUTMIX``: the run's :class:`~pytorch_distributed_amd.mix.BatchMixer`
    (kept on the context: one output buffer serves every epoch), else None."""
    if not (ctx.cfg.mixup > 0 or ctx.cfg.cutmix > 0):
        return None
    mixer = ctx.extra.get("mixer")
    if mixer is None:
        from .mix import BatchMixer
        mixer = ctx.extra["mixer"] = BatchMixer(ctx.cfg, ctx)
    return mixer


def _batch_eraser(ctx: Context):
    """``MX_RANDOM_ERASE``: the run's :class:`~pytorch_distributed_amd.erase.BatchEraser` (kept on
    the context: one box table serves every epoch), else None."""
    if not ctx.cfg.random_erase > 0:
        return None
    eraser = ctx.extra.get("eraser")
    if eraser is None:
        from .erase import BatchEraser
        eraser = ctx.extra["eraser"] = BatchEraser(ctx.cfg, ctx)
    return eraser


def train(dataloader, model, criterion, optimizer, scheduler, epoch: int, ctx: Context,
          start_step: int, best_acc: float, save_path: Path) -> int:
    """One epoch of training (reference ``restnet_ddp.py:19-47``). Returns steps run."""
    model.train()
    cfg = ctx.cfg
    steps = 0
    scaler = ctx.scaler
    soft = cfg.soft_targets
    mixer = _batch_mixer(ctx)
    eraser = _batch_eraser(ctx)
    from .utils.metrics import StepProfiler
    prof = StepProfiler(int(os.environ.get("MX_PROFILE", "0") or 0) if epoch == 0 else 0, save_path,
                        ctx.rank)
    # soft targets run the eager branches: a captured step (MX_GRAPH=1, DataParallel's train_step)
    # takes hard labels only
    graphed = None if soft else _graphed_step(model, optimizer, ctx)
    ema = ctx.extra.get("ema")          # MX_EMA: the weight average follows every optimizer step
    sb = ctx.extra.get("step_busy")     # device-busy fallback (utils/gpu_util.py StepBusy)
    # MX_CLIP_GRAD_NORM: the native optimizer clips inside its step (csrc/clip.hip) and keeps the
    # norm in optimizer.grad_norm; torch optimizers are clipped here, before optimizer.step()
    clip_params = grad_norm = None
    if cfg.clip_grad_norm > 0 and not hasattr(optimizer, "clip_grad_norm"):
        clip_params = [p for g in optimizer.param_groups for p in g["params"]]
    for step, (samples, labels) in dataloader.iter_from(start_step):
        if ctx.cfg.script == "single" and cfg.log_every and step % cfg.log_every == 0:
            print("epoch: {}, step: {}".format(epoch, step), flush=True)
        if sb is not None:
            sb.begin()
        samples = samples.to(ctx.device, non_blocking=True)
        labels = labels.to(ctx.device, non_blocking=True)
        if eraser is not None:
            # per-sample transform, so before the mixing (torchvision's order); in place: every
            # loader makes a fresh batch per step, and the captured steps (MX_GRAPH=1, DataParallel)
            # copy the batch they are handed on this stream, after the erase
            samples = eraser(samples, epoch, step)
        soft_args = ()                   # (labels_b, lam): the criterion's two further arguments
        if soft:
            labels_b, lam = None, 1.0
            if mixer is not None:
                samples, labels, labels_b, lam = mixer(samples, labels, epoch, step)
            soft_args = (labels_b, lam)
        if graphed is not None and graphed.accepts(samples):
            graphed.run_batch(samples, labels)      # MX_GRAPH=1: the whole step, one graph launch
            loss = graphed.loss
        elif (not soft and getattr(model, "graph_step_ok", None) is not None
              and model.graph_step_ok(scaler)):
            loss = model.train_step(samples, labels, optimizer)     # DP: HIP-graph replay per GPU
        elif scaler is not None and scaler.enabled:
            with _autocast(ctx):
                outputs = model(samples)
                loss = criterion(outputs, labels, *soft_args)
            scaler.scale(loss).backward()
            if clip_params is not None:
                scaler.unscale_(optimizer)
                grad_norm = torch.nn.utils.clip_grad_norm_(clip_params, cfg.clip_grad_norm)
            scaler.step(optimizer)
            scaler.update()
            optimizer.zero_grad()
        else:
            with _autocast(ctx):
                outputs = model(samples)
            optimizer.zero_grad()
            loss = criterion(outputs.float() if outputs.dtype != torch.float32 else outputs, labels,
                             *soft_args)
            loss.backward()
            if clip_params is not None:
                grad_norm = torch.nn.utils.clip_grad_norm_(clip_params, cfg.clip_grad_norm)
            optimizer.step()
        if ema is not None:
            ema.update()
        if sb is not None:
            sb.end()
        _sync_step(ctx)
        steps += 1
        prof.step()
        if ctx.suspend is not None:
            ctx.suspend.tick()
            if ctx.suspend.requested():
                if ctx.is_main:
                    save_latest(save_path, _unwrap(model).state_dict(), optimizer.state_dict(),
                                scheduler.state_dict(), best_acc, epoch, step + 1,
                                scaler.state_dict() if scaler is not None and scaler.enabled else None,
                                **({"ema_sd": ema.state_dict()} if ema is not None else {}))
                    print(f"suspend: saved {save_path / 'latest.pt'} at epoch {epoch} step {step + 1}",
                          flush=True)
                go_suspend()
    prof.close()
    if cfg.clip_grad_norm > 0:
        # the pre-clip norm of the epoch's last step: a device tensor, read by run() after validation
        ctx.extra["grad_norm"] = (getattr(optimizer, "grad_norm", None) if clip_params is None
                                  else grad_norm)
    return steps


def validate(dataloader, model, criterion, epoch: int, ctx: Context, prefix: str = "") -> float:
    """Top-1/top-5 validation (reference ``restnet_ddp.py:50-72``); ``prefix`` goes in front of the
    log line (``"EMA "``: the pass over the averaged weights).

    Counters live on the device (fixes Q3); in DDP they are all-reduced in ONE
    4-element collective (instead of 4 ``dist.reduce`` calls) so every rank returns
    the same accuracy (fixes Q7) and only global rank 0 prints (Q6). Loss is
    normalised as the reference does: sum of batch means / world / len(loader).
    """
    stats = torch.zeros(4, device=ctx.device)  # loss, correct1, correct5, total
    model.eval()
    with torch.no_grad():
        for samples, labels in dataloader:
            samples = samples.to(ctx.device, non_blocking=True)
            labels = labels.to(ctx.device, non_blocking=True)
            outputs = model(samples).float()
            stats[0] += criterion(outputs, labels)
            if ctx.engine == "native" and outputs.is_cuda:
                from .ops import native_ops as K
                # one HIP kernel: label rank per row -> top-1 / top-5 hit counters (K11)
                K.topk_hits(outputs.contiguous(), labels, stats[1:3])
            else:
                _, preds = outputs.topk(5, -1, True, True)
                hit = torch.eq(preds, labels.unsqueeze(1))
                stats[1] += hit[:, :1].sum()
                stats[2] += hit.sum()
            stats[3] += samples.size(0)
    if ctx.distributed:
        comm = getattr(model, "comm", None)
        if comm is not None and stats.is_cuda:
            comm.all_reduce(stats)        # the DDP's own RCCL communicator (M6: one 4-element call)
        else:
            import torch.distributed as dist
            dist.all_reduce(stats)
    loss, c1, c5, total = stats.tolist()
    nb = max(len(dataloader), 1)
    loss_val = loss / ctx.world / nb
    total = max(total, 1.0)
    if ctx.is_main:
        print(f'{prefix}Epoch: {epoch}, Loss: {loss_val}, Acc1: {100 * c1 / total:.2f}%, '
              f'Acc5: {100 * c5 / total:.2f}%', flush=True)
    return c1 / total


def _make_folder_loaders(cfg: RunConfig, ctx: Context, per_rank_batch: int, model=None):
    from .data.folder import ImageFolder, train_params, train_transform, val_params, val_transform
    root = cfg.data.split(":", 1)[1]
    val_resize = int(round(cfg.image_size * 256 / 224))
    extra = {}
    if cfg.aug == "gpu":
        # workers decode only; one HIP kernel (csrc/augment.hip) makes the model-ready batch. The
        # native engine on one device takes its s2d layout in the model dtype, the torch engine and
        # DataParallel (which scatters NCHW batches) take NCHW f32
        s2d = ctx.engine == "native" and not hasattr(model, "replicas")
        extra = dict(device=ctx.device, image_size=cfg.image_size, layout="s2d" if s2d else "nchw",
                     dtype=ctx.dtype if s2d else torch.float32)
        train_ds = ImageFolder(root, "train", raw_params=train_params())
        val_ds = ImageFolder(root, "val", raw_params=val_params(cfg.image_size, val_resize))
    else:
        train_ds = ImageFolder(root, "train", train_transform(cfg.image_size))
        val_ds = ImageFolder(root, "val", val_transform(cfg.image_size, val_resize))
    train_sampler = val_sampler = None
    if ctx.distributed:
        train_sampler = DistributedSampler(train_ds, ctx.world, ctx.rank, shuffle=True, seed=cfg.seed)
        val_sampler = DistributedSampler(val_ds, ctx.world, ctx.rank, shuffle=True, seed=cfg.seed)
    tl = train_ds.loader(per_rank_batch, sampler=train_sampler, num_workers=cfg.num_workers,
                         max_steps=cfg.steps_per_epoch, **extra)
    vl = val_ds.loader(per_rank_batch, sampler=val_sampler, num_workers=cfg.num_workers,
                       max_steps=cfg.val_steps, **extra)
    return tl, vl, train_sampler


def _make_packed_loaders(cfg: RunConfig, ctx: Context, per_rank_batch: int, model=None):
    """``MX_DATA=packed:<dir>``: ``<dir>/train.pack`` and ``<dir>/val.pack`` (data/packed.py), made
    resident per ``MX_PACK_RESIDENT``; crops are drawn and resampled on the GPU, no worker
    processes. Layout and dtype as for ``MX_AUG=gpu``. Under DDP every rank holds its own copy."""
    from .data.packed import PackedImages, PackedLoader
    root = cfg.data.split(":", 1)[1]
    if ctx.device.type != "cuda":
        raise ValueError(f"MX_DATA=packed: resamples on the GPU (csrc/augment.hip); the device is "
                         f"{ctx.device}. Use MX_DATA=folder:<root> on a CPU device.")
    s2d = ctx.engine == "native" and not hasattr(model, "replicas")
    kw = dict(dtype=ctx.dtype if s2d else torch.float32, layout="s2d" if s2d else "nchw",
              image_size=cfg.image_size, resize=int(round(cfg.image_size * 256 / 224)), seed=cfg.seed)
    loaders, train_sampler = [], None
    for split, max_steps in (("train", cfg.steps_per_epoch), ("val", cfg.val_steps)):
        images = PackedImages(os.path.join(root, split + ".pack"))
        sampler = None
        if ctx.distributed:
            sampler = DistributedSampler(images, ctx.world, ctx.rank, shuffle=True, seed=cfg.seed)
            train_sampler = train_sampler or sampler
        loaders.append(PackedLoader(images.to_device(ctx.device, cfg.pack_resident), split,
                                    per_rank_batch, sampler=sampler, max_steps=max_steps, **kw))
    return loaders[0], loaders[1], train_sampler


def _make_loaders(cfg: RunConfig, ctx: Context, model: nn.Module, per_rank_batch: int):
    if cfg.data.startswith("folder:"):
        return _make_folder_loaders(cfg, ctx, per_rank_batch, model)
    if cfg.data.startswith("packed:"):
        return _make_packed_loaders(cfg, ctx, per_rank_batch, model)
    if cfg.data != "synthetic":
        raise ValueError(f"MX_DATA must be 'synthetic', 'folder:<root>' or 'packed:<dir>', got "
                         f"{cfg.data!r}")
    train_ds = SyntheticImageNet("train", cfg.train_samples, cfg.seed, cfg.num_classes, cfg.image_size)
    val_ds = SyntheticImageNet("val", cfg.val_samples, cfg.seed, cfg.num_classes, cfg.image_size)
    if ctx.distributed:
        train_sampler = DistributedSampler(train_ds, ctx.world, ctx.rank, shuffle=True, seed=cfg.seed)
        val_sampler = DistributedSampler(val_ds, ctx.world, ctx.rank, shuffle=True, seed=cfg.seed)
    else:
        train_sampler = val_sampler = None
    gen_train = gen_val = None
    inner = _unwrap(model)
    if hasattr(inner, "input_generator"):
        gen_train = inner.input_generator(train_ds)
        gen_val = inner.input_generator(val_ds)
    tl = train_ds.loader(per_rank_batch, sampler=train_sampler, num_workers=cfg.num_workers,
                         device=ctx.device, generator=gen_train, max_steps=cfg.steps_per_epoch)
    vl = val_ds.loader(per_rank_batch, sampler=val_sampler, num_workers=cfg.num_workers,
                       device=ctx.device, generator=gen_val, max_steps=cfg.val_steps)
    return tl, vl, train_sampler


def build_model(cfg: RunConfig, ctx: Context) -> nn.Module:
    from .models.resnet import build_model as build_ref
    torch.manual_seed(cfg.seed)
    model = build_ref(cfg.arch, cfg.num_classes)
    if ctx.engine == "native":
        from .models.native import NativeResNet
        return NativeResNet(model, device=ctx.device, dtype=ctx.dtype, image_size=cfg.image_size)
    return model.to(ctx.device)


def _factory_owner(model: nn.Module, attr: str):
    """The wrapper (DataParallel) if it provides ``attr``, else the wrapped module."""
    return model if hasattr(model, attr) else _unwrap(model)


def build_optimizer(cfg: RunConfig, model: nn.Module, ctx: Context):
    """SGD as the reference builds it; ``MX_NESTEROV`` / ``MX_NO_BN_DECAY`` / ``MX_LARS`` turn it into
    grouped SGD (:func:`~pytorch_distributed_amd.optim.build_param_groups`): the segmented kernel on
    the native engine, ``torch.optim.SGD`` or :class:`~pytorch_distributed_amd.optim.LARS` on the
    torch engine. The captured-step paths refuse the segmented optimizer (ValueError, raised here:
    before training starts). ``MX_CLIP_GRAD_NORM`` goes to the native optimizer, which clips inside
    its step; the torch optimizers are clipped by :func:`train`. DataParallel over several devices
    (or with ``PDA_DP_FORCE_REPLAY=1``) refuses it, here as well."""
    inner = _factory_owner(model, "make_optimizer")
    native = hasattr(inner, "make_optimizer")
    clip = {}
    if cfg.clip_grad_norm > 0:
        from .runtime.graphs import CLIP_REFUSAL, DP_REPLAY, replays_captured_steps
        if replays_captured_steps(model):
            raise ValueError(CLIP_REFUSAL.format(what=DP_REPLAY))
        clip = dict(clip_grad_norm=cfg.clip_grad_norm)
    if not (cfg.nesterov or cfg.no_bn_decay or cfg.lars > 0):
        if native:
            return inner.make_optimizer(lr=cfg.lr, momentum=cfg.momentum,
                                        weight_decay=cfg.weight_decay, **clip)
        return torch.optim.SGD(model.parameters(), lr=cfg.lr, momentum=cfg.momentum,
                               weight_decay=cfg.weight_decay)
    from .optim import LARS, build_param_groups
    if native and cfg.graph and ctx.engine == "native":
        from .runtime.graphs import SEGMENTED_REFUSAL
        raise ValueError(SEGMENTED_REFUSAL.format(what="MX_GRAPH=1"))
    groups = build_param_groups(_unwrap(model), cfg.weight_decay, cfg.no_bn_decay, cfg.lars)
    kw = dict(lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay, nesterov=cfg.nesterov)
    if native:      # (DataParallel over several devices raises the same ValueError)
        return inner.make_optimizer(param_groups=groups, **kw, **clip)
    if cfg.lars > 0:
        return LARS(groups, **kw)
    return torch.optim.SGD(groups, **kw)


def _refuse_soft_targets(cfg: RunConfig, model: nn.Module, ctx: Context) -> None:
    """Captured steps bake the loss arguments in at capture: ``MX_GRAPH=1`` and DataParallel over
    several devices refuse label smoothing / mixup / CutMix (ValueError, before training starts)."""
    if not cfg.soft_targets:
        return
    from .mix import MIX_REFUSAL
    if cfg.graph and ctx.engine == "native":
        raise ValueError(MIX_REFUSAL.format(what="MX_GRAPH=1"))
    from .runtime.graphs import DP_REPLAY, replays_captured_steps
    if replays_captured_steps(model):
        raise ValueError(MIX_REFUSAL.format(what=DP_REPLAY))


def build_criterion(ctx: Context, model: nn.Module):
    """The loss: the native engine's fused kernel, else ``nn.CrossEntropyLoss``. With
    ``MX_LABEL_SMOOTHING`` / ``MX_MIXUP`` / ``MX_CUTMIX`` the criterion takes ``(outputs, labels,
    labels_b, lam)``: the native one with the smoothing passed through, on the torch engine and
    the CPU :class:`~pytorch_distributed_amd.mix.SoftCrossEntropy`."""
    cfg = ctx.cfg
    _refuse_soft_targets(cfg, model, ctx)
    inner = _factory_owner(model, "make_criterion")
    if hasattr(inner, "make_criterion"):
        if cfg.label_smoothing > 0:
            crit = inner.make_criterion(label_smoothing=cfg.label_smoothing)
        else:
            crit = inner.make_criterion()
        # a factory that wraps a torch module (DataParallel on the torch engine or the CPU) hands
        # back a hard-label loss: soft targets need one that takes (labels_b, lam)
        if not cfg.soft_targets or getattr(crit, "soft_targets", False):
            return crit
    if cfg.soft_targets:
        from .mix import SoftCrossEntropy
        return SoftCrossEntropy(cfg.label_smoothing)
    return nn.CrossEntropyLoss()


def run(cfg: RunConfig, mode: str, local_rank: int = 0, nprocs: Optional[int] = None) -> float:
    """``main()`` of the reference scripts. Returns the best top-1 accuracy."""
    from .launch import dist_env, init_distributed
    distributed = mode in ("ddp", "ddp_amp")
    if mode == "dp" or cfg.graph:   # before the first HIP call (resolve_device sets the device)
        from .runtime.graphs import request_single_queue_graphs
        request_single_queue_graphs()
    device = resolve_device(cfg, local_rank)
    dtype = resolve_dtype(cfg, device)
    engine = resolve_engine(cfg, device, dtype)
    ctx = Context(cfg=cfg, device=device, dtype=dtype, engine=engine, local_rank=local_rank)
    if distributed:
        env = dist_env(local_rank, nprocs)
        backend = "nccl" if device.type == "cuda" else "gloo"
        init_distributed(env, backend, device=device)
        # the DDP scripts take the distributed code path (sampler, all-reduced validation) even
        # with a single process, as the reference does
        ctx.rank, ctx.world, ctx.distributed = env.rank, env.world_size, True
    save_path = Path(cfg.save_path)
    save_path.mkdir(exist_ok=True, parents=True)
    ctx.metrics = MetricsLog(save_path / "metrics.jsonl", enabled=cfg.metrics and ctx.is_main)
    ctx.suspend = SuspendMonitor()

    model = build_model(cfg, ctx)
    if mode == "dp":
        from .parallel.dp import DataParallel
        model = DataParallel(model)
    elif distributed:
        from .parallel.ddp import DistributedDataParallel, convert_sync_batchnorm
        if cfg.sync_bn:
            model = convert_sync_batchnorm(model)
        model = DistributedDataParallel(model, device_ids=[local_rank] if device.type == "cuda" else None,
                                        bucket_cap_mb=cfg.bucket_mb or None)
    per_rank_batch = cfg.batch_size
    train_loader, val_loader, train_sampler = _make_loaders(cfg, ctx, model, per_rank_batch)
    criterion = build_criterion(ctx, model)
    optimizer = build_optimizer(cfg, model, ctx)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=cfg.lr_step, gamma=cfg.lr_gamma)
    if mode == "ddp_amp":
        from .amp import LossScaler
        ctx.scaler = LossScaler(enabled=(dtype == torch.float16))

    best_acc, start_epoch, start_step = 0.0, 0, 0
    ckpt = load_latest(save_path)
    if ckpt is not None:
        load_model_state(model, ckpt["model"])
        optimizer.load_state_dict(ckpt["optimizer"])
        scheduler.load_state_dict(ckpt["scheduler"])
        if ctx.scaler is not None and "scaler" in ckpt:
            ctx.scaler.load_state_dict(ckpt["scaler"])
        best_acc, start_epoch, start_step = ckpt["acc"], ckpt["epoch"], ckpt["step"]
        if ctx.is_main:
            print(f"resume: epoch {start_epoch} step {start_step} (best acc {best_acc})", flush=True)
    if cfg.ema > 0:
        # after the resume: the average starts from the weights the run continues with, unless the
        # checkpoint brings its own (every DDP rank averages its own, identical weights)
        from .ema import build_ema
        ema = ctx.extra["ema"] = build_ema(cfg, model, ctx)
        if ckpt is not None and "ema" in ckpt:
            ema.load_state_dict(ckpt["ema"])
    ema = ctx.extra.get("ema")

    for epoch in range(start_epoch, cfg.epochs):
        t1 = time.time()
        if train_sampler is not None:
            train_sampler.set_epoch(epoch)
        if hasattr(train_loader, "set_epoch"):      # packed data: the epoch of the crop draws
            train_loader.set_epoch(epoch)
        from .utils.gpu_util import BusySampler, StepBusy, busy_path
        devs = ([ctx.device.index if ctx.device.index is not None else torch.cuda.current_device()]
                if ctx.device.type == "cuda" else [])
        if hasattr(model, "device_ids"):     # DataParallel: every replica's device
            devs = list(model.device_ids)
        # where the driver's sysfs counter is unreadable (containers), HIP events around the steps
        sbusy = StepBusy(torch.device("cuda", devs[0]) if devs else None)
        ctx.extra["step_busy"] = sbusy if not any(busy_path(d) is not None for d in devs) else None
        with BusySampler(devs) as busy, sbusy:   # the reference's "Avg GPU Util" panel (README:33-40)
            steps = train(train_loader, model, criterion, optimizer, scheduler, epoch, ctx,
                          start_step, best_acc, save_path)
        util, util_method = busy.overall(), "sysfs gpu_busy_percent"
        if util is None:
            util, util_method = sbusy.overall(), "step intervals (HIP events) / wall time"
        start_step = 0
        scheduler.step()
        acc = validate(val_loader, model, criterion, epoch, ctx)
        # MX_EMA: a second pass over the averaged weights, which then decide (and are) best.pt
        with ema.swapped() if ema is not None else contextlib.nullcontext():
            more = {}
            if cfg.clip_grad_norm > 0 and ctx.extra.get("grad_norm") is not None:
                more["grad_norm"] = float(ctx.extra["grad_norm"])
            if ema is not None:
                more["ema_acc1"] = validate(val_loader, model, criterion, epoch, ctx, prefix="EMA ")
            t2 = time.time()
            if cfg.empty_cache == "epoch" and device.type == "cuda":
                torch.cuda.empty_cache()
            if ctx.is_main:
                print("cost time per epoch: {:.4f} s".format(t2 - t1), flush=True)
                ctx.metrics.write(epoch=epoch, steps=steps, epoch_s=t2 - t1, acc1=acc,
                                  images=steps * per_rank_batch * ctx.world, gpu_mem_gb=gpu_mem_gb(),
                                  gpu_util_pct=util,
                                  gpu_util_method=util_method if util is not None else None,
                                  engine=engine, dtype=str(dtype), **more)
                acc = more.get("ema_acc1", acc)
                if acc > best_acc:
                    best_acc = acc
                    print(f'New Best Acc: {100 * acc:.2f}%!', flush=True)
                    save_best(save_path, _unwrap(model).state_dict())
    if distributed:
        import torch.distributed as dist
        from .launch import host_group
        dist.barrier(group=host_group())
        dist.destroy_process_group()
    return best_acc
