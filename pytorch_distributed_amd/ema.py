"""Exponential moving average (EMA) of the weights: the model that torchvision's reference recipe
and timm validate and save when training with mixup, CutMix and large batches.

* :func:`ema_weight` -- the schedule: ``d = min(decay, (1 + t) / (10 + t))`` with warmup (``t`` = the
  updates already applied), else ``decay``; computed in double and handed on as ``float32(1 - d)``.
* :class:`NativeEMA` -- the native engine: the averaged parameters and BatchNorm statistics live in
  two flat buffers beside the model's, one HIP launch (``csrc/ema.hip``) updates both per step, and
  the same kernel run as an exchange puts them under the model for validation.
* :class:`ModelEMA` -- the same interface and arithmetic in plain torch (torch engine, CPU).
* :func:`build_ema` -- the run's EMA from ``MX_EMA`` / ``MX_EMA_EVERY`` / ``MX_EMA_WARMUP``, or None.

Every step updates the average, also one whose optimizer step AMP skipped on overflow (the weights
did not move; torchvision's training script does the same), so no device flag is read.
"""
from __future__ import annotations

import contextlib
import math
from collections import OrderedDict

import numpy as np
import torch

__all__ = ["ema_weight", "NativeEMA", "ModelEMA", "build_ema", "EMA_REFUSAL"]

EMA_REFUSAL = ("{what} cannot run MX_EMA: captured steps (MX_GRAPH=1, the DataParallel replica "
               "graphs) replay the launches recorded at capture, and the weight average is updated "
               "after the optimizer step outside them. Run without MX_GRAPH / on one device (the "
               "single-GPU and DDP scripts work), or drop MX_EMA")

_SCALARS = ("decay", "every", "warmup", "num_updates", "steps")


def ema_weight(decay: float, num_updates: int, warmup: bool = True) -> float:
    """``w`` of update number ``num_updates`` (0-based) in ``e += w * (p - e)``: a float32 value."""
    d = min(decay, (1.0 + num_updates) / (10.0 + num_updates)) if warmup else decay
    return float(np.float32(1.0 - d))


class _EMABase:
    def __init__(self, decay: float, every: int = 1, warmup: bool = True) -> None:
        decay, every = float(decay), int(every)
        if not (math.isfinite(decay) and 0.0 < decay < 1.0):
            raise ValueError(f"EMA decay lies in (0, 1), got {decay!r}")
        if every < 1:
            raise ValueError(f"EMA update interval is >= 1 step, got {every!r}")
        self.decay, self.every, self.warmup = decay, every, bool(warmup)
        self.steps = 0          # optimizer steps seen
        self.num_updates = 0    # updates applied (every `every`-th step)

    def update(self) -> None:
        """Call once per optimizer step."""
        self.steps += 1
        if self.steps % self.every:
            return
        self._lerp(ema_weight(self.decay, self.num_updates, self.warmup))
        self.num_updates += 1

    @contextlib.contextmanager
    def swapped(self):
        """Within the block the model computes with the averaged weights, statistics and counters
        (and the EMA holds the live ones); on exit both are back, bit for bit."""
        self._swap()
        try:
            yield
        finally:
            self._swap()

    def _tensors(self) -> "OrderedDict[str, torch.Tensor]":
        raise NotImplementedError

    def state_dict(self) -> dict:
        """The schedule's scalars and ``model``: the averaged weights under the model's (torchvision)
        keys and logical shapes, as references to the EMA's own storage."""
        sd = {k: getattr(self, k) for k in _SCALARS}
        sd["model"] = OrderedDict(self._tensors())
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        mine, theirs = self._tensors(), sd["model"]
        if set(mine) != set(theirs):
            raise KeyError(f"EMA state: missing keys {sorted(set(mine) - set(theirs))}, unexpected "
                           f"keys {sorted(set(theirs) - set(mine))}")
        for k, t in mine.items():
            if tuple(t.shape) != tuple(theirs[k].shape):
                raise ValueError(f"EMA state: {k} has shape {tuple(theirs[k].shape)}, the model's has "
                                 f"{tuple(t.shape)}")
            t.copy_(theirs[k])
        self.decay, self.every = float(sd["decay"]), int(sd["every"])
        self.warmup = bool(sd["warmup"])
        self.num_updates, self.steps = int(sd["num_updates"]), int(sd["steps"])


class NativeEMA(_EMABase):
    """EMA of a :class:`~pytorch_distributed_amd.models.native.NativeResNet`: ``ema_params`` follows
    ``flat_params`` and ``ema_bufstore`` follows ``flat_bufstore`` (running mean / var, then the
    ``num_batches_tracked`` counters). ``update()`` is one launch over (parameters, statistics) and
    a copy of the counters: no host synchronisation, no allocation."""

    def __init__(self, model, decay: float, every: int = 1, warmup: bool = True) -> None:
        super().__init__(decay, every, warmup)
        from .ops import native_ops as K
        self._K = K
        self.model = model
        self.ema_params = torch.empty_like(model.flat_params)
        self.ema_bufstore = torch.empty_like(model.flat_bufstore)
        nb = model.flat_buffers.numel()
        self.ema_buffers = self.ema_bufstore[:nb * 4].view(torch.float32)
        self.ema_nbt = self.ema_bufstore[nb * 4:].view(torch.int64)
        # the exchange and the first copy move the whole buffer store as 32-bit words, counters
        # included; the average runs over the f32 statistics only
        shadow = None if model.f32 else model.flat_shadow
        self._whole = K.EmaRanges([(self.ema_params, model.flat_params, shadow),
                                   (self.ema_bufstore.view(torch.float32),
                                    model.flat_bufstore.view(torch.float32))])
        self._floats = K.EmaRanges([(self.ema_params, model.flat_params),
                                    (self.ema_buffers, model.flat_buffers)])
        K.ema_update(self._whole, K.EMA_COPY)
        self._views = None

    def _lerp(self, w: float) -> None:
        self._K.ema_update(self._floats, self._K.EMA_LERP, w)
        self.ema_nbt.copy_(self.model.flat_nbt)

    def _swap(self) -> None:
        # one launch: parameters, statistics and counters change places and the 16-bit shadow of the
        # parameters now under the model is written; the packed stem weights follow them
        self._K.ema_update(self._whole, self._K.EMA_SWAP)
        self.model._pack_stem()

    def _tensors(self):
        """The model's state-dict entries re-pointed into the EMA's storage: same keys, shapes,
        strides and offsets (conv weights are OIHW views of channels-last storage, as the model's)."""
        if self._views is None:
            m = self.model
            stores = {m.flat_params.untyped_storage().data_ptr(): self.ema_params,
                      m.flat_bufstore.untyped_storage().data_ptr(): self.ema_bufstore}
            views = OrderedDict()
            for k, t in m.state_dict().items():
                mine = stores.get(t.untyped_storage().data_ptr())
                if mine is None:
                    raise RuntimeError(f"NativeEMA: {k} lies outside the model's flat buffers")
                views[k] = torch.empty(0, dtype=t.dtype, device=t.device).set_(
                    mine.untyped_storage(), t.storage_offset(), t.size(), t.stride())
            self._views = views
        return self._views


class ModelEMA(_EMABase):
    """EMA of any ``nn.Module`` in plain torch: floating-point parameters and buffers are averaged
    with the same float32 ``w`` as the kernel uses (``e += w * (p - e)``), integer buffers copied."""

    def __init__(self, module, decay: float, every: int = 1, warmup: bool = True) -> None:
        super().__init__(decay, every, warmup)
        self.module = module
        self.ema = OrderedDict((k, v.detach().clone()) for k, v in module.state_dict().items())

    @torch.no_grad()
    def _lerp(self, w: float) -> None:
        live = self.module.state_dict()
        for k, e in self.ema.items():
            if e.is_floating_point():
                e.add_(live[k].detach() - e, alpha=w)
            else:
                e.copy_(live[k])

    @torch.no_grad()
    def _swap(self) -> None:
        live = self.module.state_dict()
        for k, e in self.ema.items():
            p = live[k].detach()
            keep = p.clone()
            p.copy_(e)
            e.copy_(keep)

    def _tensors(self):
        return self.ema


def build_ema(cfg, model, ctx):
    """The run's EMA (``MX_EMA`` > 0), built from the model as it stands (after a resume has loaded
    it): :class:`NativeEMA` on the native engine, else :class:`ModelEMA`; None when off. Captured
    steps -- ``MX_GRAPH=1``, DataParallel over several devices or with ``PDA_DP_FORCE_REPLAY=1`` --
    are refused with a ValueError."""
    if not cfg.ema > 0:
        return None
    if cfg.graph and ctx.engine == "native":
        raise ValueError(EMA_REFUSAL.format(what="MX_GRAPH=1"))
    from .runtime.graphs import DP_REPLAY, replays_captured_steps
    if replays_captured_steps(model):
        raise ValueError(EMA_REFUSAL.format(what=DP_REPLAY))
    inner = getattr(model, "module", model)
    cls = NativeEMA if hasattr(inner, "flat_params") else ModelEMA
    return cls(inner, cfg.ema, every=cfg.ema_every, warmup=cfg.ema_warmup)
