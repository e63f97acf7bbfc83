"""Loss, optimizer and bench trainer of the native engine (``models/native.py``): the fused
cross-entropy nodes, the flat-buffer SGD and the trainer ``bench.py`` drives. None of them knows the
forward / backward schedule; the loss hands its 16-bit d(loss)/d(logits) to the network through
``NativeResNet._pending_dlog16``."""
from __future__ import annotations

from typing import TYPE_CHECKING, Optional

import torch
from torch import nn

from ..ops import native_ops as K

if TYPE_CHECKING:
    from .native import NativeResNet

__all__ = ["NativeSGD", "NativeCrossEntropy", "NativeTrainer"]


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, model: NativeResNet):
        B = logits.shape[0]
        loss_rows = torch.empty(B, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        K.xent(logits, labels, loss_rows, loss)
        ctx.save_for_backward(logits, labels)
        ctx.model = model
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels = ctx.saved_tensors
        m: NativeResNet = ctx.model
        B = logits.shape[0]
        dlog16 = torch.empty(B, m.fc_rows, dtype=m.dtype, device=logits.device)
        gdev = g.reshape(1).to(torch.float32).contiguous()
        K.xent(logits, labels, torch.empty(B, device=logits.device), None, dlog=dlog16,
               gscale=1.0 / B, gdev=gdev)
        m._pending_dlog16 = dlog16
        # the dlogits handed to the network node are carried by dlog16; return a placeholder
        return torch.empty_like(logits), None, None


class _XentSoftFn(torch.autograd.Function):
    """:class:`_XentFn` against the soft target of two labels per row (K.xent_soft)."""

    @staticmethod
    def forward(ctx, logits, labels, labels_b, lam, eps, model: NativeResNet):
        B = logits.shape[0]
        loss_rows = torch.empty(B, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        K.xent_soft(logits, labels, loss_rows, loss, labels_b=labels_b, lam=lam, eps=eps)
        ctx.save_for_backward(logits, labels, *(() if labels_b is None else (labels_b,)))
        ctx.model, ctx.lam, ctx.eps = model, lam, eps
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, *rest = ctx.saved_tensors
        m: NativeResNet = ctx.model
        B = logits.shape[0]
        dlog16 = torch.empty(B, m.fc_rows, dtype=m.dtype, device=logits.device)
        gdev = g.reshape(1).to(torch.float32).contiguous()
        K.xent_soft(logits, labels, torch.empty(B, device=logits.device), None,
                    labels_b=rest[0] if rest else None, lam=ctx.lam, eps=ctx.eps, dlog=dlog16,
                    gscale=1.0 / B, gdev=gdev)
        m._pending_dlog16 = dlog16
        return torch.empty_like(logits), None, None, None, None, None


class NativeCrossEntropy(nn.Module):
    """CrossEntropyLoss (mean) fused with its gradient kernel for the native engine.
    ``label_smoothing`` (eps) and a second label per row with its weight (``labels_b``, ``lam``:
    mixup / CutMix) select the soft-target kernel; with neither, the hard-label kernel runs."""

    soft_targets = True      # forward takes (logits, labels, labels_b, lam): trainer.build_criterion

    def __init__(self, model: Optional[NativeResNet] = None, label_smoothing: float = 0.0) -> None:
        super().__init__()
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing!r}")
        self.model = model
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor,
                labels_b: Optional[torch.Tensor] = None, lam: float = 1.0) -> torch.Tensor:
        m = self.model
        eps = self.label_smoothing
        if m is None or not logits.is_cuda or logits.dtype != torch.float32:
            x = logits.float()
            if eps == 0.0 and labels_b is None:
                return nn.functional.cross_entropy(x, labels)
            from ..mix import soft_cross_entropy
            return soft_cross_entropy(x, labels, labels_b, lam, eps)
        if eps == 0.0 and labels_b is None:
            if logits.requires_grad:
                return _XentFn.apply(logits, labels, m)
            B = logits.shape[0]
            loss = torch.empty((), dtype=torch.float32, device=logits.device)
            K.xent(logits.contiguous(), labels, torch.empty(B, device=logits.device), loss)
            return loss
        lam = float(lam)
        if logits.requires_grad:
            return _XentSoftFn.apply(logits, labels, labels_b, lam, eps, m)
        B = logits.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        K.xent_soft(logits.contiguous(), labels, torch.empty(B, device=logits.device), loss,
                    labels_b=labels_b, lam=lam, eps=eps)
        return loss


class NativeSGD(torch.optim.Optimizer):
    """torch.optim.SGD semantics (momentum, dampening 0, weight decay on every parameter -- as the
    reference, quirk Q12) executed as ONE fused kernel over the flat buffers, which also refreshes
    the 16-bit weight shadow. ``state_dict()`` has torch SGD's format (per-parameter
    ``momentum_buffer``), so checkpoints interchange with the reference's optimizer.

    ``param_groups`` (torch-style group dicts: ``params`` plus any of ``lr``, ``momentum``,
    ``weight_decay``, ``nesterov``, ``lars``, ``lars_eps``; the constructor arguments are the
    defaults), ``nesterov=True`` or a trust coefficient ``lars > 0`` select the *segmented* step
    (``self.segmented``): one ``sgd_seg`` launch (``csrc/optim.hip``) that reads each parameter
    tensor's hyper-parameters from a device table, after a ``seg_norms`` launch when some group has a
    trust coefficient. Parameters given to no group are frozen: their master weights, momentum and
    shadow are never touched. The groups' hyper-parameters may change between steps (``StepLR``); the
    table is re-uploaded when they do. Without these arguments the optimizer is the one-launch
    ``sgd_flat`` step, unchanged.

    ``clip_grad_norm > 0`` clips the gradient by its global L2 norm
    (``torch.nn.utils.clip_grad_norm_``) over every parameter of the groups, on the device: one
    ``grad_clip`` launch (``csrc/clip.hip``) ahead of the update publishes the norm and the
    coefficient, already multiplied by AMP's 1/scale, and the SGD launch takes that scalar as its
    gradient scale -- no host sync, no second pass over the gradient. ``grad_norm`` is the
    one-element device tensor holding the unscaled pre-clip norm of the last step that ran. The
    clip keeps no state of its own. With 0 (the default) none of this exists."""

    @staticmethod
    def wants_segments(param_groups=None, nesterov=False, lars=0.0, **_kw) -> bool:
        """Whether these constructor arguments select the segmented step."""
        return param_groups is not None or bool(nesterov) or lars != 0

    def __init__(self, model: NativeResNet, lr=0.1, momentum=0.9, weight_decay=1e-4,
                 dampening=0.0, nesterov=False, lars=0.0, lars_eps=1e-8, param_groups=None,
                 clip_grad_norm=0.0) -> None:
        self._sealed = False
        if (not isinstance(clip_grad_norm, (int, float)) or isinstance(clip_grad_norm, bool)
                or not clip_grad_norm >= 0 or clip_grad_norm == float("inf")):
            raise ValueError(f"NativeSGD: clip_grad_norm is a finite maximum norm >= 0 (0 = off), "
                             f"got {clip_grad_norm!r}")
        self.clip_grad_norm = float(clip_grad_norm)
        self.segmented = self.wants_segments(param_groups, nesterov, lars)
        if dampening != 0.0:
            raise ValueError("NativeSGD implements dampening=0 (reference setting)")
        defaults = dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay,
                        nesterov=False, maximize=False, foreach=None, differentiable=False,
                        fused=None)
        if self.segmented:
            from ..optim import normalize_param_groups
            defaults.update(nesterov=bool(nesterov), lars=lars, lars_eps=lars_eps)
            groups = normalize_param_groups(list(model.parameters()), param_groups, defaults)
            if not any(g["params"] for g in groups):
                raise ValueError("NativeSGD: the parameter groups hold no parameter")
            super().__init__(groups, defaults)
        else:
            super().__init__(list(model.parameters()), defaults)
        self._sealed = True
        self.model = model
        self.flat_mom = torch.zeros_like(model.flat_params)
        self._initialized = False
        self._amp_ws = None    # step_amp's scan counters and 1/scale, allocated on its device
        self._amp_inv = None
        # per-parameter momentum views (torch format in state_dict)
        self._views = {}
        fp = model.flat_params
        base = fp.data_ptr()
        segments = []
        for g in self.param_groups:
            for p in g["params"]:
                off = (p.data_ptr() - base) // 4
                segments.append((off, p.numel()))
                v = self.flat_mom[off:off + p.numel()]
                if p.dim() == 4:
                    O, I, R, S_ = p.shape
                    v = v.view(O, R, S_, I).permute(0, 3, 1, 2)
                else:
                    v = v.view(p.shape)
                self._views[p] = v
        if self.segmented:
            # one segment per parameter tensor (the fc weight: its num_classes rows, not the padded
            # ones), in group order; the device table is built once and re-uploaded on a change
            self._uploaded = self._hyper_rows()
            self._tables, _ = K.seg_tables(segments, self._uploaded, fp.device)
        self.grad_norm = None
        if self.clip_grad_norm > 0:
            # every buffer of the clip launch, once: step() allocates nothing. The segmented step's
            # block table covers the same tensors; the flat step gets one of its own
            self._clip_tables = (self._tables if self.segmented else
                                 K.seg_tables(segments, [{"lr": 0.0}] * len(segments), fp.device)[0])
            self._clip_slab = torch.zeros(self._clip_tables.nblocks, dtype=torch.float64,
                                          device=fp.device)
            self._clip_cnt = torch.zeros(1, dtype=torch.int32, device=fp.device)
            self._clip_out = torch.zeros(2, dtype=torch.float32, device=fp.device)
            self.grad_norm = self._clip_out[0:1]

    def add_param_group(self, param_group) -> None:
        if getattr(self, "_sealed", False):
            raise ValueError("NativeSGD: the groups are fixed at construction (the segment table is "
                             "built once); pass param_groups to the constructor")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.model.zero_grad_flat()

    def _hyper_rows(self) -> list:
        """One hyper-parameter row per segment, from the groups as they are now."""
        from ..optim import GROUP_KEYS, check_hyper
        rows = []
        for i, g in enumerate(self.param_groups):
            h = {k: g[k] for k in GROUP_KEYS}
            check_hyper(h, f"NativeSGD: param_groups[{i}]: ")
            rows += [h] * len(g["params"])
        return rows

    def _launch_segments(self, inv_scale=None, found_inf=None) -> None:
        m = self.model
        rows = self._hyper_rows()
        if rows != self._uploaded:      # a scheduler (or the user) edited a group since the last step
            self._tables.set_hyper(rows)
            self._uploaded = rows
        if self._tables.any_trust:
            K.seg_norms(m.flat_params, m.flat_grad, self._tables)
        K.sgd_seg(m.flat_params, m.flat_grad, self.flat_mom, None if m.f32 else m.flat_shadow,
                  self._tables, self._initialized, inv_scale=inv_scale, found_inf=found_inf)

    def _launch_range(self, lo: int, hi: int, inv_scale=None, found_inf=None) -> None:
        g = self.param_groups[0]
        m = self.model
        K.sgd_flat(m.flat_params[lo:hi], m.flat_grad[lo:hi], self.flat_mom[lo:hi],
                   None if m.f32 else m.flat_shadow[lo:hi], g["lr"], g["momentum"],
                   g["weight_decay"], self._initialized, inv_scale=inv_scale, found_inf=found_inf)

    def _launch(self, inv_scale=None, found_inf=None) -> None:
        m = self.model
        if m._grads_zero:
            # zero_grad() and no backward since: torch 2.x's set_to_none leaves every .grad None,
            # and SGD skips parameters without a gradient -- the flat gradient still holds the
            # previous step's values (no memset), so applying it would be a stale update
            return
        if self.clip_grad_norm > 0:
            # norm and coefficient on the device; the update unscales AND clips by out[1]
            K.grad_clip(m.flat_grad, self._clip_tables, self.clip_grad_norm, self._clip_slab,
                        self._clip_cnt, self._clip_out, inv_scale=inv_scale, found_inf=found_inf)
            inv_scale = self._clip_out[1:2]
        if self.segmented:
            self._launch_segments(inv_scale, found_inf)
        else:
            self._launch_range(0, m.numel, inv_scale, found_inf)
        m._pack_stem()
        # (an overflow-skipped first step leaves the momentum buffer unset on the device but the
        # flag set: the next step then reads the zero-initialised buffer, m*0 + d == d)
        self._initialized = True
        for g in self.param_groups:
            for p in g["params"]:
                self.state[p]["momentum_buffer"] = self._views[p]

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._launch()
        return loss

    @torch.no_grad()
    def step_amp(self, scale: torch.Tensor, found_inf: torch.Tensor, tracker=None,
                 growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000) -> None:
        """AMP step, two launches and no host sync: ``amp_scan`` (non-finite check of the flat
        gradient; its last workgroup publishes found_inf and 1/scale and, given ``tracker``, runs
        the GradScaler scale update) then the fused SGD, which unscales by 1/scale and skips the
        whole update when found_inf is set."""
        if self._amp_ws is None or self._amp_ws.device != scale.device:
            self._amp_ws = torch.zeros(2, dtype=torch.int32, device=scale.device)
            self._amp_inv = torch.ones(1, dtype=torch.float32, device=scale.device)
        K.amp_scan(self.model.flat_grad, found_inf, self._amp_inv, scale, tracker, self._amp_ws,
                   growth_factor, backoff_factor, growth_interval)
        self._launch(inv_scale=self._amp_inv, found_inf=found_inf)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self.segmented:
            # a checkpoint of a plain torch.optim.SGD carries no lars / lars_eps: keep the defaults
            for g in self.param_groups:
                for k, v in self.defaults.items():
                    g.setdefault(k, v)
        with torch.no_grad():
            any_buf = False
            for g in self.param_groups:
                for p in g["params"]:
                    st = self.state.get(p, {})
                    buf = st.get("momentum_buffer")
                    if buf is not None:
                        self._views[p].copy_(buf)
                        st["momentum_buffer"] = self._views[p]
                        any_buf = True
            self._initialized = any_buf


# ------------------------------------------------------------------ bench trainer
class NativeTrainer:
    engine = "native"

    def __init__(self, arch, batch, dtype, device, world=1, rank=0, bucket_mb=32.0, image_size=224,
                 graph: bool = False):
        from .native import NativeResNet
        from .resnet import build_model
        from ..data.synthetic import SyntheticImageNet
        torch.manual_seed(0)
        ref = build_model(arch)
        self.model = NativeResNet(ref, device=device, dtype=dtype, image_size=image_size)
        self.net = self.model
        if world > 1:
            from ..parallel.ddp import DistributedDataParallel
            self.net = DistributedDataParallel(self.model, bucket_cap_mb=bucket_mb)
        self.opt = self.model.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4)
        self.crit = self.model.make_criterion()
        self.ds = SyntheticImageNet("train", seed=0, image_size=image_size)
        self.gen = self.model.input_generator(self.ds)
        self.batch, self.world, self.rank, self.device = batch, world, rank, device
        self.scaler = None
        if dtype == torch.float16:
            from ..amp import LossScaler
            self.scaler = LossScaler()
        self._loss = None
        self.graphed = None
        if graph:
            from ..runtime.graphs import graphs_unsafe_warning, single_queue_graphs
            if not single_queue_graphs():
                graphs_unsafe_warning("NativeTrainer(graph=True)")
                graph = False
        if graph:
            if world > 1:
                raise ValueError("graph capture of the distributed step is not enabled (RCCL "
                                 "collectives stay eager); use graph=False with world > 1")
            from ..runtime.graphs import GraphedNativeStep
            self.graphed = GraphedNativeStep(self.model, self.opt, self.gen, batch, self.scaler,
                                             device)

    def step(self, i: int) -> None:
        if self.graphed is not None:
            self.graphed.run((i * self.world + self.rank) * self.batch)
            self._loss = self.graphed.loss
            return
        ids = torch.arange(self.batch, dtype=torch.int64) + (i * self.world + self.rank) * self.batch
        x, y = self.gen(ids)
        out = self.net(x)
        loss = self.crit(out, y)
        if self.scaler is not None:
            self.scaler.scale(loss).backward()
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            loss.backward()
            self.opt.step()
        self.opt.zero_grad()
        self._loss = loss.detach()

    def last_loss(self):
        return None if self._loss is None else float(self._loss.item())

    def state_checksum(self) -> torch.Tensor:
        """Bit-exact checksum of master weights + momentum (bench cross-rank consistency)."""
        from ..bench_step import tensor_checksum
        return tensor_checksum([self.model.flat_params, self.opt.flat_mom])
