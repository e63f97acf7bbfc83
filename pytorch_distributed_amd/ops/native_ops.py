"""Op-level Python API over the gfx950 kernels (torch tensors in, torch tensors out).

Layout conventions: activations are NHWC 16-bit (bf16 or f16) tensors of shape
``[N, H, W, C]``; conv weights are 16-bit OHWI ``[Cout, R, S, Cin]`` (the stem
uses a packed ``[64, 448]`` image, see :func:`pack_stem`); statistics, BN
parameters, gradients and the optimizer state are f32.

These functions are what the native ResNet engine
(:mod:`pytorch_distributed_amd.models.native`) schedules, and what the GPU
numerics tests compare against plain PyTorch fp32 references.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import ext
from .ext import BlkRow, BwdArgs, ConvDesc, EmaRange, SegRow, check, dt_of, ptr, stream

__all__ = [
    "ConvGeom", "conv_fwd", "conv_dgrad", "conv_wgrad", "pick_tile", "fwd_tile", "wgrad_plan",
    "BnStats", "stats_totals", "bn_finalize_tot", "bn_finalize_partials", "bn_eval_coeffs",
    "bn_apply", "stem_pool", "maxpool_bwd", "tail_pool", "bn_epilogue", "bn_bwd_finish",
    "bn_bwd", "xent", "topk_hits", "col_sum", "sgd_flat", "cast_flat", "amp_scan",
    "pack_stem", "synth_batch", "Workspace", "aug_check", "aug_resize",
    "aug_draw", "aug_resize_dev", "aug_record_bytes", "batch_layout", "batch_shape",
    "FLAT_CHUNK", "SEG_CHUNK", "SegTables", "seg_tables", "seg_norms", "sgd_seg", "grad_clip",
    "xent_soft", "xent_soft_check", "batch_mix", "batch_mix_check", "mix_weights",
    "erase_draw", "erase_bounds", "batch_erase", "batch_erase_check",
]


@dataclass(frozen=True)
class ConvGeom:
    Nb: int
    H: int
    W: int
    Cin: int     # channels of the stored input (stem: 16, the 2x2 space-to-depth image)
    Cout: int
    R: int
    S: int
    stride: int
    pad: int
    ho: Optional[int] = None   # explicit output size (asymmetric-padding forms, e.g. the s2d stem)
    wo: Optional[int] = None

    @property
    def Ho(self) -> int:
        return self.ho if self.ho is not None else (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def Wo(self) -> int:
        return self.wo if self.wo is not None else (self.W + 2 * self.pad - self.S) // self.stride + 1

    def desc(self, Nb: Optional[int] = None) -> ConvDesc:
        return ConvDesc(self.Nb if Nb is None else Nb, self.H, self.W, self.Cin, self.Cout, self.R,
                        self.S, self.stride, self.pad, self.Ho, self.Wo)

    def with_batch(self, Nb: int) -> "ConvGeom":
        return ConvGeom(Nb, self.H, self.W, self.Cin, self.Cout, self.R, self.S, self.stride, self.pad,
                        self.ho, self.wo)


class ReduceBatch:
    """Split-K reductions queued instead of launched one by one (:func:`conv_wgrad` on a
    :class:`Workspace` whose ``reduce_batch`` is set): each queued weight gradient gets a slab of its
    own, and :meth:`flush` reduces all of them in ONE launch (csrc/conv_gemm.hip
    wgrad_reduce_batch_kernel: the same fixed-order sums, deterministic). The owner flushes on the
    stream the weight gradients ran on, before anything reads the gradients."""

    MAX = 24

    def __init__(self, ws: "Workspace") -> None:
        self.ws = ws
        self.items = []
        self._keep = []

    def slab(self, numel: int) -> torch.Tensor:
        if len(self.items) >= self.MAX:
            self.flush()
        return self.ws.get(f"wgrad_slab_b{len(self.items)}", numel)

    def add(self, slab, grad, splits, M, N, cin_log2, cin_real, pitch, scale, accumulate,
            ck=None, cB=None, cs=None) -> None:
        self.items.append(ext.RedDescC(ptr(slab), ptr(grad), ptr(ck), ptr(cB), ptr(cs), splits, M, N,
                                       cin_log2, cin_real, pitch, int(accumulate), float(scale)))
        self._keep.extend(t for t in (ck, cB, cs) if t is not None)

    def flush(self) -> None:
        if not self.items:
            return
        arr = (ext.RedDescC * len(self.items))(*self.items)
        check(ext.lib().pda_wgrad_reduce_batch(arr, len(self.items), stream(self.ws.device)),
              "wgrad_reduce_batch")
        self.items = []
        self._keep = []


class Workspace:
    """Grow-only scratch buffers (split-K slabs, BN partials) reused by every layer on a stream.

    ``sync_comm``: when set (SyncBatchNorm, :func:`~pytorch_distributed_amd.parallel.ddp.
    convert_sync_batchnorm`), every BatchNorm finalize of this workspace first all-reduces its
    per-channel sums over the communicator, so statistics and their gradients are global."""

    def __init__(self, device) -> None:
        self.device = device
        self._bufs = {}
        self._retired = []   # outgrown buffers stay allocated: a captured HIP graph may use them
        self.sync_comm = None
        self.reduce_batch: Optional[ReduceBatch] = None   # set: conv_wgrad queues its reduce

    @property
    def local_stats(self) -> bool:
        """BatchNorm statistics are per rank: no SyncBatchNorm, or a communicator of one rank."""
        return self.sync_comm is None or self.sync_comm.world_size == 1

    def get(self, name: str, numel: int, dtype=torch.float32) -> torch.Tensor:
        b = self._bufs.get(name)
        if b is None or b.numel() < numel or b.dtype != dtype:
            if b is not None:
                self._retired.append(b)
            b = torch.empty(max(numel, 1), dtype=dtype, device=self.device)
            self._bufs[name] = b
        return b[:numel]

    def counters(self, numel: int, name: str = "_counters") -> torch.Tensor:
        """int32 arrival counters of the one-launch reduction kernels: zero when allocated, and
        every kernel that uses them leaves them zero again (its last arrivers reset them). One
        ``name`` per kernel family that may run concurrently with another on the stream."""
        b = self._bufs.get(name)
        if b is None or b.numel() < numel:
            if b is not None:
                self._retired.append(b)
            b = torch.zeros(max(numel, 64), dtype=torch.int32, device=self.device)
            self._bufs[name] = b
        return b[:numel]


_NUM_CU = 256
_WGRAD_TARGET = 2 * _NUM_CU   # default split-K block target of the weight gradients
# every weight-gradient block target x 0.7 in the step: the targets above were tuned per kernel in
# isolation, but a weight gradient shares the device with the main-stream chain, and fewer,
# longer split-K blocks leave it more CUs (bench.py, 5 alternating rounds on one box: x1.0 28.20,
# x0.85 28.15, x0.7 28.04, x0.6 28.11, x0.4 28.24, x1.5 28.34 ms/step; profiles/ab_r3_dma.md)
_WGRAD_SCALE = float(os.environ.get("PDA_WGRAD_SCALE", "0.7"))


# f32 convolutions: "split" (default) = f32 tensors with the products on the bf16 MFMA as a
# three-term hi/lo split (DT_F32S, ~16 significant bits per product: every ResNet-50 conv pass at
# or below the error of TF32 convolutions -- the reference's fp32 runs on A100 -- against float64,
# tests/test_f32_precision_gpu.py; 1.6x the exact path); "exact" = MFMA 16x16x4 f32 (DT_F32, f32
# rounding only; csrc/common.h DType)
_F32_CONV = os.environ.get("PDA_F32_CONV", os.environ.get("MX_F32_CONV", "split"))
if _F32_CONV not in ("exact", "split"):
    raise ValueError(f"MX_F32_CONV / PDA_F32_CONV must be exact|split, got {_F32_CONV!r}")
_SPLIT_BN = 128      # widest N tile of the split kernels
_STEM_G = 4096       # block cap of the one-pass stem backward (profiles/ab_r2_inlaunch_bn.md)
# downsample-tail BN backward: both branches' apply in one pass over dz (False: two launches, kept
# for tests/test_native_model_gpu.py's bitwise parity test of the two forms)
_BWD_APPLY2 = True


def _kdt(t: torch.Tensor) -> int:
    """Kernel dtype code of a conv launch on tensor ``t`` (see _F32_CONV)."""
    d = dt_of(t)
    return 3 if d == 0 and _F32_CONV == "split" else d


def tile_rows(bm: int) -> int:
    """M rows of a tile code: -bm = single-stage register-staged, bm > 1000 = the LDS-DMA 8-wave
    variant of (bm - 1000) rows, bm > 2000 = its tap-reuse form for 3x3 stride-1 fwd / dgrad
    (csrc/conv_gemm.hip dispatch)."""
    return bm - 2000 if bm > 2000 else bm - 1000 if bm > 1000 else abs(bm)


def _ktile(bm: int, bn: int, kdt: int, pro: bool = False) -> Tuple[int, int]:
    """The tile a launch actually uses. The LDS-DMA tiles (bm > 1000) are 16-bit only and cannot
    apply an operand prologue (the bytes never pass through registers): those launches fall back
    to the register-staged 128-row tile. The split-f32 kernels stage hi + lo tiles: single-stage
    tiles of at most 128 x 128."""
    if bm > 1000 and (kdt not in (1, 2) or pro):   # (the HALO tiles too)
        bm, bn = -128, min(bn, 128)
    if kdt != 3:
        return bm, bn
    return -min(abs(bm), 128), min(bn, _SPLIT_BN)


def pick_tile(M: int, N: int, K: Optional[int] = None, dma: bool = False) -> Tuple[int, int]:
    """(bm, bn) for an implicit GEMM; a negative bm selects the single-LDS-buffer variant: half the
    LDS admits a third resident block per CU, which hides the global-load latency better than
    double buffering does at two blocks per CU (measured on all 23 ResNet-50 shapes). ``dma``
    (forward launches): the LDS-DMA 128x256 tile where it measured faster -- deep K (>= 1024) and
    >= 256 output channels with enough tiles for every CU (profiles/convbench_r3_dma.txt: C12 C16
    C17 C18 C20 C22, 4-9 %); the launch falls back to the 128-row register tile when the operand
    needs the BN prologue or is not 16-bit (:func:`_ktile`)."""
    if (dma and _DMA and K is not None and K >= 1024 and N >= 256 and N % 256 == 0
            and math.ceil(M / 128) * (N // 256) >= _NUM_CU):
        return 1128, 256
    bn = 64 if N <= 64 else 128
    bm = 128
    if math.ceil(M / 128) * math.ceil(N / bn) < 2 * _NUM_CU:
        bm = 64
    if bm == 128:
        bm = -128     # single-stage: measured faster on every ResNet-50 shape (tools/conv_bench.py)
    return bm, bn


# ------------------------------------------------------------------ conv
class BnStats:
    """BatchNorm (training) statistics of a conv forward: the conv epilogue writes per-M-tile
    shifted partial sums, which ONE follow-up launch (:func:`bn_finalize_partials`) combines in f64
    and finalizes into mean / invstd / scale / shift and the running statistics. (Finalizing inside
    the conv launch itself measured slower: the finalize code costs the conv epilogue ~2% even when
    idle -- profiles/ab_r2_inlaunch_bn.md.) With SyncBatchNorm (``ws.sync_comm``) the launch stops
    at f64 totals, all-reduced before a small finalize kernel."""

    def __init__(self, ws: "Workspace", gamma, beta, eps: float, momentum: float, mean, invstd,
                 scale, shift, rmean=None, rvar=None, nbt=None, update_running: bool = True):
        self.ws, self.gamma, self.beta = ws, gamma, beta
        self.eps, self.momentum = float(eps), float(momentum)
        self.mean, self.invstd, self.scale, self.shift = mean, invstd, scale, shift
        self.rmean, self.rvar, self.nbt, self.update = rmean, rvar, nbt, update_running


def fwd_tile(g: ConvGeom, Nb: int, dtype: torch.dtype, pro: bool = False,
             Kpad: Optional[int] = None) -> Tuple[int, int]:
    """Default tile of a forward conv. The LDS-DMA tiles take 16-bit operands without the BN
    prologue (their bytes never pass through registers): tap reuse (HALO) on the 3x3 stride-1
    layers with >= 128 output channels (C10 118 -> 105 us, C16 114 -> 98, C22 127 -> 109); other
    launches keep the register-staged choice."""
    dma = _kdt(torch.empty(0, dtype=dtype)) in (1, 2) and not pro and g.Cin >= 64
    if dma and _DMA and _halo_geom(g) and g.Cout >= 128:
        return 2256, 128
    M = Nb * g.Ho * g.Wo
    # (the 128x256 LDS-DMA tile wins 4-9 % per kernel on the deep-K layers but loses in the step:
    # 28.65 -> 28.52 ms/step without it, profiles/ab_r3_dma.md section 12; explicit tile only)
    return pick_tile(M, g.Cout, Kpad if Kpad is not None else g.R * g.S * g.Cin)


def _launch_fwd(launch, what: str, T: int, rows: int, M: int, Cout: int, stats, bn, before_finalize):
    """What the three forward launches share: the workspace's statistics buffer (T tiles of ``rows``
    rows of M) when ``bn`` is given, ``launch(stats)`` -> rc, ``before_finalize``, the BN finalize."""
    if bn is not None:
        stats = bn.ws.get("fwd_stats", T * 3 * Cout)
    check(launch(stats), what)
    if before_finalize is not None:
        before_finalize()
    if bn is not None:
        bn_finalize_partials(stats, T, Cout, rows, M, bn)


def conv_fwd(x: torch.Tensor, w: torch.Tensor, g: ConvGeom, out: torch.Tensor,
             stats: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
             relu: bool = False, tile: Optional[Tuple[int, int]] = None,
             pro: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
             bn: Optional[BnStats] = None, before_finalize=None,
             tail: Optional["TailIn"] = None) -> torch.Tensor:
    """out[M, Cout] (16-bit or f32) = conv(x, w). w: [Cout, Kpad] 16-bit, Kpad = w.shape[1].
    stats (f32, >= ceil(M/bm)*3*Cout) receives per-M-tile shifted partials (sum(y-s),
    sum((y-s)^2), s) -- see :func:`stats_totals`; ``bn`` (:class:`BnStats`) also finalizes the
    BatchNorm from them. pro = (scale, shift): x is a PRE-BatchNorm tensor and the conv consumes
    relu(x*scale+shift). ``tail`` (:class:`TailIn`, 1x1 stride-1 convs, see :func:`tail_fuse_ok`):
    x is the previous block's pre-BN tail y3 and the conv consumes a = relu(bn3(y3) + r), writing a
    (and its ReLU bitmask) on the way -- the tail's BN-apply pass folded into its consumer."""
    if tail is not None:
        return _conv_fwd_tail(x, w, g, out, pro, tail, stats, bn, before_finalize)
    Nb = x.shape[0]
    M = Nb * g.Ho * g.Wo
    Kpad = w.shape[-1] if w.dim() == 2 else w[0].numel()
    dense = (tile is None and bias is None and not relu and out.dtype == x.dtype
             and x.is_contiguous() and out.is_contiguous() and w.is_contiguous()
             and x.numel() == Nb * g.H * g.W * g.Cin and out.numel() == M * g.Cout)
    # (the stem kernel writes one statistics partial per output ROW, not per fwd_tile M-tile: a
    # caller-sized ``stats`` buffer without ``bn`` keeps the generic tile's layout)
    if dense and pro is None and Kpad == 256 and (stats is None or bn is not None) \
            and stem_fwd_ok(g, x.dtype):
        return stem_fwd(x, w, g, out, stats, bn, before_finalize)
    bm, bn_ = tile or fwd_tile(g, Nb, x.dtype, pro is not None, Kpad)
    d = g.desc(Nb)
    # direct (unstaged) f32 store + bias: the fc head (16-bit features -> f32 logits, or any conv
    # with a bias); f32 activations of the exact-fp32 engine take the staged path with statistics
    out_f32 = bias is not None or out.dtype != x.dtype
    pitch = out.stride(0) if out.dim() == 2 else g.Cout
    kdt = _kdt(x)
    kbm, kbn = _ktile(bm, bn_, kdt, pro is not None or g.Cin < 64)
    _launch_fwd(lambda st: ext.lib().pda_conv_fwd(
        C.byref(d), ptr(x), ptr(w), Kpad, ptr(out), int(out_f32), pitch, ptr(bias), ptr(st),
        int(relu), ptr(pro[0] if pro else None), ptr(pro[1] if pro else None), kdt, kbm, kbn,
        stream(x.device)),
        "conv_fwd", math.ceil(M / tile_rows(kbm)), tile_rows(kbm), M, g.Cout, stats, bn,
        before_finalize)
    return out


@dataclass
class TailIn:
    """Operands of a residual block's tail a = relu(y3 * sc + sh + r) formed by the consumer conv
    (conv_fwd ``tail``): ``res`` is r itself (identity shortcut) or, with ``sc2`` / ``sh2``, the
    downsample branch's pre-BN output whose BN is applied too; ``out`` receives a, ``mask`` (uint8,
    numel / 8, identity tails) its ReLU bitmask -- exactly what :func:`bn_apply` would write."""
    res: torch.Tensor
    out: torch.Tensor
    mask: Optional[torch.Tensor] = None
    sc2: Optional[torch.Tensor] = None
    sh2: Optional[torch.Tensor] = None


def tail_fuse_ok(g: ConvGeom, dtype: torch.dtype) -> bool:
    """Whether a tail can be folded into this consumer conv (csrc/conv_gemm.hip FWD_TAIL): a 1x1
    stride-1 conv without padding on 16-bit operands, Cin a multiple of 64."""
    return (dtype in (torch.bfloat16, torch.float16) and g.R == 1 and g.S == 1 and g.stride == 1
            and g.pad == 0 and g.Cin % 64 == 0
            and ext.has("pda_conv_fwd_tail"))


def _conv_fwd_tail(y3, w, g: ConvGeom, out, pro, tail: TailIn, stats, bn, before_finalize):
    if pro is None or not tail_fuse_ok(g, y3.dtype):
        raise ValueError("conv_fwd tail: needs pro = (scale, shift) of the tail BN and a 1x1 "
                         "stride-1 16-bit conv (tail_fuse_ok)")
    if tail.out.shape != y3.shape or tail.res.shape != y3.shape or tail.out.dtype != y3.dtype:
        raise ValueError("conv_fwd tail: y3, the residual and the output activation share one shape")
    if tail.mask is not None and tail.mask.numel() * 8 < y3.numel():
        raise ValueError("conv_fwd tail: mask needs numel / 8 bytes")
    Nb = y3.shape[0]
    M = Nb * g.Ho * g.Wo
    Kpad = w.shape[-1] if w.dim() == 2 else w[0].numel()
    bm, bn_ = -128, (64 if g.Cout <= 64 else 128)
    mode = 2 if tail.sc2 is not None else 1
    d = g.desc(Nb)
    _launch_fwd(lambda st: ext.lib().pda_conv_fwd_tail(
        C.byref(d), ptr(y3), ptr(w), Kpad, ptr(out), ptr(st), ptr(pro[0]), ptr(pro[1]),
        ptr(tail.res), ptr(tail.sc2), ptr(tail.sh2), ptr(tail.out), ptr(tail.mask), mode, _kdt(y3),
        bm, bn_, stream(y3.device)),
        "conv_fwd_tail", math.ceil(M / 128), 128, M, g.Cout, stats, bn, before_finalize)
    return out


_STEM_FWD = True   # the stem conv on csrc/stem.hip (False: the generic 128x64 tile, tests)
# persistent blocks of the stem kernel: 256 / 512 / 1024 / 2048 measured 305 / 267 / 258 / 278 us
# (profiles/ab_r4.md section 15); 0 = the kernel's default, 1024
_STEM_GRID = 0


def stem_fwd_ok(g: ConvGeom, dtype: torch.dtype) -> bool:
    """Whether the space-to-depth stem conv (4x4/1, pad 2 top/left, 16 -> 64 channels) runs on the
    dedicated tap-reuse kernel (csrc/stem.hip): 16-bit, H % 4 == 0, W % 16 == 0, W <= 128."""
    return (_STEM_FWD and dtype in (torch.bfloat16, torch.float16) and g.R == 4 and g.S == 4
            and g.Cin == 16 and g.Cout == 64 and g.stride == 1 and g.pad == 2 and g.Ho == g.H
            and g.Wo == g.W and g.H % 4 == 0 and g.W % 16 == 0 and 16 <= g.W <= 128
            and ext.has("pda_stem_fwd"))


def stem_fwd(x: torch.Tensor, w: torch.Tensor, g: ConvGeom, out: torch.Tensor,
             stats: Optional[torch.Tensor] = None, bn: Optional[BnStats] = None,
             before_finalize=None) -> torch.Tensor:
    """The stem conv on csrc/stem.hip (input slab staged once per 4-row tile in LDS, taps read
    from it; persistent blocks keep the 64 x 256 weights in LDS). Statistics: shifted partials over
    output rows, the format :func:`bn_finalize_partials` / :func:`stats_totals` take
    (pass ``bm = stem_stats_rows(g)``)."""
    Nb = x.shape[0]
    M = Nb * g.Ho * g.Wo
    rows = stem_stats_rows(g)
    T = M // rows
    if bn is None and stats is not None and stats.numel() < T * 3 * g.Cout:
        raise ValueError(f"stem_fwd: stats needs {T * 3 * g.Cout} floats (one partial per output "
                         f"row, stem_stats_rows), got {stats.numel()}")
    _launch_fwd(lambda st: ext.lib().pda_stem_fwd(ptr(x), ptr(w), ptr(out), ptr(st), Nb, g.H, g.W,
                                                  _kdt(x), _STEM_GRID, stream(x.device)),
                "stem_fwd", T, rows, M, g.Cout, stats, bn, before_finalize)
    return out


def stem_stats_rows(g: ConvGeom) -> int:
    """Rows of M per statistics tile of :func:`stem_fwd` (one output row)."""
    return g.Wo


def stats_totals(stats: torch.Tensor, M: int, C_: int, bm: int) -> torch.Tensor:
    """f64 [2][C] (sum y, sum y^2) from conv_fwd's shifted per-tile partials (tests, tools)."""
    T = math.ceil(M / tile_rows(bm))
    p = stats[:T * 3 * C_].view(T, 3, C_).double()
    rows = torch.full((T, 1), float(tile_rows(bm)), dtype=torch.float64, device=stats.device)
    rows[-1, 0] = M - (T - 1) * tile_rows(bm)
    d0, d1, sh = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([(rows * sh + d0).sum(0), (d1 + sh * (2 * d0 + rows * sh)).sum(0)])


def bn_finalize_partials(stats: torch.Tensor, T: int, C_: int, bm: int, M: int, bn: BnStats) -> None:
    """BatchNorm forward statistics from conv_fwd's shifted per-tile partials in one launch
    (csrc/bn.hip bn_stats_kernel<0>): S blocks per 256-channel group reduce tile ranges to f64 slabs,
    the group's last arriving block sums them and finalizes. SyncBatchNorm (``ws.sync_comm``): the
    launch stops at f64 totals, which are all-reduced before :func:`bn_finalize_tot`."""
    G = math.ceil(C_ / _stats_cg(C_))
    S = _stats_slabs(T, C_)
    ws = bn.ws
    slabs = ws.get("bn_slabs", S * 2 * C_, torch.float64)
    cnt = ws.counters(G)
    sync = None if ws.local_stats else ws.sync_comm
    tot = ws.get("bn_tot", 2 * C_, torch.float64) if sync is not None else None
    o = ext.BnFwdOut(ptr(bn.gamma), ptr(bn.beta), bn.eps, bn.momentum, ptr(bn.mean),
                     ptr(bn.invstd), ptr(bn.scale), ptr(bn.shift), ptr(bn.rmean), ptr(bn.rvar),
                     ptr(bn.nbt), int(bn.update), ptr(tot))
    check(ext.lib().pda_bn_fwd_stats(ptr(stats), T, C_, bm, M, S, ptr(slabs), ptr(cnt), C.byref(o),
                                     _stats_cg(C_), stream(stats.device)), "bn_fwd_stats")
    if sync is not None:   # SyncBatchNorm: global f64 totals, then finalize
        sync.all_reduce(tot)
        bn_finalize_tot(tot, C_, M * sync.world_size, bn)


def bn_finalize_tot(tot: torch.Tensor, C_: int, count: int, bn: BnStats) -> None:
    rc = ext.lib().pda_bn_finalize_tot(ptr(tot), C_, float(count), ptr(bn.gamma), ptr(bn.beta),
                                       bn.eps, bn.momentum, ptr(bn.mean), ptr(bn.invstd),
                                       ptr(bn.scale), ptr(bn.shift), ptr(bn.rmean), ptr(bn.rvar),
                                       ptr(bn.nbt), int(bn.update), stream(tot.device))
    check(rc, "bn_finalize_tot")


def stats_tiles(M: int, Cout: int, tile: Optional[Tuple[int, int]] = None) -> int:
    bm, _ = tile or pick_tile(M, Cout)
    return math.ceil(M / tile_rows(bm))


def _halo_geom(g: ConvGeom) -> bool:
    """3x3 / stride 1 / pad 1 convolutions whose input rows fit the tap-reuse slab (W <= 63)."""
    return (g.R == 3 and g.S == 3 and g.stride == 1 and g.pad == 1 and g.W <= 63
            and g.Cin % 64 == 0 and g.Cout % 64 == 0)


def dgrad_tile(g: ConvGeom, Nb: int, dma: bool = True) -> Tuple[int, int]:
    """Data-gradient tile: the tap-reuse (HALO) 256x128 LDS-DMA tile for 3x3 stride-1 layers with
    >= 128 channels (``PDA_DGRAD_HALO``; round 3 measured it slower in the step, 28.03 -> 27.88
    ms/step without it, profiles/ab_r3_dma.md section 11; with the round-4 MFMA-burst priority it
    wins, profiles/ab_r4.md section 17), the register-staged tiles otherwise. ``dma``: 16-bit
    operands (the DMA tiles need them)."""
    if dma and _DMA and _DGRAD_HALO and _halo_geom(g) and g.Cin >= 128:
        return 2256, 128
    M = Nb * (g.H // g.stride) * (g.W // g.stride)
    return pick_tile(M * g.stride * g.stride, g.Cin, g.Cout * _max_class_taps(g))


# the HALO data-gradient tile in the step: slower in round 3; with this round's raised-priority
# MFMA bursts (profiles/ab_r4.md section 11) -0.03 ms/step over 7 in-step pairs (section 17)
_DGRAD_HALO = os.environ.get("PDA_DGRAD_HALO", "1") != "0"


def _max_class_taps(g: ConvGeom) -> int:
    if g.stride == 1:
        return g.R * g.S
    return max(sum(1 for r in range(g.R) if (ph + g.pad - r) % 2 == 0) *
               sum(1 for s in range(g.S) if (pw + g.pad - s) % 2 == 0)
               for ph in (0, 1) for pw in (0, 1))


def dgrad_slabs(g: ConvGeom, Nb: int, tile: Optional[Tuple[int, int]] = None,
                dtype: Optional[torch.dtype] = None) -> int:
    """Number of partial-sum slabs the fused BN epilogue of a dgrad writes (classes x M-tiles);
    ``dtype`` = the dgrad's operand dtype (the tile it launches may differ: :func:`_ktile`)."""
    kdt = 1 if dtype is None else _kdt(torch.empty(0, dtype=dtype))
    bm, bn = tile or dgrad_tile(g, Nb, dma=kdt in (1, 2))
    bm, _ = _ktile(bm, bn, kdt)
    M = Nb * (g.H // g.stride) * (g.W // g.stride)
    return g.stride * g.stride * math.ceil(M / tile_rows(bm))


def conv_dgrad(dy: torch.Tensor, w: torch.Tensor, g: ConvGeom, dx: torch.Tensor,
               tile: Optional[Tuple[int, int]] = None, epi: Optional[ext.BnEpi] = None) -> torch.Tensor:
    """dx[Nb,H,W,Cin] = conv_transpose(dy[Nb,Ho,Wo,Cout], w[Cout,R,S,Cin]).

    With ``epi`` (see :func:`bn_epilogue`) the kernel instead stores dz = dA * relu_mask (dA = the
    transposed conv result [+ epi.g2]) and writes the BatchNorm-backward partial sums."""
    Nb = dy.shape[0]
    kdt = _kdt(dy)
    bm, bn = tile or dgrad_tile(g, Nb, dma=kdt in (1, 2))
    d = g.desc(Nb)
    kbm, kbn = _ktile(bm, bn, kdt)
    rc = ext.lib().pda_conv_dgrad(C.byref(d), ptr(dy), ptr(w), ptr(dx),
                                  C.byref(epi) if epi is not None else None, kdt, kbm, kbn,
                                  stream(dy.device))
    check(rc, "conv_dgrad")
    return dx


def bn_fold(w: torch.Tensor, k: torch.Tensor, wf: torch.Tensor, bias: torch.Tensor,
            ws: Optional["Workspace"] = None) -> None:
    """Operands of :func:`conv_dgrad_bnf` for a 1x1 conv (``w`` 16-bit [Cout, Cin], ``k`` =
    [k1; k2; k3] 3 x Cout f32 of the BatchNorm after it): ``wf`` [Cout + Cin, Cin] = [k1 o W ;
    W^T diag(k2) W], ``bias`` [Cin] = W^T k3 (csrc/conv_gemm.hip bn_fold_kernel, one launch;
    ``ws`` is accepted for call-site symmetry and unused)."""
    Cout, Cin = w.shape[0], w.shape[-1]
    if wf.shape[0] != Cout + Cin or wf.shape[-1] != Cin or wf.dtype != w.dtype or k.numel() < 3 * Cout:
        raise ValueError("bn_fold: wf [Cout + Cin, Cin] of the weights' dtype, k 3 x Cout")
    check(ext.lib().pda_bn_fold(ptr(w), ptr(k), Cout, Cin, ptr(wf), ptr(bias), dt_of(w),
                                stream(w.device)), "bn_fold")


def bnf_ok(g: ConvGeom, dtype: torch.dtype) -> bool:
    """Whether the consumer-side BN-backward fold (:func:`conv_dgrad_bnf`) serves this conv: a 1x1
    conv without padding, 16-bit operands, channel counts in whole 64-column panels."""
    return (g.R == 1 and g.S == 1 and g.pad == 0 and dtype in (torch.bfloat16, torch.float16)
            and g.Cin % 64 == 0 and g.Cout % 64 == 0
            and ext.has("pda_conv_dgrad_bnf"))


def conv_dgrad_bnf(dz: torch.Tensor, wf: torch.Tensor, g: ConvGeom, dx: torch.Tensor,
                   xa: torch.Tensor, bias: torch.Tensor, xa_pro=None,
                   epi: Optional[ext.BnEpi] = None,
                   tile: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """dX of a 1x1 conv whose dY = k1*dz + k2*y + k3 is never materialised (y = the conv's forward
    output): dX = dz . (k1 o W) + xa . G + b with (wf, bias) from :func:`bn_fold` and ``xa`` the
    conv's forward input (``xa_pro`` = (scale, shift): xa is PRE-BatchNorm and the activation
    relu(xa*scale+shift) is recomputed, as the forward's prologue did). ``epi``: the same fused
    BN-backward epilogue as :func:`conv_dgrad`."""
    Nb = dz.shape[0]
    kdt = _kdt(dz)
    bm, bn = tile or dgrad_tile(g, Nb)
    kbm, kbn = _ktile(bm, bn, kdt)
    if kbm > 1000:    # the fold's Gram operand needs the register-staged loader
        kbm, kbn = -128, min(kbn, 128)
    d = g.desc(Nb)
    rc = ext.lib().pda_conv_dgrad_bnf(C.byref(d), ptr(dz), ptr(wf), ptr(dx),
                                      C.byref(epi) if epi is not None else None, ptr(xa),
                                      ptr(xa_pro[0] if xa_pro else None),
                                      ptr(xa_pro[1] if xa_pro else None), ptr(bias),
                                      kdt, kbm, kbn, stream(dz.device))
    check(rc, "conv_dgrad_bnf")
    return dx


def bn_epilogue(ws: "Workspace", G: int, y, scale, shift, res=None, y2=None, scale2=None,
                shift2=None, g2=None, mask=None):
    """Describe the BN-backward reduction a dgrad epilogue performs for a = relu(bn(y) [+res | +bn2(y2)]).
    ``mask`` (the forward's ReLU bitmask of a, see :func:`bn_apply`) replaces ``res``: the epilogue
    then reads one byte per 8 elements instead of the residual tensor (mode 3).
    Returns (epi, part, nq): ``part`` holds G*nq*C partials after the dgrad (:func:`bn_bwd_finish`
    finalizes them)."""
    C_ = y.shape[-1]
    mode = 3 if mask is not None else (2 if y2 is not None else (1 if res is not None else 0))
    nq = 3 if mode == 2 else 2
    part = ws.get("bn_part", G * nq * C_)
    epi = ext.BnEpi(mode, nq, ptr(y), ptr(scale), ptr(shift),
                    ptr(y2 if y2 is not None else res), ptr(scale2), ptr(shift2), ptr(g2), ptr(part),
                    ptr(mask))
    return epi, part, nq


# Weight-gradient tile / split-K block target per ResNet conv geometry (Cout, R, Cin, stride, Ho),
# measured on MI355X at batch 400: tools/wgrad_sweep.py (profiles/wgrad_sweep_r1_v2.txt), then
# tools/conv_bench.py re-measurements (profiles/convbench_r2.txt; round 3: the LDS-DMA 8-wave tiles,
# 1000 + rows, win on the 3x3 and strided weight gradients, profiles/convbench_r3_dma.txt).
_WGRAD_TUNED = {
    (64, 1, 64, 1, 56): ((-64, 128), 512),      # C1
    (64, 3, 64, 1, 56): ((64, 128), 512),       # C2
    (256, 1, 64, 1, 56): ((-128, 64), 512),     # C3 (round 5, decomposed conv3 fold: -128x128 +0.05 ms)
    (64, 1, 256, 1, 56): ((128, 128), 512),     # C4
    (128, 1, 256, 1, 56): ((-128, 128), 512),   # C5
    (128, 3, 128, 2, 28): ((128, 64), 2048),    # C6
    (512, 1, 128, 1, 28): ((128, 128), 512),    # C7
    (512, 1, 256, 2, 28): ((-256, 128), 512),   # C8
    (128, 1, 512, 1, 28): ((-128, 128), 512),   # C9
    (128, 3, 128, 1, 28): ((-64, 128), 512),    # C10
    (256, 1, 512, 1, 28): ((-256, 128), 1024),  # C11
    (256, 3, 256, 2, 14): ((-256, 128), 512),   # C12
    (1024, 1, 256, 1, 14): ((-128, 128), 512),  # C13 (round 5: -0.17 ms/step vs -128x64, ab_r5.md s.14)
    (1024, 1, 512, 2, 14): ((128, 128), 512),   # C14
    (256, 1, 1024, 1, 14): ((-128, 64), 512),   # C15
    (256, 3, 256, 1, 14): ((-256, 128), 2048),  # C16
    (512, 1, 1024, 1, 14): ((128, 128), 512),   # C17
    (512, 3, 512, 2, 7): ((-256, 128), 4096),   # C18
    (2048, 1, 512, 1, 7): ((-128, 128), 512),   # C19
    (2048, 1, 1024, 2, 7): ((-128, 128), 512),  # C20
    (512, 1, 2048, 1, 7): ((128, 128), 512),    # C21
    (512, 3, 512, 1, 7): ((-256, 128), 1024),   # C22
    # stem (4x4/1 on the space-to-depth image, WGRAD_BNA): the 64x256 tile (the whole N: dz and y
    # staged once) at ~1024 splits, 404 us vs 440 for 64x128 at 1536 blocks and 490 at the 512
    # default -- it runs alone at the end of the backward (tools/stem_wgrad_sweep.py)
    (64, 4, 16, 1, 112): ((-64, 256), 1536),
}
_WGRAD_ALONE = {(64, 4, 16, 1, 112)}   # weight gradients with nothing beside them (no x0.7)
# LDS-DMA tiles (16-bit, no operand prologue; the register-staged entry above is the fallback)
_DMA = os.environ.get("PDA_DMA", "1") != "0"
_WGRAD_DMA = {   # tools/wgrad_sweep.py, kernel + slab reduce (profiles/wgrad_sweep_r3{,b}.txt)
    (256, 1, 64, 1, 56): ((1256, 128), 256),    # C3  159 -> 153 us (the downsample; conv3: prologue)
    (64, 1, 256, 1, 56): ((1128, 256), 256),    # C4  160 -> 151
    (128, 1, 256, 1, 56): ((1128, 256), 256),   # C5  206 -> 182
    (128, 3, 128, 2, 28): ((1128, 256), 512),   # C6  200 -> 200 (conv_bench: 221 -> 197)
    (512, 1, 128, 1, 28): ((1256, 128), 256),   # C7  113 ->  98
    (512, 1, 256, 2, 28): ((1256, 256), 512),   # C8  168 -> 137
    (128, 1, 512, 1, 28): ((1128, 256), 256),   # C9  115 ->  96
    (128, 3, 128, 1, 28): ((1128, 256), 512),   # C10 171 -> 168
    (256, 1, 512, 1, 28): ((1256, 256), 256),   # C11 165 -> 140
    (256, 3, 256, 2, 14): ((1256, 256), 512),   # C12 171 -> 124
    (1024, 1, 512, 2, 14): ((1256, 256), 512),  # C14 133 -> 121
    (256, 1, 1024, 1, 14): ((1256, 256), 256),  # C15  78 ->  75
    (256, 3, 256, 1, 14): ((1256, 256), 256),   # C16 161 -> 120
    (512, 1, 1024, 1, 14): ((1256, 256), 256),  # C17 130 -> 122
    (512, 3, 512, 2, 7): ((1256, 256), 512),    # C18 134 -> 119
    (2048, 1, 512, 1, 7): ((1128, 256), 256),   # C19  67 ->  60
    (2048, 1, 1024, 2, 7): ((1256, 256), 512),  # C20 118 -> 111
    (512, 1, 2048, 1, 7): ((1256, 128), 256),   # C21  70 ->  61
    (512, 3, 512, 1, 7): ((1256, 256), 512),    # C22 129 -> 116
}


def wgrad_plan(g: ConvGeom, Nb: int, tile: Optional[Tuple[int, int]] = None,
               target_blocks: Optional[int] = None, max_slab_bytes: int = 64 << 20,
               f32: bool = False, dma: bool = False, wscale: Optional[float] = None,
               bna: bool = False):
    """(bm, bn, splits, k_chunk) of a weight gradient; ``dma``: the launch may use an LDS-DMA tile
    (16-bit operands, no operand prologue); ``wscale``: the split-K block-target factor of the
    caller's schedule (None: ``PDA_WGRAD_SCALE``, the concurrent eager step's x0.7)."""
    M, N, K = g.Cout, g.R * g.S * g.Cin, Nb * g.Ho * g.Wo
    key = (g.Cout, g.R, g.Cin, g.stride, g.Ho)
    tuned = _WGRAD_TUNED.get(key)
    if dma and _DMA and key in _WGRAD_DMA:
        tuned = _WGRAD_DMA[key]
    bn = 128 if N >= 128 else 64
    bm = 128 if M >= 128 else 64
    if bm == 128 or bn == 128:
        bm = -bm      # single-LDS-buffer variants (tools/conv_bench.py: best or within 2%)
    if tuned and not tile:
        (bm, bn), tb = tuned
        target_blocks = target_blocks or tb
        if f32 and (tile_rows(bm) > 128 or bn > 128):   # 256-wide tiles are 16-bit only
            bm, bn = -128, 128
        if bna and (abs(bm), bn) not in _BNA_TILES:     # the nearest tile WGRAD_BNA is built for
            bm, bn = -128, 128
        if bna and M <= 64 and tile_rows(bm) > 64:        # Cout 64 (the layer1 conv1): no idle rows
            bm, bn = -64, 128
    if target_blocks is None:
        target_blocks = _WGRAD_TARGET
    # (the stem's weight gradient runs alone at the end of the backward: its isolated optimum holds)
    sc = _WGRAD_SCALE if wscale is None else wscale
    target_blocks = max(1, int(target_blocks * (1.0 if key in _WGRAD_ALONE else sc)))
    if tile:
        bm, bn = tile
    tiles = math.ceil(M / tile_rows(bm)) * math.ceil(N / bn)
    splits = max(1, min(math.ceil(target_blocks / tiles), math.ceil(K / 256),
                        max(1, max_slab_bytes // (M * N * 4))))
    k_chunk = math.ceil(K / splits / 64) * 64
    splits = math.ceil(K / k_chunk)
    return bm, bn, splits, k_chunk


def wgrad_bna_ok(g: ConvGeom, Nb: int, dtype: torch.dtype) -> bool:
    """Whether :func:`conv_wgrad` can form dY from the BN backward in-kernel for this geometry: 16-bit
    operands on the tiles WGRAD_BNA is built for (64x128, 64x256: the stem's Cout = 64)."""
    if dtype not in (torch.bfloat16, torch.float16) or g.Cout % 8:
        return False
    if not ext.has("pda_conv_wgrad_bna"):
        return False
    bm, bn, _, _ = wgrad_plan(g, Nb, bna=True)
    return (abs(bm), bn) in _BNA_TILES


# tiles pda_conv_wgrad_bna is built for (csrc/conv_gemm.hip BNA_CASE): the stem's 64-row tiles and
# the bottleneck conv3 weight gradients of the consumer-side tail fold
_BNA_TILES = {(64, 128), (64, 256), (128, 128), (128, 64)}


def conv_wgrad(dy: torch.Tensor, x: torch.Tensor, g: ConvGeom, grad: torch.Tensor, ws: Workspace,
               cin_real: Optional[int] = None, scale: float = 1.0, accumulate: bool = False,
               tile: Optional[Tuple[int, int]] = None,
               pro: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               target_blocks: Optional[int] = None,
               bna: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               wscale: Optional[float] = None,
               combine: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """grad (f32, OHWI with cin_real channels, rows of pitch R*S*cin_real) = scale * dW.
    pro = (scale, shift): x is PRE-BatchNorm; the activation relu(x*scale+shift) is recomputed.
    bna = (y, k) with k = [k1; k2; k3] (3 x Cout f32): ``dy`` is the BN-backward's masked gradient
    dz and the kernel stages dY = k1*dz + k2*y + k3 itself (csrc/conv_gemm.hip WGRAD_BNA; see
    :func:`wgrad_bna_ok`).
    combine = (k, B, s): the decomposed form of that weight gradient -- ``dy`` is dz, the GEMM is
    the plain dz^T x, and the split-K reduce writes k1*(dz^T x) + k2*B + k3*s^T per row, with
    B = W Gram(x) and s the column sums of x (:func:`conv_wgrad_gram`, :func:`fold_bgemm`)."""
    Nb = dy.shape[0]
    if (tile is None and target_blocks is None and bna is None and combine is None
            and cin_real is None and wgrad_tap_ok(g, dy.dtype)):
        return conv_wgrad_tap(dy, x, g, grad, ws, scale, accumulate, pro)
    if (tile is None and target_blocks is None and bna is not None and combine is None
            and cin_real is None and pro is None and stem_wgrad_tap_ok(g, dy.dtype)):
        return conv_wgrad_stem_tap(dy, bna[0], bna[1], x, g, grad, ws, scale, accumulate)
    bm, bn, splits, k_chunk = wgrad_plan(g, Nb, tile, target_blocks, f32=dy.dtype == torch.float32,
                                         dma=dy.dtype != torch.float32 and pro is None and bna is None,
                                         wscale=wscale, bna=bna is not None)
    if bna is None and bm == -64 and bn == 256:
        # 64x256 is a WGRAD_BNA tile: the plain weight gradient of that plan runs 64x128 tiles over
        # the same split-K chunks (same accumulation order per element: bitwise the same result)
        bn = 128
    M, N = g.Cout, g.R * g.S * g.Cin
    rb = ws.reduce_batch if N % 4 == 0 else None
    slab = rb.slab(splits * M * N) if rb is not None else ws.get("wgrad_slab", splits * M * N)
    d = g.desc(Nb)
    st = stream(dy.device)
    kdt = _kdt(dy)
    kbm, kbn = _ktile(bm, bn, kdt)
    if bna is not None:
        y, k = bna
        Co = g.Cout
        rc = ext.lib().pda_conv_wgrad_bna(C.byref(d), ptr(dy), ptr(y), ptr(k[0:Co]), ptr(k[Co:2 * Co]),
                                          ptr(k[2 * Co:3 * Co]), ptr(x), ptr(slab), splits, k_chunk,
                                          ptr(pro[0] if pro else None), ptr(pro[1] if pro else None),
                                          kdt, kbm, kbn, st)
        check(rc, "conv_wgrad_bna")
    else:
        rc = ext.lib().pda_conv_wgrad(C.byref(d), ptr(dy), ptr(x), ptr(slab), splits, k_chunk,
                                      ptr(pro[0] if pro else None), ptr(pro[1] if pro else None),
                                      kdt, kbm, kbn, st)
        check(rc, "conv_wgrad")
    cr = g.Cin if cin_real is None else cin_real
    ck, cB, cs = combine if combine is not None else (None, None, None)
    if rb is not None:
        rb.add(slab, grad, splits, M, N, int(math.log2(g.Cin)), cr, g.R * g.S * cr, scale,
               accumulate, ck, cB, cs)
        return grad
    rc = ext.lib().pda_wgrad_reduce(ptr(slab), ptr(grad), splits, M, N, int(math.log2(g.Cin)), cr,
                                    g.R * g.S * cr, float(scale), int(accumulate), ptr(ck), ptr(cB),
                                    ptr(cs), st)
    check(rc, "wgrad_reduce")
    return grad


# which 3x3 stride-1 weight gradients run the tap-reuse kernel (csrc/wgrad_tap.hip), by image width
# ("0": none); the generic tiles re-read X per (tap, channel) column tile and dY per N-tile
_WGRAD_TAP = {int(v) for v in os.environ.get("PDA_WGRAD_TAP", "56,28").replace("+", ",").split(",")
              if v.strip() not in ("", "0")}
# blocks of the tap-reuse weight gradient (one 104 KiB block per CU: the split count is the block
# count). Alone 256 is fastest (C2 165 vs 176 us at 512); in the step fewer blocks leave the other
# CUs to the main chain: 256 / 192 / 128 / 112 / 96 / 80 / 64 -> 96 (-0.2 ms/step vs 256;
# profiles/ab_r5.md section 15)
_WGRAD_TAP_BLOCKS = int(os.environ.get("PDA_WGRAD_TAP_BLOCKS", "96"))


def wgrad_tap_ok(g: ConvGeom, dtype: torch.dtype) -> bool:
    """Whether :func:`conv_wgrad` runs the tap-reuse kernel for this conv: 3x3 / stride 1 / pad 1,
    16-bit, channel counts in 64-column tiles, image width in the ``PDA_WGRAD_TAP`` set (<= 59).
    Cin must be a power of two: the reduce decodes a slab column's tap as ``n >> log2(Cin)``."""
    return (dtype in (torch.bfloat16, torch.float16) and g.R == 3 and g.S == 3 and g.stride == 1
            and g.pad == 1 and g.Ho == g.H and g.Wo == g.W and g.W <= 59 and g.W in _WGRAD_TAP
            and g.Cin % 64 == 0 and g.Cout % 64 == 0 and (g.Cin & (g.Cin - 1)) == 0
            and ext.has("pda_wgrad_tap"))


def wgrad_tap_plan(g: ConvGeom, Nb: int, blocks: int = _WGRAD_TAP_BLOCKS) -> Tuple[int, int]:
    """(kb, splits): padded pixel rows per split (a multiple of 64) and the split count of the
    tap-reuse weight gradient for ~``blocks`` blocks over its (Cout / 64) x (Cin / 64) tiles."""
    kp = Nb * (g.H + 2) * (g.W + 2)
    tiles = (g.Cout // 64) * (g.Cin // 64)
    want = max(1, blocks // tiles)
    kb = max(64, math.ceil(kp / want / 64) * 64)
    return kb, math.ceil(kp / kb)


def conv_wgrad_tap(dy: torch.Tensor, x: torch.Tensor, g: ConvGeom, grad: torch.Tensor,
                   ws: "Workspace", scale: float = 1.0, accumulate: bool = False,
                   pro: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:
    """grad (f32 OHWI) = scale * dW of a 3x3 stride-1 conv on the tap-reuse kernel: each block
    loads its pixel range of dY and X once for all nine taps (csrc/wgrad_tap.hip), split-K slabs
    reduced by the same fixed-order launch as :func:`conv_wgrad`. ``pro`` as there."""
    Nb = dy.shape[0]
    kb, splits = wgrad_tap_plan(g, Nb)
    M, N = g.Cout, 9 * g.Cin
    rb = ws.reduce_batch
    slab = rb.slab(splits * M * N) if rb is not None else ws.get("wgrad_slab", splits * M * N)
    st = stream(dy.device)
    L = ext.lib()
    check(L.pda_wgrad_tap(ptr(dy), ptr(x), ptr(slab), ptr(pro[0] if pro else None),
                          ptr(pro[1] if pro else None), Nb, g.H, g.W, g.Cin, g.Cout, kb, splits,
                          _kdt(dy), st), "wgrad_tap")
    if rb is not None:
        rb.add(slab, grad, splits, M, N, int(math.log2(g.Cin)), g.Cin, N, scale, accumulate)
        return grad
    check(L.pda_wgrad_reduce(ptr(slab), ptr(grad), splits, M, N, int(math.log2(g.Cin)), g.Cin, N,
                             float(scale), int(accumulate), None, None, None, st), "wgrad_reduce")
    return grad


# PDA_STEM_WGRAD=tap: the stem's weight gradient (WGRAD_BNA operand) on the tap-reuse kernel
# (csrc/wgrad_tap.hip wgrad_stem_tap_kernel) instead of the implicit-GEMM WGRAD_BNA 64x256 tile.
# Off by default: 368-381 us vs 375-380 us alone at batch 400, step time unchanged within noise
# (profiles/ab_r6.md section 15). Blocks = splits (one 113 KiB block per CU)
_STEM_WGRAD = os.environ.get("PDA_STEM_WGRAD", "generic")
_STEM_TAP_BLOCKS = int(os.environ.get("PDA_STEM_TAP_BLOCKS", "512"))


# Events that order the second stream after the main one (fork tracking's per-launch completion
# event, the DataParallel replay's side-graph hand-offs). PDA_EVENT_SYSFENCE=1: HIP's default event,
# whose completion carries a SYSTEM-scope release (a full L2 write-back, for host / peer
# visibility); 0: hipEventDisableSystemFence -- only a stream of the same device waits on these,
# for which the agent-scope release of the kernel's own completion is enough.
_EVENT_SYSFENCE = os.environ.get("PDA_EVENT_SYSFENCE", "1") == "1"


def fork_event_create():
    """A ``hipEvent_t`` (ctypes void pointer) for same-device stream ordering: timing disabled,
    system-scope fence per PDA_EVENT_SYSFENCE."""
    ev = C.c_void_p()
    flags = 0x2 | (0 if _EVENT_SYSFENCE else 0x20000000)   # hipEventDisableTiming | ...SystemFence
    check(ext.lib().pda_event_create_flags(C.byref(ev), flags), "pda_event_create_flags")
    return ev


def stem_wgrad_tap_ok(g: ConvGeom, dtype: torch.dtype, force: bool = False) -> bool:
    """The space-to-depth stem conv (4x4, stride 1, pad 2, 16 -> 64 channels, same-size output) in
    16 bit, with the tap-reuse stem kernel built (and selected, unless ``force``)."""
    return ((force or _STEM_WGRAD == "tap") and dtype in (torch.bfloat16, torch.float16) and g.R == 4
            and g.S == 4 and g.stride == 1 and g.pad == 2 and g.Cin == 16 and g.Cout == 64
            and g.Ho == g.H and g.Wo == g.W and g.W + 3 <= 122
            and ext.has("pda_wgrad_stem_tap"))


def conv_wgrad_stem_tap(dz: torch.Tensor, y: torch.Tensor, k: torch.Tensor, x: torch.Tensor,
                        g: ConvGeom, grad: torch.Tensor, ws: "Workspace", scale: float = 1.0,
                        accumulate: bool = False, blocks: Optional[int] = None) -> torch.Tensor:
    """grad (f32 [64][16 taps x 16]) = scale * dW of the stem conv with dY = k1*dz + k2*y + k3
    formed in LDS (:func:`conv_wgrad` ``bna``): each block loads its pixel range of dz, y and the
    input once for all 16 taps; split-K slabs reduced by the same fixed-order launch."""
    Nb = dz.shape[0]
    kp = Nb * (g.H + 3) * (g.W + 3)
    nb = blocks or _STEM_TAP_BLOCKS
    kb = max(64, math.ceil(kp / nb / 64) * 64)
    splits = math.ceil(kp / kb)
    M, N = 64, 256
    rb = ws.reduce_batch
    slab = rb.slab(splits * M * N) if rb is not None else ws.get("wgrad_slab", splits * M * N)
    st = stream(dz.device)
    L = ext.lib()
    check(L.pda_wgrad_stem_tap(ptr(dz), ptr(y), ptr(k), ptr(x), ptr(slab), Nb, g.H, g.W, kb, splits,
                               _kdt(dz), st), "wgrad_stem_tap")
    if rb is not None:
        rb.add(slab, grad, splits, M, N, 4, 16, N, scale, accumulate)
        return grad
    check(L.pda_wgrad_reduce(ptr(slab), ptr(grad), splits, M, N, 4, 16, N, float(scale),
                             int(accumulate), None, None, None, st), "wgrad_reduce")
    return grad


_TAP_MASKS: Dict = {}


def stem_tap_colsum(x: torch.Tensor, g: ConvGeom) -> torch.Tensor:
    """f32 [R*S*Cin] (column t*Cin + ci, t = r*S + s): the sum over every valid output pixel of
    the stem conv's tap-(r, s) input, X[n][oy + r - pad][ox + s - pad][ci] (zero outside) -- the
    k3 term of the decomposed stem weight gradient. Tap r sees input rows [r - pad, H - 1 + r - pad]
    clipped to the image, so each tap's sum is the image total minus its excluded border rows /
    columns (the first R-1-pad, the last pad) plus their corners: a few small reductions of x
    (slices only: no index tensors, no host copies after the first call), not a pass per tap."""
    Nb, H, W, Cin = x.shape
    R, S, pad = g.R, g.S, g.pad
    assert g.stride == 1 and g.Ho == H and g.Wo == W and H > 2 * R and W > 2 * S and pad < R
    nt, nb = R - 1 - pad, pad            # excluded top / bottom rows (and left / right columns)
    key = (H, W, R, S, pad, x.device)
    if key not in _TAP_MASKS:
        rows = list(range(nt)) + list(range(H - nb, H))
        cols = list(range(nt)) + list(range(W - nb, W))
        mr = [[0.0 if r - pad <= y <= H - 1 + r - pad else 1.0 for y in rows] for r in range(R)]
        mc = [[0.0 if q - pad <= c <= W - 1 + q - pad else 1.0 for c in cols] for q in range(S)]
        _TAP_MASKS[key] = (torch.tensor(mr, device=x.device), torch.tensor(mc, device=x.device))
    mr, mc = _TAP_MASKS[key]
    f32 = torch.float32
    tot = x.sum(dim=(0, 1, 2), dtype=f32)                                            # [Cin]
    rs = torch.cat([x[:, :nt].sum(dim=(0, 2), dtype=f32),
                    x[:, H - nb:].sum(dim=(0, 2), dtype=f32)])                       # [nr, Cin]
    cs = torch.cat([x[:, :, :nt].sum(dim=(0, 1), dtype=f32),
                    x[:, :, W - nb:].sum(dim=(0, 1), dtype=f32)])                    # [nc, Cin]
    q = torch.cat([torch.cat([x[:, :nt, :nt].sum(0, dtype=f32), x[:, :nt, W - nb:].sum(0, dtype=f32)], 1),
                   torch.cat([x[:, H - nb:, :nt].sum(0, dtype=f32),
                              x[:, H - nb:, W - nb:].sum(0, dtype=f32)], 1)])        # [nr, nc, Cin]
    out = (tot[None, None] - (mr @ rs)[:, None] - (mc @ cs)[None, :]
           + torch.einsum("ra,sb,abc->rsc", mr, mc, q))
    return out.reshape(-1).contiguous()


def conv_wgrad_gram(y: torch.Tensor, sc: torch.Tensor, sh: torch.Tensor, gram: torch.Tensor,
                    ws: "Workspace") -> None:
    """gram [C + 1][C]: rows 0..C-1 = a^T a, row C = the column sums of a = relu(y*sc + sh) (y
    16-bit NHWC, C channels; csrc/conv_gemm.hip WGRAD_GRAM: both operands staged through the
    BN+ReLU, the diagonal tiles stage one image for both; split-K slabs reduced in fixed order by
    one launch). The forward-time half of the decomposed tail-fold weight gradient
    (:func:`conv_wgrad` ``combine``)."""
    Nb, H, W, C_ = y.shape
    if gram.numel() < (C_ + 1) * C_ or gram.dtype != torch.float32:
        raise ValueError("conv_wgrad_gram: gram f32 [C + 1][C]")
    P = Nb * H * W
    bm, bn = (64, 64) if C_ <= 64 else (-128, 128)
    tiles = math.ceil(C_ / tile_rows(bm)) * math.ceil(C_ / bn)
    splits = max(1, min(math.ceil(2 * _NUM_CU / tiles), math.ceil(P / 256),
                        max(1, (64 << 20) // (C_ * (C_ + 1) * 4))))
    k_chunk = math.ceil(P / splits / 64) * 64
    splits = math.ceil(P / k_chunk)
    slab = ws.get("gram_slab", splits * C_ * (C_ + 1))
    d = ConvGeom(Nb, H, W, C_, C_, 1, 1, 1, 0).desc(Nb)
    st = stream(y.device)
    L = ext.lib()
    check(L.pda_conv_wgrad_gram(C.byref(d), ptr(y), ptr(sc), ptr(sh), ptr(slab), splits, k_chunk,
                                _kdt(y), bm, bn, st), "conv_wgrad_gram")
    check(L.pda_wgrad_reduce(ptr(slab), ptr(gram), splits, C_ + 1, C_, int(math.log2(C_)), C_, C_,
                             1.0, 0, None, None, None, st), "gram_reduce")


def fold_bgemm(w: torch.Tensor, gram: torch.Tensor, out: torch.Tensor) -> None:
    """out [Cout][C] f32 = W Gram (W 16-bit [Cout][C], the forward's weights)."""
    Cout, C_ = w.shape[0], w.shape[-1]
    check(ext.lib().pda_fold_bgemm(ptr(w), ptr(gram), Cout, C_, ptr(out), dt_of(w), stream(w.device)),
          "fold_bgemm")


# ------------------------------------------------------------------ batchnorm
_PRE_S = 96


def prereduce(part: torch.Tensor, G: int, QC: int, ws: Optional["Workspace"] = None):
    """[G][QC] partial slabs -> [S][QC] with S in [96, 512] (coalesced first stage; narrow layers
    get more slices so the stage fills the chip), so the per-channel finalize kernels never walk
    thousands of slabs serially. Returns (part, G)."""
    S = max(_PRE_S, min(512, 65536 // max(QC, 1)))   # enough blocks for narrow layers
    if G <= 2 * S:
        return part, G
    out = (ws.get("bn_pre", 512 * QC) if ws is not None
           else torch.empty(S * QC, dtype=torch.float32, device=part.device))
    s = ext.lib().pda_slab_reduce(ptr(part), G, QC, S, ptr(out), stream(part.device))
    if s < 0:
        raise RuntimeError("slab_reduce launch failed")
    return out, s


def _sync_sums(part: torch.Tensor, G: int, QC: int, ws: "Workspace"):
    """SyncBatchNorm: [G][QC] partials -> one [QC] row (own slab kernel, fixed order), summed over
    the ranks of ``ws.sync_comm`` (ordered on the current stream). Returns (part, G, world)."""
    if ws.local_stats:
        return part, G, 1
    comm = ws.sync_comm
    tot = ws.get("bn_sync", QC)
    if ext.lib().pda_slab_reduce(ptr(part), G, QC, 1, ptr(tot), stream(part.device)) < 0:
        raise RuntimeError("slab_reduce launch failed")
    comm.all_reduce(tot)
    return tot, 1, comm.world_size


def bn_eval_coeffs(gamma, beta, rmean, rvar, eps, scale, shift) -> None:
    rc = ext.lib().pda_bn_eval_coeffs(ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(eps),
                                      gamma.numel(), ptr(scale), ptr(shift), stream(gamma.device))
    check(rc, "bn_eval_coeffs")


def _bn_shape(what: str, y, reduce: bool = False) -> None:
    """The stand-alone BatchNorm kernels (csrc/bn.hip) work on 8-channel chunks of whole rows; the
    reduce walks a row in passes of 256 chunks with no tail check. ValueError otherwise (the C
    launchers refuse the same shapes with -2)."""
    C_ = y.shape[-1] if y.dim() else 0
    if C_ < 8 or C_ % 8 or y.numel() % C_:
        raise ValueError(f"{what}: shape {tuple(y.shape)} needs a channel count (last dimension) "
                         f"that is a multiple of 8")
    if reduce and (y.numel() == 0 or (C_ > 2048 and C_ % 2048)):
        raise ValueError(f"{what}: shape {tuple(y.shape)} needs at least one row and a channel "
                         f"count of at most 2048 or a multiple of 2048")


def _bn_check(rc: int, what: str, y) -> None:
    if rc == -2:
        raise ValueError(f"{what}: shape {tuple(y.shape)} refused by the kernel library")
    check(rc, what)


def bn_apply(y, scale, shift, out, res=None, y2=None, scale2=None, shift2=None, relu=True,
             mask=None):
    """out = act(bn(y) [+ res | + bn2(y2)]); mask (uint8, numel/8) optionally receives the output's
    ReLU bitmask (bit e of byte i: element 8i+e > 0)."""
    _bn_shape("bn_apply", y)
    mode = 2 if y2 is not None else (1 if res is not None else 0)
    r2 = y2 if y2 is not None else res
    rc = ext.lib().pda_bn_apply(ptr(y), ptr(scale), ptr(shift), ptr(r2), ptr(scale2), ptr(shift2),
                                ptr(out), y.numel(), y.shape[-1], mode, int(relu), ptr(mask),
                                dt_of(y), stream(y.device))
    _bn_check(rc, "bn_apply", y)
    return out


def stem_pool(y, scale, shift, out, arg):
    N, H, W, C_ = y.shape
    Ho, Wo = out.shape[1], out.shape[2]
    rc = ext.lib().pda_stem_pool(ptr(y), ptr(scale), ptr(shift), ptr(out), ptr(arg), N, H, W, C_, Ho,
                                 Wo, dt_of(y), stream(y.device))
    check(rc, "stem_pool")
    return out


def maxpool_bwd(dout, arg, din, dout2=None):
    N, H, W, C_ = din.shape
    Ho, Wo = dout.shape[1], dout.shape[2]
    rc = ext.lib().pda_maxpool_bwd(ptr(dout), ptr(dout2), ptr(arg), ptr(din), N, H, W, C_, Ho, Wo,
                                   dt_of(din), stream(din.device))
    check(rc, "maxpool_bwd")
    return din


def tail_pool(y, scale, shift, out, res=None, y2=None, scale2=None, shift2=None):
    N, H, W, C_ = y.shape
    mode = 2 if y2 is not None else 1
    r2 = y2 if y2 is not None else res
    rc = ext.lib().pda_tail_pool(ptr(y), ptr(scale), ptr(shift), ptr(r2), ptr(scale2), ptr(shift2),
                                 ptr(out), N, H * W, C_, mode, dt_of(y), stream(y.device))
    check(rc, "tail_pool")
    return out


def stem_bwd_reduce(ws: "Workspace", dout, arg, y, scale, shift, dz_out, dout2=None):
    """Stem backward, one pass: max-pool gradient gather (``dout`` [+ ``dout2``] through the argmax
    bytes) -> ReLU mask of relu(bn(y)) -> ``dz_out`` -> BatchNorm-backward partial sums.
    Returns (part, G, nq) for :func:`bn_bwd_finish`."""
    N, H, W, C_ = y.shape
    Ho, Wo = dout.shape[1], dout.shape[2]
    G = max(1, min(_STEM_G, (N * H * W) // 512))   # gather-latency bound: more blocks than a reduce
    part = ws.get("bn_part", G * 2 * C_)
    rc = ext.lib().pda_stem_bwd_reduce(ptr(dout), ptr(dout2), ptr(arg), ptr(y), ptr(scale), ptr(shift),
                                       ptr(dz_out), ptr(part), G, N, H, W, C_, Ho, Wo, dt_of(y),
                                       stream(y.device))
    check(rc, "stem_bwd_reduce")
    return part, G, 2


def _reduce_blocks(rows: int, C_: int) -> int:
    tpr = min(C_ // 8, 256)
    rpi = 256 // tpr
    # aim for ~1024 blocks with >= 4 row iterations each
    return max(1, min(1024, rows // (rpi * 4) or 1))


def bn_bwd(ws: Workspace, y, mean, invstd, gamma, scale, shift, dgamma, dbeta, dy_out,
           g1=None, g2=None, gp=None, res=None, y2=None, mean2=None, invstd2=None, gamma2=None,
           scale2=None, shift2=None, dgamma2=None, dbeta2=None, dy2_out=None, dz_buf=None,
           no_mask: bool = False, gscale: float = 1.0, accumulate: bool = False) -> None:
    """Backward of  a = relu(bn(y) [+ res | + bn2(y2)])  w.r.t. y (and y2).

    The incoming gradient is ``g1 (+ g2)`` or, for the pooled head, ``gp[n][c] / HW``.
    Writes dgamma/dbeta (f32, * gscale, optionally accumulated) and dy_out (16-bit).
    With a residual (``res`` or ``y2``) the masked gradient dz is materialised in ``dz_buf``
    because it is also the gradient of the shortcut input."""
    _bn_shape("bn_bwd", y, reduce=True)
    N, H, W, C_ = y.shape
    rows = N * H * W
    mode = 3 if no_mask else (2 if y2 is not None else (1 if res is not None else 0))
    nq = 3 if mode == 2 else 2
    G = _reduce_blocks(rows, C_)
    part = ws.get("bn_part", G * nq * C_)
    a = BwdArgs(ptr(g1), ptr(g2), ptr(gp), H * W if gp is not None else 0,
                ptr(y), ptr(scale), ptr(shift),
                ptr(y2 if y2 is not None else res), ptr(scale2), ptr(shift2),
                mode, ptr(dz_buf), ptr(part), nq, rows, C_)
    st = stream(y.device)
    L = ext.lib()
    dt = dt_of(y)
    _bn_check(L.pda_bn_bwd_reduce(C.byref(a), G, dt, st), "bn_bwd_reduce", y)
    _bn_bwd_tail(ws, part, G, nq, mode, a, y, mean, invstd, gamma, dgamma, dbeta, dy_out,
                 y2, mean2, invstd2, gamma2, dgamma2, dbeta2, dy2_out, dz_buf, gscale, accumulate)


def bn_bwd_reduce_pooled(ws: "Workspace", gp, dz, y, scale, shift, res=None, y2=None, scale2=None,
                         shift2=None):
    """BN-backward reduction of the last tail a = relu(bn(y) [+res | +bn2(y2)]) from the pooled head
    gradient ``gp`` [N][C] (each position's gradient is gp / HW: no producing dgrad to fuse into).
    Writes the masked gradient ``dz``; returns (part, G, nq) for :func:`bn_bwd_finish`."""
    N, H, W, C_ = y.shape
    G = _reduce_blocks(N * H * W, C_)
    nq = 3 if y2 is not None else 2
    part = ws.get("bn_part", G * nq * C_)
    a = BwdArgs(None, None, ptr(gp), H * W, ptr(y), ptr(scale), ptr(shift),
                ptr(y2 if y2 is not None else res), ptr(scale2), ptr(shift2),
                2 if y2 is not None else 1, ptr(dz), ptr(part), nq, N * H * W, C_)
    check(ext.lib().pda_bn_bwd_reduce(C.byref(a), G, dt_of(dz), stream(dz.device)), "bn_bwd_reduce")
    return part, G, nq


def bn_bwd_finish(ws: "Workspace", part, G: int, nq: int, y, mean, invstd, gamma, dgamma, dbeta,
                  dz, dy_out, y2=None, mean2=None, invstd2=None, gamma2=None, dgamma2=None,
                  dbeta2=None, dy2_out=None, gscale: float = 1.0, accumulate: bool = False,
                  k_out: Optional[torch.Tensor] = None) -> None:
    """Finalize + apply of a BN backward whose reduction a dgrad epilogue already produced
    (partials ``part`` [G][nq][C], masked gradient ``dz``): ONE finalize launch (csrc/bn.hip
    bn_stats_kernel<1>: f64 slabs + last-arriver combine -> gamma/beta gradients and the apply
    coefficients of both branches), then the apply pass(es). SyncBatchNorm takes the separate
    reduce -> all-reduce -> finalize path.
    ``k_out`` (f32, 3 x C per branch: [k1; k2; k3] of branch 1, then of the shortcut branch; not
    SyncBatchNorm): the apply coefficients are written there and the apply pass of every branch
    whose output is None is skipped -- its consumer forms dy itself (:func:`conv_wgrad` ``bna``,
    :func:`conv_dgrad_bnf`)."""
    _bn_shape("bn_bwd_finish", y)
    N, H, W, C_ = y.shape
    mode = 2 if nq == 3 else 1   # dz is materialised in both cases
    a = BwdArgs(None, None, None, 0, ptr(y), None, None, ptr(y2), None, None, mode, None, ptr(part),
                nq, N * H * W, C_)
    if k_out is not None and (not ws.local_stats or k_out.numel() < 3 * (nq - 1) * C_):
        raise ValueError("bn_bwd_finish: k_out needs the non-synchronised form and 3 x C per branch")
    if ws.local_stats:
        k = ws.get("bn_k", 6 * C_) if k_out is None else k_out
        S = _stats_slabs(G, C_)
        slabs = ws.get("bn_slabs", S * nq * C_, torch.float64)
        cnt = ws.counters(math.ceil(C_ / _stats_cg(C_)))
        o = ext.BnBwdOut(float(N * H * W), float(gscale), int(accumulate))
        o.gamma[0], o.mean[0], o.invstd[0] = ptr(gamma), ptr(mean), ptr(invstd)
        o.dgamma[0], o.dbeta[0] = ptr(dgamma), ptr(dbeta)
        if nq == 3:
            o.gamma[1], o.mean[1], o.invstd[1] = ptr(gamma2), ptr(mean2), ptr(invstd2)
            o.dgamma[1], o.dbeta[1] = ptr(dgamma2), ptr(dbeta2)
        o.k = ptr(k)
        L, st, dt = ext.lib(), stream(y.device), dt_of(y)
        check(L.pda_bn_bwd_stats(ptr(part), G, nq, C_, S, ptr(slabs), ptr(cnt), C.byref(o),
                                 _stats_cg(C_), st), "bn_bwd_stats")
        if mode == 2 and dy_out is not None and dy2_out is not None and _BWD_APPLY2:
            rc = L.pda_bn_bwd_apply2(ptr(dz), ptr(y), ptr(y2), ptr(k), ptr(dy_out), ptr(dy2_out),
                                     N * H * W, C_, dt, st)
            if rc == 0:
                return   # both branches in one pass over dz
            if rc != -1:   # -1: this dtype / grid takes the two passes below
                _bn_check(rc, "bn_bwd_apply2", y)
        if dy_out is not None:
            _bn_check(L.pda_bn_bwd_apply(C.byref(a), ptr(dz), ptr(y), ptr(k[0:C_]),
                                         ptr(k[C_:2 * C_]), ptr(k[2 * C_:3 * C_]), ptr(dy_out), dt,
                                         st), "bn_bwd_apply", y)
        if mode == 2 and dy2_out is not None:
            _bn_check(L.pda_bn_bwd_apply(C.byref(a), ptr(dz), ptr(y2), ptr(k[3 * C_:4 * C_]),
                                         ptr(k[4 * C_:5 * C_]), ptr(k[5 * C_:6 * C_]), ptr(dy2_out),
                                         dt, st), "bn_bwd_apply2", y)
        return
    _bn_bwd_tail(ws, part, G, nq, mode, a, y, mean, invstd, gamma, dgamma, dbeta, dy_out,
                 y2, mean2, invstd2, gamma2, dgamma2, dbeta2, dy2_out, dz, gscale, accumulate)


# channels per block group of the statistics kernel (csrc/bn.hip stats_cg): a quad of channels gets
# 1024 / cg lanes, so narrower groups shorten both levels' serial load chains.  Measured in step
# (profiles/ab_r5.md section 17): 64-channel groups -0.12 ms/step against 256 since the round-5
# hand-off dropped its release fence (round 4, with the fence: 64 was +0.03), 32 -0.05; S =
# sqrt(0.75 T) slabs with at least 8 (0.2: +0.16, 1.5 / 3.0: within noise)
_BN_CG = 64
_BN_SK = 0.75
_BN_SMIN = 8


def _stats_cg(C_: int) -> int:
    return min(C_, _BN_CG)


def _stats_slabs(T: int, C_: int) -> int:
    """Blocks per channel group of the one-launch statistics kernel: level 1 reads T/S tiles per
    block, the group's last arriver S slabs -- S ~ sqrt(T) balances the two (both run at one CU's
    bandwidth), at least 8 when T allows so the level-1 reads spread over CUs."""
    return max(1, min(T, max(_BN_SMIN, int(math.sqrt(_BN_SK * T)))))


def _bn_bwd_tail(ws, part, G, nq, mode, a, y, mean, invstd, gamma, dgamma, dbeta, dy_out,
                 y2, mean2, invstd2, gamma2, dgamma2, dbeta2, dy2_out, dz_buf, gscale, accumulate):
    C_ = y.shape[-1]
    rows = y.numel() // C_
    st = stream(y.device)
    L = ext.lib()
    dt = dt_of(y)
    part, G = prereduce(part, G, nq * C_, ws)
    part, G, world = _sync_sums(part, G, nq * C_, ws)
    # SyncBN: the input-gradient coefficients need the GLOBAL sums, while gamma/beta keep the
    # per-rank gradient (torch SyncBatchNorm) that the DDP bucket average then combines
    gscale = gscale / world
    k = ws.get("bn_k", 6 * C_)
    check(L.pda_bn_bwd_finalize(ptr(part), G, nq, 1, C_, float(rows * world), ptr(gamma), ptr(mean),
                                ptr(invstd), ptr(dgamma), ptr(dbeta), ptr(k[0:C_]),
                                ptr(k[C_:2 * C_]), ptr(k[2 * C_:3 * C_]), float(gscale),
                                int(accumulate), st), "bn_bwd_finalize")
    if mode == 2:
        check(L.pda_bn_bwd_finalize(ptr(part), G, nq, 2, C_, float(rows * world), ptr(gamma2), ptr(mean2),
                                    ptr(invstd2), ptr(dgamma2), ptr(dbeta2), ptr(k[3 * C_:4 * C_]),
                                    ptr(k[4 * C_:5 * C_]), ptr(k[5 * C_:6 * C_]), float(gscale),
                                    int(accumulate), st), "bn_bwd_finalize2")
    dz_in = dz_buf if mode in (1, 2) else None
    check(L.pda_bn_bwd_apply(C.byref(a), ptr(dz_in), ptr(y), ptr(k[0:C_]), ptr(k[C_:2 * C_]),
                             ptr(k[2 * C_:3 * C_]), ptr(dy_out), dt, st), "bn_bwd_apply")
    if mode == 2:
        check(L.pda_bn_bwd_apply(C.byref(a), ptr(dz_buf), ptr(y2), ptr(k[3 * C_:4 * C_]),
                                 ptr(k[4 * C_:5 * C_]), ptr(k[5 * C_:6 * C_]), ptr(dy2_out), dt, st),
              "bn_bwd_apply2")


# ------------------------------------------------------------------ head / loss
def xent(logits: torch.Tensor, labels: torch.Tensor, loss_rows, loss, dlog=None,
         gscale: float = 1.0, gdev: Optional[torch.Tensor] = None) -> None:
    """loss_rows (f32 [B], always written) / loss (nullable) = CE(logits, labels); dlog (16-bit
    [B, ld]) = d(mean CE)/dlogits * gscale * gdev[0] (zero in the padding columns)."""
    if loss_rows is None:
        raise ValueError("xent: loss_rows is required (the kernel writes it on every launch)")
    B, K = logits.shape[0], logits.shape[1]
    ld_out = dlog.shape[1] if dlog is not None else 0
    dt = dt_of(dlog) if dlog is not None else 1
    rc = ext.lib().pda_xent(ptr(logits), B, K, logits.stride(0), ptr(labels), ptr(loss_rows), ptr(loss),
                            ptr(dlog), ld_out, float(gscale), ptr(gdev), dt, int(dlog is not None),
                            stream(logits.device))
    check(rc, "xent")


def xent_soft_check(logits, labels, labels_b, lam: float, eps: float, dlog=None) -> Tuple[int, int]:
    """Host-side validation of an :func:`xent_soft` call; returns (B, K). Pure Python, run before
    the launch (NaN fails every comparison)."""
    if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
        raise ValueError("xent_soft: logits must be f32 [B, K] with unit column stride")
    B, K = logits.shape
    if B < 1 or K < 1 or logits.stride(0) < K:
        raise ValueError(f"xent_soft: bad logits shape {tuple(logits.shape)} / row stride {logits.stride(0)}")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or not labels.is_contiguous():
        raise ValueError(f"xent_soft: labels must be contiguous int64 [{B}], got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    if labels_b is not None and (labels_b.dtype != labels.dtype or labels_b.shape != labels.shape
                                 or not labels_b.is_contiguous() or labels_b.device != labels.device):
        raise ValueError(f"xent_soft: labels_b must have the shape, dtype and device of labels "
                         f"({labels.dtype} {tuple(labels.shape)}), got {labels_b.dtype} "
                         f"{tuple(labels_b.shape)}")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"xent_soft: lam must lie in [0, 1], got {lam!r}")
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"xent_soft: eps (label smoothing) must lie in [0, 1), got {eps!r}")
    if dlog is not None:
        if dlog.dim() != 2 or dlog.shape[0] != B or dlog.shape[1] < K or not dlog.is_contiguous():
            raise ValueError(f"xent_soft: dlog must be contiguous [{B}, >= {K}], got {tuple(dlog.shape)}")
        if dlog.dtype not in ext.DT:
            raise ValueError(f"xent_soft: unsupported dlog dtype {dlog.dtype}")
    return B, K


def xent_soft(logits: torch.Tensor, labels: torch.Tensor, loss_rows, loss, labels_b=None,
              lam: float = 1.0, eps: float = 0.0, dlog=None, gscale: float = 1.0,
              gdev: Optional[torch.Tensor] = None) -> None:
    """:func:`xent` against the soft target q_k = eps/K + (1-eps) * (lam*[k==labels] +
    (1-lam)*[k==labels_b]) (label smoothing eps, mixup / CutMix weight lam; ``labels_b`` None:
    labels): loss_rows / loss = lse - sum_k q_k x_k, dlog = (softmax - q) * gscale * gdev[0]
    (csrc/mix.hip). Arguments are validated on the host first (:func:`xent_soft_check`)."""
    if loss_rows is None:
        raise ValueError("xent_soft: loss_rows is required (the kernel writes it on every launch)")
    lam, eps = float(lam), float(eps)
    B, K = xent_soft_check(logits, labels, labels_b, lam, eps, dlog)
    ld_out = dlog.shape[1] if dlog is not None else 0
    dt = dt_of(dlog) if dlog is not None else 1
    rc = ext.lib().pda_xent_soft(ptr(logits), B, K, logits.stride(0), ptr(labels), ptr(labels_b), lam,
                                 eps, ptr(loss_rows), ptr(loss), ptr(dlog), ld_out, float(gscale),
                                 ptr(gdev), dt, int(dlog is not None), stream(logits.device))
    check(rc, "xent_soft")


def topk_hits(logits, labels, hits) -> None:
    B, K = logits.shape
    rc = ext.lib().pda_topk(ptr(logits), B, K, logits.stride(0), ptr(labels), ptr(hits),
                            stream(logits.device))
    check(rc, "topk")


def col_sum(x, C_: int, out, scale: float = 1.0, accumulate: bool = False) -> None:
    rc = ext.lib().pda_col_sum(ptr(x), x.shape[0], C_, x.stride(0), float(scale), ptr(out), dt_of(x),
                               int(accumulate), stream(x.device))
    check(rc, "col_sum")


# ------------------------------------------------------------------ optimizer / amp
def sgd_flat(p, g, buf, shadow, lr, momentum, wd, initialized: bool, inv_scale=None,
             found_inf=None):
    """Fused SGD over the flat buffers; ``inv_scale`` / ``found_inf`` (device scalars published by
    :func:`amp_scan`) unscale the gradient and skip the whole update on overflow."""
    flags = (1 if initialized else 0) | (2 if shadow is not None else 0)
    dt = dt_of(shadow) if shadow is not None else 1
    rc = ext.lib().pda_sgd_flat(ptr(p), ptr(g), ptr(buf), ptr(shadow), p.numel(), float(lr),
                                float(momentum), float(wd), ptr(inv_scale), ptr(found_inf), flags, dt,
                                stream(p.device))
    check(rc, "sgd_flat")


def cast_flat(p, shadow) -> None:
    rc = ext.lib().pda_cast_flat(ptr(p), ptr(shadow), p.numel(), dt_of(shadow), stream(p.device))
    check(rc, "cast_flat")


def amp_scan(g, found_inf, inv_scale, scale, tracker, ws, growth=2.0, backoff=0.5,
             interval=2000) -> None:
    """One launch: found_inf = any non-finite in g; inv_scale = 1/scale; then (tracker given) the
    GradScaler update of scale/tracker -- all on the device, no host sync. ``ws``: int32[2] zeros
    (reset by the kernel itself)."""
    if g.numel() % 4 or g.dtype != torch.float32 or ws.dtype != torch.int32 or ws.numel() < 2:
        raise ValueError("amp_scan: f32 gradient with numel % 4 == 0 and an int32[2] workspace")
    check(ext.lib().pda_amp_scan(ptr(g), g.numel(), ptr(found_inf), ptr(inv_scale), ptr(scale),
                                 ptr(tracker), ptr(ws), float(growth), float(backoff), int(interval),
                                 stream(g.device)), "amp_scan")


# ------------------------------------------------------------------ segmented optimizer (csrc/optim.hip)
FLAT_CHUNK = 4096     # most elements one block of a flat-buffer kernel handles (csrc/common.h)
SEG_CHUNK = FLAT_CHUNK    # seg_norms / sgd_seg / grad_clip block rows
SEG_NESTEROV = 1      # SegRow.flags


_SEG_ERRORS = {-1: "bad counts or a missing buffer", -2: "a segment offset is negative or no multiple of 4",
               -3: "a segment is empty or ends past the flat buffer", -4: "segments overlap",
               -5: "a hyper-parameter is negative or not finite",
               -6: "the block table does not cover every segment exactly once in chunks of at most "
                   "SEG_CHUNK elements"}
_SEG_HYPER = ("lr", "momentum", "weight_decay", "lars", "lars_eps", "nesterov")


class SegTables:
    """Segment and block tables of the segmented optimizer: host rows (ctypes arrays, validated by the
    launchers before every launch) and their device copies (what the kernels read)."""

    def __init__(self, seg_host, blk_host, device) -> None:
        self.seg_host, self.blk_host = seg_host, blk_host
        self.nseg, self.nblocks = len(seg_host), len(blk_host)
        self.device = self.seg_dev = self.blk_dev = None    # device=None: host rows only
        if device is not None:
            self.device = torch.device(device)
            self.seg_dev = self._upload(seg_host)
            self.blk_dev = self._upload(blk_host)
            self.device = self.seg_dev.device     # with its index
        self.slab = None    # 2 doubles per block, allocated when a trust coefficient first needs it
        self.any_trust = any(r.trust > 0 for r in seg_host)   # seg_norms runs only then

    def _upload(self, rows) -> torch.Tensor:
        if len(rows) == 0:
            return torch.zeros(16, dtype=torch.uint8, device=self.device)
        return torch.frombuffer(rows, dtype=torch.uint8).to(self.device)

    def set_hyper(self, hyper) -> None:
        """New hyper-parameters for every segment: the host rows are rewritten and uploaded in stream
        order (a copy from pageable memory returns once the rows are staged)."""
        if len(hyper) != self.nseg:
            raise ValueError(f"seg_tables: {len(hyper)} hyper-parameter rows for {self.nseg} segments")
        for r, h in zip(self.seg_host, hyper):
            _fill_hyper(r, h)
        self.any_trust = any(r.trust > 0 for r in self.seg_host)
        if self.nseg and self.seg_dev is not None:
            self.seg_dev.copy_(torch.frombuffer(self.seg_host, dtype=torch.uint8))


def _fill_hyper(r: SegRow, h) -> None:
    unknown = set(h) - set(_SEG_HYPER)
    if unknown:
        raise ValueError(f"seg_tables: unknown hyper-parameter(s) {sorted(unknown)}")
    r.lr, r.momentum = float(h["lr"]), float(h.get("momentum", 0.0))
    r.wd, r.trust = float(h.get("weight_decay", 0.0)), float(h.get("lars", 0.0))
    r.eps = float(h.get("lars_eps", 1e-8))
    r.flags = SEG_NESTEROV if h.get("nesterov", False) else 0


def seg_tables(segments, hyper, device="cuda") -> Tuple[SegTables, int]:
    """Device tables of the segmented optimizer. ``segments``: one ``(offset, numel)`` per parameter
    tensor (elements of the flat buffer); ``hyper``: one dict per segment with ``lr`` and optionally
    ``momentum``, ``weight_decay``, ``nesterov``, ``lars`` (trust coefficient, 0 = off), ``lars_eps``.
    Every segment is cut into chunks of SEG_CHUNK elements, one block each. Returns (tables, number
    of blocks); the launchers validate the tables against the buffers they are launched on."""
    segments = [(int(o), int(n)) for o, n in segments]
    if len(segments) != len(hyper):
        raise ValueError(f"seg_tables: {len(hyper)} hyper-parameter rows for {len(segments)} segments")
    nblk = sum(max((n + SEG_CHUNK - 1) // SEG_CHUNK, 0) for _, n in segments)
    if nblk >= 2 ** 31:
        raise ValueError("seg_tables: more than 2^31 - 1 blocks")
    segs, blks = (SegRow * len(segments))(), (BlkRow * nblk)()
    b = 0
    for i, ((off, n), h) in enumerate(zip(segments, hyper)):
        r = segs[i]
        r.off, r.numel, r.blk0 = off, n, b
        _fill_hyper(r, h)
        for first in range(off, off + n, SEG_CHUNK):
            blks[b].first, blks[b].seg, blks[b].count = first, i, min(SEG_CHUNK, off + n - first)
            b += 1
        r.nblk = b - r.blk0
    return SegTables(segs, blks, device), nblk


def _seg_check(rc: int, what: str) -> None:
    if rc < 0:
        raise ValueError(f"{what}: {_SEG_ERRORS.get(rc, f'bad tables ({rc})')}")
    check(rc, what)


def _seg_flat(what: str, n: int, dev, **ts) -> None:
    if dev is None or dev.type != "cuda":
        raise ValueError(f"{what} runs on a GPU; the tables are on {dev}")
    for name, t in ts.items():
        if t is None:
            continue
        if t.device != dev or not t.is_contiguous() or t.numel() != n or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be a contiguous, 16-byte aligned tensor of {n} "
                             f"elements on {dev}")


def seg_norms(p, g, tables: SegTables) -> None:
    """Per-block sums of p^2 and g^2 (double) of every segment with a trust coefficient, into
    ``tables.slab``; :func:`sgd_seg` turns them into the LARS trust ratios."""
    _seg_flat("seg_norms", p.numel(), tables.device, p=p, g=g)
    if p.dtype != torch.float32 or g.dtype != torch.float32:
        raise ValueError("seg_norms: p and g are f32")
    if tables.slab is None or tables.slab.numel() < 2 * tables.nblocks:
        tables.slab = torch.zeros(max(2 * tables.nblocks, 2), dtype=torch.float64, device=tables.device)
    rc = ext.lib().pda_seg_norms(ptr(p), ptr(g), p.numel(), ptr(tables.seg_dev), ptr(tables.blk_dev),
                                 C.cast(tables.seg_host, C.c_void_p), C.cast(tables.blk_host, C.c_void_p),
                                 tables.nseg, tables.nblocks, ptr(tables.slab), stream(p.device))
    _seg_check(rc, "seg_norms")


def sgd_seg(p, g, buf, shadow, tables: SegTables, initialized: bool, inv_scale=None,
            found_inf=None) -> None:
    """SGD over the segments of ``tables`` (per-segment lr, momentum, weight decay, Nesterov and LARS
    trust ratio); ``inv_scale`` / ``found_inf`` as in :func:`sgd_flat`. Segments with a trust
    coefficient read the norms of a preceding :func:`seg_norms`. Elements in no segment stay."""
    n = p.numel()
    _seg_flat("sgd_seg", n, tables.device, p=p, g=g, buf=buf, shadow=shadow)
    if any(t.dtype != torch.float32 for t in (p, g, buf)):
        raise ValueError("sgd_seg: p, g and buf are f32")
    if shadow is not None and shadow.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("sgd_seg: the shadow is bf16 or fp16")
    if tables.any_trust and tables.slab is None:
        raise ValueError("sgd_seg: a trust coefficient needs seg_norms before the update")
    flags = (1 if initialized else 0) | (2 if shadow is not None else 0)
    dt = dt_of(shadow) if shadow is not None else 1
    rc = ext.lib().pda_sgd_seg(ptr(p), ptr(g), ptr(buf), ptr(shadow), n, ptr(tables.seg_dev),
                               ptr(tables.blk_dev), C.cast(tables.seg_host, C.c_void_p),
                               C.cast(tables.blk_host, C.c_void_p), tables.nseg, tables.nblocks,
                               ptr(tables.slab), ptr(inv_scale), ptr(found_inf), flags, dt,
                               stream(p.device))
    _seg_check(rc, "sgd_seg")


# ------------------------------------------------------------------ gradient clipping (csrc/clip.hip)
_CLIP_ERRORS = {-1: "no block rows or a missing buffer", -2: "a row start is negative or no multiple of 4",
                -3: "a row ends past the gradient", -4: "rows overlap",
                -5: "max_norm must be finite and > 0",
                -6: "a row's count lies outside [1, SEG_CHUNK]"}


def grad_clip(g, tables: SegTables, max_norm: float, slab, cnt, out, inv_scale=None,
              found_inf=None) -> None:
    """Global-norm gradient clipping, the device half (one launch, no host sync): over the block
    rows of ``tables`` (:func:`seg_tables`; elements of ``g`` in no row are never read),
    ``out[0] = inv * sqrt(sum g^2)`` -- the unscaled norm, summed in double in a fixed order -- and
    ``out[1] = inv * min(1, max_norm / (out[0] + 1e-6))`` in single precision, which the SGD
    launches take as their ``inv_scale``. ``inv = inv_scale[0]`` (1 when None); with ``found_inf``
    set ``out[1] = inv``. ``slab``: f64, one entry per block row; ``cnt``: one int32, zero (the
    kernel leaves it zero); ``out``: f32[2]. Bad arguments raise ValueError and launch nothing."""
    _seg_flat("grad_clip", g.numel(), tables.device, g=g)
    dev = tables.device
    if g.dtype != torch.float32:
        raise ValueError("grad_clip: g is f32")
    for name, t, dtype, least in (("slab", slab, torch.float64, tables.nblocks),
                                  ("cnt", cnt, torch.int32, 1), ("out", out, torch.float32, 2),
                                  ("inv_scale", inv_scale, torch.float32, 1),
                                  ("found_inf", found_inf, torch.float32, 1)):
        if t is None and name in ("inv_scale", "found_inf"):
            continue
        if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype
                or not t.is_contiguous() or t.numel() < least or t.data_ptr() % t.element_size()):
            raise ValueError(f"grad_clip: {name} must be a contiguous {dtype} tensor of at least "
                             f"{least} element(s) on {dev}")
    rc = ext.lib().pda_grad_clip(ptr(g), g.numel(), ptr(tables.blk_dev),
                                 C.cast(tables.blk_host, C.c_void_p), tables.nblocks, ptr(slab),
                                 ptr(cnt), float(max_norm), ptr(inv_scale), ptr(found_inf), ptr(out),
                                 stream(g.device))
    if rc < 0:
        raise ValueError(f"grad_clip: {_CLIP_ERRORS.get(rc, f'bad arguments ({rc})')}")
    check(rc, "grad_clip")


# ------------------------------------------------------------------ weight EMA (csrc/ema.hip)
EMA_CHUNK = FLAT_CHUNK                    # elements one block of the EMA kernel handles
EMA_LERP, EMA_COPY, EMA_SWAP = 0, 1, 2    # csrc/ema.hip EmaMode


_EMA_ERRORS = {-1: "bad mode or shadow dtype, or a missing e / p buffer",
               -2: "a range does not start 16-byte aligned (8-byte for the shadow)",
               -3: "a negative element count", -4: "e, p and shadow ranges overlap",
               -5: "w is not finite or lies outside [0, 1]"}


class EmaRanges:
    """A checked range table of :func:`ema_update`: ``ranges`` is a sequence of ``(e, p)`` or
    ``(e, p, shadow)`` tensors -- e and p contiguous f32 of one length on one GPU, the optional
    shadow bf16 or fp16 of that length. Built once, launched many times: the rows hold the tensors'
    addresses (and the tensors themselves, so they stay alive)."""

    def __init__(self, ranges) -> None:
        self.tensors = [tuple(r) + (None,) * (3 - len(r)) for r in ranges]
        self.rows = (EmaRange * len(self.tensors))()
        self.device, self.shadow_dtype = None, None
        for row, (e, p, sh) in zip(self.rows, self.tensors):
            for name, t in (("e", e), ("p", p)):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                    raise ValueError(f"ema_update: {name} is an f32 tensor, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)}")
            if sh is not None:
                if sh.dtype not in (torch.bfloat16, torch.float16):
                    raise ValueError("ema_update: the shadow is bf16 or fp16")
                if self.shadow_dtype not in (None, sh.dtype):
                    raise ValueError("ema_update: every shadow of one launch has the same dtype")
                self.shadow_dtype = sh.dtype
            if self.device is None:
                self.device = e.device
            for name, t in (("e", e), ("p", p), ("shadow", sh)):
                if t is None:
                    continue
                if t.device != self.device or not t.is_contiguous() or t.numel() != e.numel():
                    raise ValueError(f"ema_update: {name} must be a contiguous tensor of {e.numel()} "
                                     f"elements on {self.device}")
            row.e, row.p, row.shadow, row.count = ptr(e), ptr(p), ptr(sh), e.numel()
        if self.device is not None and self.device.type != "cuda":
            raise ValueError(f"ema_update runs on a GPU; the buffers are on {self.device}")


def ema_weight(w: float) -> float:
    """The float32 value of ``w`` the kernel computes with (NaN and out-of-range values pass through
    for the launcher to refuse)."""
    return C.c_float(float(w)).value


def ema_update(ranges, mode: int, w: float = 0.0) -> None:
    """One launch over ``ranges`` (an :class:`EmaRanges`, or the sequence it is built from):
    ``EMA_LERP`` e = fmaf(w, p - e, e) with the float32 ``w``; ``EMA_COPY`` e = p bit for bit;
    ``EMA_SWAP`` e and p exchange their bits and each given shadow receives the 16-bit cast of the
    new p. Elements outside the ranges stay; bad ranges raise ValueError and launch nothing."""
    if not isinstance(ranges, EmaRanges):
        ranges = EmaRanges(ranges)
    if mode not in (EMA_LERP, EMA_COPY, EMA_SWAP):
        raise ValueError(f"ema_update: mode is EMA_LERP, EMA_COPY or EMA_SWAP, got {mode!r}")
    if len(ranges.rows) == 0:
        return
    dt = dt_of(ranges.shadow_dtype) if ranges.shadow_dtype is not None else 1
    rc = ext.lib().pda_ema(ranges.rows, len(ranges.rows), int(mode), float(w), dt,
                           stream(ranges.device))
    if rc < 0:
        raise ValueError(f"ema_update: {_EMA_ERRORS.get(rc, f'bad ranges ({rc})')}")
    check(rc, "ema_update")


def pack_stem(src_ohwi, dst, Cout=64, RS=49, Cin=3, Cpad=8) -> None:
    Kpad = dst.shape[1]
    check(ext.lib().pda_pack_stem(ptr(src_ohwi), ptr(dst), Cout, RS, Cin, Cpad, Kpad, dt_of(dst),
                                  stream(dst.device)), "pack_stem")


# ------------------------------------------------------------------ data
def synth_salt(seed: int, split: str) -> int:
    from ..data.synthetic import SPLIT_ID
    return ((seed * 97 + SPLIT_ID[split]) * 0x632BE5AB) & 0xFFFFFFFF


def synth_batch(ids: torch.Tensor, seed: int, split: str, num_classes: int, S: int, out, labels,
                keys) -> None:
    B = ids.numel()
    check(ext.lib().pda_synth(ptr(ids), B, synth_salt(seed, split), num_classes, ptr(keys),
                              ptr(labels), S, ptr(out), dt_of(out), stream(out.device)), "synth")


# ------------------------------------------------------------------ stem (space-to-depth form)
def stem_s2d_geom(Nb: int, S: int) -> ConvGeom:
    """The 7x7/2/3 stem as a 4x4/1 conv with pad 2 on the 2x2 space-to-depth image (16 ch)."""
    return ConvGeom(Nb, S // 2, S // 2, 16, 64, 4, 4, 1, 2, ho=S // 2, wo=S // 2)


def synth_batch_s2d(ids, seed: int, split: str, num_classes: int, S: int, out, labels, keys) -> None:
    check(ext.lib().pda_synth_s2d(ptr(ids), ids.numel(), synth_salt(seed, split), num_classes,
                                  ptr(keys), ptr(labels), S, ptr(out), dt_of(out), stream(out.device)),
          "synth_s2d")


def nchw_to_s2d(x, out) -> None:
    B, C_, S, _ = x.shape
    check(ext.lib().pda_nchw_to_s2d(ptr(x), B, C_, S, ptr(out), dt_of(out), stream(x.device)),
          "nchw_to_s2d")


# ------------------------------------------------------------------ folder-image augmentation
AUG_S2D, AUG_NCHW = 0, 1
AUG_RGB, AUG_YUV420 = 0, 1          # source record format: HWC RGB | Y plane + half-resolution CbCr
AUG_MAX_SIDE = 32768               # csrc/batch_image.h S2D_MAX_SIDE
NCHW_MAX_SIDE = 26000              # ... NCHW_MAX_SIDE: 3*S*S < 2^31


def batch_layout(x) -> Optional[Tuple[int, int]]:
    """``(layout, S)`` of a model-ready batch: ``AUG_S2D`` [B, S/2, S/2, 16] or ``AUG_NCHW``
    [B, 3, S, S]; None for any other shape (no shape fits both)."""
    if x.dim() == 4 and x.shape[3] == 16 and x.shape[1] == x.shape[2]:
        return AUG_S2D, 2 * x.shape[1]
    if x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == x.shape[3]:
        return AUG_NCHW, x.shape[2]
    return None


_BATCH_SAYS = {"s2d": "s2d input must be [B, S/2, S/2, 16], got {shape}", "dtype": "unsupported dtype {dtype}",
               "nchw": "NCHW input must be [B, 3, S, S], got {shape}", "f32": "the NCHW layout is f32, got {dtype}",
               "even": "the image side must be even, got {S}", "contiguous": "x must be contiguous",
               "side": "empty batch or image side {S} out of range"}


def batch_shape(what: str, t, layout: int, B: Optional[int] = None, smin: int = 1, capped: bool = True,
                even: bool = False, contiguous: bool = True, says=None) -> Tuple[int, int]:
    """``(B, S)`` of the model-ready batch ``t`` in ``layout``, or ``ValueError("{what}: ...")``: shape
    (of ``B`` rows, when given), dtype, an ``even`` side, ``smin <= S`` (``capped``: <= the kernels'
    ``AUG_MAX_SIDE`` / ``NCHW_MAX_SIDE``), contiguity. ``says`` rewords refusals: a dict over the keys
    of ``_BATCH_SAYS``, or one string for all but the layout's. Pure Python: no library is loaded."""
    if layout not in (AUG_S2D, AUG_NCHW):
        raise ValueError(f"{what}: layout must be {AUG_S2D} (s2d) or {AUG_NCHW} (NCHW f32)")
    found = batch_layout(t)
    S = found[1] if found else 0

    def refuse(key):
        text = says if isinstance(says, str) else {**_BATCH_SAYS, **(says or {})}[key]
        raise ValueError(f"{what}: " + text.format(shape=tuple(t.shape), dtype=t.dtype, S=S))

    s2d = layout == AUG_S2D
    if found is None or found[0] != layout or (B is not None and t.shape[0] != B):
        refuse("s2d" if s2d else "nchw")
    if t.dtype not in ext.DT if s2d else t.dtype != torch.float32:
        refuse("dtype" if s2d else "f32")
    if even and S % 2:
        refuse("even")
    if t.shape[0] < 1 or S < smin or (capped and S > (AUG_MAX_SIDE if s2d else NCHW_MAX_SIDE)):
        refuse("side")
    if contiguous and not t.is_contiguous():
        refuse("contiguous")
    return t.shape[0], S


def aug_record_bytes(H: int, W: int, fmt: int) -> int:
    """Bytes of one HxW source record: ``3*H*W`` (RGB) or ``H*W + 2*Hc*Wc`` with ``Hc = (H+1)//2``,
    ``Wc = (W+1)//2`` (YCbCr 4:2:0)."""
    if fmt == AUG_RGB:
        return 3 * H * W
    if fmt == AUG_YUV420:
        return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
    raise ValueError(f"aug_resize: fmt must be {AUG_RGB} (rgb) or {AUG_YUV420} (yuv420), got {fmt!r}")


def aug_check(packed, table_i64, table_f64, out, layout: int, fmt: int = AUG_RGB) -> Tuple[int, int]:
    """Host-side validation of an :func:`aug_resize` call; returns (B, S). Pure Python on host
    tensors (the kernel library is not loaded), and run before anything is launched: the kernel
    (csrc/augment.hip) trusts every offset, size and box it is given. Each image is bounded by the
    record size of ``fmt`` (:func:`aug_record_bytes`)."""
    aug_record_bytes(1, 1, fmt)
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("aug_resize: packed must be a contiguous 1-D uint8 tensor")
    for name, t, dt in (("table_i64", table_i64, torch.int64), ("table_f64", table_f64, torch.float64)):
        if t.device.type != "cpu":
            raise ValueError(f"aug_resize: {name} is validated on the host and uploaded by the wrapper")
        if t.dtype != dt or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous():
            raise ValueError(f"aug_resize: {name} must be a contiguous [B, 4] {dt} tensor")
    B = table_i64.shape[0]
    if B < 1 or table_f64.shape[0] != B:
        raise ValueError("aug_resize: the tables must have the same B >= 1 rows")
    _, S = batch_shape("aug_resize", out, layout, B, smin=2, capped=False, even=True, says={
        "s2d": f"s2d output must be [{B}, S/2, S/2, 16], got {{shape}}",
        "nchw": f"NCHW output must be [{B}, 3, S, S], got {{shape}}",
        "dtype": "unsupported output dtype {dtype}", "f32": "the NCHW layout is f32",
        "even": "the output size must be even, got {S}",
        "side": "the output must be contiguous with S >= 2",
        "contiguous": "the output must be contiguous with S >= 2"})
    if out.device != packed.device:
        raise ValueError(f"aug_resize: output on {out.device}, packed images on {packed.device}")
    n = packed.numel()
    for b, ((off, H, W, _), box) in enumerate(zip(table_i64.tolist(), table_f64.tolist())):
        if not (1 <= H <= AUG_MAX_SIDE and 1 <= W <= AUG_MAX_SIDE):
            raise ValueError(f"aug_resize: image {b}: size {W}x{H} outside 1..{AUG_MAX_SIDE}")
        m = aug_record_bytes(H, W, fmt)
        if off < 0 or off + m > n:
            raise ValueError(f"aug_resize: image {b}: bytes [{off}, {off + m}) outside the "
                             f"packed buffer of {n}")
        x0, y0, x1, y1 = box
        if not all(math.isfinite(v) for v in box):
            raise ValueError(f"aug_resize: image {b}: non-finite box {box}")
        if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
            raise ValueError(f"aug_resize: image {b}: box {box} outside the {W}x{H} image")
    return B, S


def aug_resize(packed, table_i64, table_f64, out, layout: int = AUG_S2D, fmt: int = AUG_RGB) -> None:
    """Resample / flip / normalise a packed batch of raw uint8 images into ``out`` (one launch,
    csrc/augment.hip). ``packed``: device bytes; ``table_i64`` [B,4] = byte offset, H, W, flip and
    ``table_f64`` [B,4] = box x0, y0, x1, y1: HOST tensors (pinned ones upload asynchronously),
    validated by :func:`aug_check` before the launch. ``fmt``: the records are HWC RGB
    (``AUG_RGB``) or a Y plane followed by the interleaved half-resolution CbCr plane
    (``AUG_YUV420``, decoded inside the kernel)."""
    from ..data.synthetic import MEAN, STD
    B, S = aug_check(packed, table_i64, table_f64, out, layout, fmt)
    if packed.device.type != "cuda":
        raise ValueError("aug_resize runs on a GPU; the packed images are on " + str(packed.device))
    if out.data_ptr() % 16:
        raise ValueError("aug_resize: the output must be 16-byte aligned")
    ti = table_i64.to(packed.device, non_blocking=True)
    tf = table_f64.to(packed.device, non_blocking=True)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    check(ext.lib().pda_aug_resize_fmt(ptr(packed), ptr(ti), ptr(tf), B, S, ptr(out), dt_of(out), layout,
                                       fmt, mean, std, stream(out.device)), "aug_resize")


# ------------------------------------------------------------------ mixup / CutMix of a batch
MIX_MIXUP, MIX_CUTMIX = 0, 1


def mix_weights(lam: float) -> Tuple[float, float]:
    """(lam, 1 - lam) as the float32 values :func:`batch_mix` hands its kernel: lam rounded to
    float32, and one float32 subtraction from 1."""
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]
    lam32 = f32(float(lam))
    return lam32, f32(1.0 - lam32)


def batch_mix_check(x, out, layout: int, mode: int, lam: float, box=None) -> Tuple[int, int, tuple]:
    """Host-side validation of a :func:`batch_mix` call; returns (B, S, box). Pure Python (the
    kernel library is not loaded), run before the launch: the kernel trusts the shape and the box."""
    B, S = batch_shape("batch_mix", x, layout, contiguous=False)      # (contiguity: with out, below)
    if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
        raise ValueError(f"batch_mix: out must have the shape, dtype and device of x "
                         f"({tuple(x.shape)} {x.dtype} {x.device}), got {tuple(out.shape)} {out.dtype} "
                         f"{out.device}")
    if not x.is_contiguous() or not out.is_contiguous():
        raise ValueError("batch_mix: x and out must be contiguous")
    nbytes = x.numel() * x.element_size()
    if x.device.type != "meta" and (x.data_ptr() < out.data_ptr() + nbytes
                                    and out.data_ptr() < x.data_ptr() + nbytes):
        raise ValueError("batch_mix: out overlaps x (sample b reads sample b-1: it runs out of place)")
    if mode not in (MIX_MIXUP, MIX_CUTMIX):
        raise ValueError(f"batch_mix: mode must be {MIX_MIXUP} (mixup) or {MIX_CUTMIX} (CutMix)")
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"batch_mix: lam must lie in [0, 1], got {lam!r}")
    if mode == MIX_CUTMIX:
        if box is None or len(box) != 4 or any(int(v) != v for v in box):
            raise ValueError(f"batch_mix: CutMix needs an integer box (y1, y2, x1, x2), got {box!r}")
        y1, y2, x1, x2 = (int(v) for v in box)
        if not (0 <= y1 <= y2 <= S and 0 <= x1 <= x2 <= S):
            raise ValueError(f"batch_mix: box rows [{y1}, {y2}) columns [{x1}, {x2}) outside the "
                             f"{S}x{S} image")
        box = (y1, y2, x1, x2)
    else:
        box = (0, 0, 0, 0)
    return B, S, box


def batch_mix(x, out, layout: int, mode: int, lam: float, box=None) -> None:
    """Mix every sample of a finished batch with the one above it (sample 0 with the last;
    torchvision's ``roll(1, 0)``) into ``out`` (one launch, csrc/mix.hip). ``layout``: ``AUG_S2D``
    [B, S/2, S/2, 16] (f32 / bf16 / f16) or ``AUG_NCHW`` [B, 3, S, S] f32. ``MIX_MIXUP``: out =
    lam*x + (1-lam)*partner, in f32 with one rounding; ``MIX_CUTMIX``: pixels with y1 <= y < y2 and
    x1 <= x < x2 (``box`` = (y1, y2, x1, x2)) take the partner's bits, every other x's."""
    lam = float(lam)
    B, S, box = batch_mix_check(x, out, layout, mode, lam, box)
    if x.device.type != "cuda":
        raise ValueError("batch_mix runs on a GPU; the batch is on " + str(x.device))
    if x.data_ptr() % 16 or out.data_ptr() % 16:
        raise ValueError("batch_mix: x and out must be 16-byte aligned")
    lam32, oml32 = mix_weights(lam)
    check(ext.lib().pda_batch_mix(ptr(x), ptr(out), B, S, dt_of(x), layout, mode, lam32, oml32, *box,
                                  0, stream(x.device)), "batch_mix")


# ------------------------------------------------------------------ random erasing of a batch
ERASE_SCALE, ERASE_RATIO = (0.02, 0.33), (0.3, 3.3)      # torchvision's RandomErasing defaults


def erase_bounds(p: float, scale, ratio) -> Tuple[float, float, float, float, float]:
    """``(p, s0, s1, l0, l1)`` of a random-erasing draw, validated: the probability, the scale
    bounds and the LOGARITHMS of the ratio bounds, as ``pda_erase_draw`` takes them (and as
    ``erase.draw_erase`` evaluates them: one ``math.log`` per bound, on the host)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"erase_draw: p must be a probability in [0, 1], got {p!r}")
    if len(scale) != 2 or len(ratio) != 2:
        raise ValueError(f"erase_draw: scale {scale!r} and ratio {ratio!r} must be (low, high) pairs")
    s0, s1, r0, r1 = float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1])
    if not (math.isfinite(s0) and math.isfinite(s1) and 0.0 <= s0 <= s1):
        raise ValueError(f"erase_draw: scale {scale!r} must be finite, >= 0 and ascending")
    if not (math.isfinite(r0) and math.isfinite(r1) and 0.0 < r0 <= r1):
        raise ValueError(f"erase_draw: ratio {ratio!r} must be finite, > 0 and ascending")
    return p, s0, s1, math.log(r0), math.log(r1)


def _erase_table_check(what: str, boxes, B: Optional[int] = None) -> int:
    if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous():
        raise ValueError(f"{what}: boxes must be a contiguous int32 [B, 4] tensor, got "
                         f"{tuple(boxes.shape)} {boxes.dtype}")
    if boxes.shape[0] < 1 or (B is not None and boxes.shape[0] != B):
        raise ValueError(f"{what}: boxes has {boxes.shape[0]} rows for a batch of {B if B is not None else '>= 1'}")
    return boxes.shape[0]


def erase_draw(boxes, S: int, bkey: int, p: float, scale=ERASE_SCALE, ratio=ERASE_RATIO) -> None:
    """Draw the random-erasing boxes of a batch on the device (one launch, csrc/erase.hip
    ``erase_draw_kernel``) into ``boxes``, a device int32 [B, 4] table: row b = (y1, y2, x1, x2),
    half-open, of the sample at batch position b, all zeros when it is left alone. ``bkey``:
    ``erase.batch_key(seed, rank, epoch, step)``; ``erase.draw_erase`` is the host mirror."""
    B = _erase_table_check("erase_draw", boxes)
    p, s0, s1, l0, l1 = erase_bounds(p, scale, ratio)
    if int(S) != S or not 1 <= S <= AUG_MAX_SIDE:
        raise ValueError(f"erase_draw: image side {S!r} outside 1..{AUG_MAX_SIDE}")
    if boxes.device.type != "cuda":
        raise ValueError("erase_draw runs on a GPU; the table is on " + str(boxes.device))
    if boxes.data_ptr() % 4:
        raise ValueError("erase_draw: boxes must be 4-byte aligned")
    check(ext.lib().pda_erase_draw(B, int(S), int(bkey) & 0xFFFFFFFF, p, s0, s1, l0, l1, ptr(boxes),
                                   stream(boxes.device)), "erase_draw")


def batch_erase_check(x, boxes, layout: int) -> Tuple[int, int]:
    """Host-side validation of a :func:`batch_erase` call; returns (B, S). Pure Python (the kernel
    library is not loaded), run before the launch. The table's VALUES are not read: the kernel
    clamps every box to the image."""
    B, S = batch_shape("batch_erase", x, layout)
    _erase_table_check("batch_erase", boxes, B)
    if boxes.device != x.device:
        raise ValueError(f"batch_erase: boxes on {boxes.device}, the batch on {x.device}")
    return B, S


def batch_erase(x, boxes, layout: int) -> None:
    """Set the pixels inside each sample's box to +0.0, in place (one launch, csrc/erase.hip).
    ``layout``: ``AUG_S2D`` [B, S/2, S/2, 16] (f32 / bf16 / f16) or ``AUG_NCHW`` [B, 3, S, S] f32;
    ``boxes``: device int32 [B, 4] rows (y1, y2, x1, x2), half-open, as :func:`erase_draw` writes
    them. Every bit outside the boxes stays, the s2d padding slots included."""
    B, S = batch_erase_check(x, boxes, layout)
    if x.device.type != "cuda":
        raise ValueError("batch_erase runs on a GPU; the batch is on " + str(x.device))
    if x.data_ptr() % 16 or boxes.data_ptr() % 4:
        raise ValueError("batch_erase: x must be 16-byte aligned (boxes 4-byte)")
    check(ext.lib().pda_batch_erase(ptr(x), ptr(boxes), B, S, dt_of(x), layout, 0, stream(x.device)),
          "batch_erase")


AUG_TRAIN, AUG_VAL = 0, 1


def aug_draw(ids, index_dev, N: int, seed: int, split: str, epoch: int, mode: int, S: int,
             resize: int = 0, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), batch_off=None):
    """Crop boxes, flips and labels of the samples ``ids`` of a packed dataset, drawn on the device
    (one launch, csrc/augment.hip ``aug_draw_kernel``): returns device ``(ti [B,4] int64 = byte
    offset, H, W, flip; tf [B,4] float64 = x0, y0, x1, y1; labels [B] int64)``, the tables of
    :func:`aug_resize_dev`.

    ``ids``: HOST int64 [B], checked here against ``N`` and uploaded (pinned ones asynchronously);
    ``index_dev``: device int64 [N,4] = byte offset, H, W, label, validated when the file was opened
    (``data.packed.PackedImages``); ``batch_off``: device int64 [B] byte offsets that replace the
    index's (host residency). ``mode`` ``AUG_TRAIN``: ``data.folder.train_crop_params`` with
    uniforms that are a pure function of (seed, split, epoch, id); ``AUG_VAL``:
    ``val_crop_params(W, H, S, resize)``."""
    from ..data.synthetic import SPLIT_ID
    if ids.device.type != "cpu" or ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("aug_draw: ids must be a contiguous host int64 [B] tensor (checked on the host)")
    B = ids.numel()
    if B < 1:
        raise ValueError("aug_draw: empty batch")
    if index_dev.device.type != "cuda":
        raise ValueError(f"aug_draw runs on a GPU; the index is on {index_dev.device}")
    if (index_dev.dtype != torch.int64 or index_dev.dim() != 2 or index_dev.shape[1] != 4
            or not index_dev.is_contiguous() or index_dev.shape[0] != N or N < 1):
        raise ValueError(f"aug_draw: the index must be a contiguous device int64 [{N}, 4] tensor")
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= N:
        raise ValueError(f"aug_draw: sample ids span [{lo}, {hi}], outside the {N} records")
    if batch_off is not None and (batch_off.device != index_dev.device or batch_off.dtype != torch.int64
                                  or batch_off.shape != (B,) or not batch_off.is_contiguous()):
        raise ValueError(f"aug_draw: batch_off must be a contiguous int64 [{B}] tensor on {index_dev.device}")
    if split not in SPLIT_ID:
        raise ValueError(f"aug_draw: split must be one of {sorted(SPLIT_ID)}, got {split!r}")
    if mode not in (AUG_TRAIN, AUG_VAL) or S < 2 or epoch < 0:
        raise ValueError(f"aug_draw: mode {mode}, S {S}, epoch {epoch}")
    s0, s1, r0, r1 = float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1])
    if mode == AUG_TRAIN and not (0.0 < s0 <= s1 <= 1.0 and 1e-3 <= r0 <= r1 <= 1e3):
        raise ValueError(f"aug_draw: scale {scale} must lie in (0, 1] and ratio {ratio} in [1e-3, 1e3], "
                         "both ascending")
    if mode == AUG_VAL and not S <= resize <= 65536:
        raise ValueError(f"aug_draw: val mode resizes to {resize}, below the crop size {S} (or above 65536)")
    dev = index_dev.device
    ti = torch.empty(B, 4, dtype=torch.int64, device=dev)
    tf = torch.empty(B, 4, dtype=torch.float64, device=dev)
    labels = torch.empty(B, dtype=torch.int64, device=dev)
    ids_dev = ids.to(dev, non_blocking=True)
    check(ext.lib().pda_aug_draw(ptr(ids_dev), ptr(index_dev), ptr(batch_off), B, N,
                                 seed & 0xFFFFFFFF, SPLIT_ID[split], epoch & 0xFFFFFFFF, mode, S,
                                 int(resize), s0, s1, r0, r1, ptr(ti), ptr(tf), ptr(labels),
                                 stream(dev)), "aug_draw")
    return ti, tf, labels


def aug_resize_dev(packed, ti_dev, tf_dev, out, layout: int = AUG_S2D, fmt: int = AUG_RGB) -> None:
    """:func:`aug_resize` on DEVICE tables that :func:`aug_draw` wrote from a validated index (the
    kernel trusts them; nothing is read back): resample / flip / normalise into ``out``. ``fmt`` is
    the record format the index was validated for."""
    from ..data.synthetic import MEAN, STD
    aug_record_bytes(1, 1, fmt)
    if packed.device.type != "cuda":
        raise ValueError("aug_resize_dev runs on a GPU; the packed images are on " + str(packed.device))
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("aug_resize_dev: packed must be a contiguous 1-D uint8 tensor")
    for name, t, dt in (("ti_dev", ti_dev, torch.int64), ("tf_dev", tf_dev, torch.float64)):
        if t.device != packed.device or out.device != packed.device:
            raise ValueError(f"aug_resize_dev: {name} and the output must be on {packed.device}")
        if t.dtype != dt or t.dim() != 2 or t.shape[1] != 4 or not t.is_contiguous():
            raise ValueError(f"aug_resize_dev: {name} must be a contiguous [B, 4] {dt} tensor")
    B = ti_dev.shape[0]
    if B < 1 or tf_dev.shape[0] != B:
        raise ValueError("aug_resize_dev: the tables must have the same B >= 1 rows")
    unfit = (f"output {{shape}} {{dtype}} does not fit layout {layout} for {B} images (even S >= 2, "
             f"contiguous, 16-byte aligned)")
    _, S = batch_shape("aug_resize_dev", out, layout, B, smin=2, capped=False, even=True, says=unfit)
    if out.data_ptr() % 16:
        raise ValueError("aug_resize_dev: " + unfit.format(shape=tuple(out.shape), dtype=out.dtype))
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    check(ext.lib().pda_aug_resize_fmt(ptr(packed), ptr(ti_dev), ptr(tf_dev), B, S, ptr(out), dt_of(out),
                                       layout, fmt, mean, std, stream(out.device)), "aug_resize_dev")


def pack_stem_s2d(src_ohwi, dst) -> None:
    check(ext.lib().pda_pack_stem_s2d(ptr(src_ohwi), ptr(dst), dst.shape[0], dt_of(dst),
                                      stream(dst.device)), "pack_stem_s2d")


def stem_s2d_grad(gpacked, grad_ohwi, accumulate: bool = False) -> None:
    check(ext.lib().pda_stem_s2d_grad(ptr(gpacked), ptr(grad_ohwi), gpacked.numel() // 256,
                                      int(accumulate), stream(gpacked.device)), "stem_s2d_grad")
