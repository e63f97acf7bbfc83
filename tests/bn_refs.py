"""References and exact-data case builders for the stand-alone train-time BatchNorm kernels of
csrc/bn.hip (tests/test_bn_kernels_gpu.py).

The operations are written from the formulas in the header of bn.hip as plain torch arithmetic on
the CPU, generic in the dtype of their arguments: float64 is the reference, float32 the proof of
the builders' premise. No kernel of this project and no GPU result enters them;
tests/test_bn_refs_cpu.py checks them against torch autograd and torch's own statistics.

The case builders produce *exact* data: activations, gradients and coefficients are small dyadic
values (integers, quarter steps, power-of-two scales, shifts on a 1/256 grid), so every f32
product, fma and sum a kernel may form is exact in any order and its result must equal the float64
reference rounded once to the storage dtype, bit for bit. Each builder proves that on the CPU
(float32 evaluation == float64 evaluation; sums: sum |term| / quantum < 2^24) and asserts that its
data hits what a kernel gets wrong: ``pre == 0`` in more than 5 % of the elements (the ReLU mask is
``pre > 0``) and exact 16-bit rounding ties in the output. Cases are cached: treat as read-only.
"""
import functools
import math

import numpy as np
import torch

from head_refs import EPS32, F64, _gen, quantised, to_dtype, ulp_out, within_ulp  # noqa: F401

F32 = torch.float32
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
DT16 = (torch.bfloat16, torch.float16)
_PICK = torch.tensor([0.5, 1.0, 2.0], dtype=F64)


def f32c(x: float) -> float:
    """A Python float as the kernel's ``float`` argument sees it."""
    return float(np.float32(x))


def representable(t64: torch.Tensor, dtypes=(torch.bfloat16, torch.float16, torch.float32)) -> bool:
    return all(torch.equal(t64.to(d).to(F64), t64) for d in dtypes)


def ties(ref64: torch.Tensor, dtype: torch.dtype, delta: float = 2.0 ** -16) -> torch.Tensor:
    """Elements of ``ref64`` exactly half-way between two neighbours of ``dtype`` (``delta``: far
    below half a spacing of every value, exact to add in float32)."""
    return to_dtype(ref64 + delta, dtype) != to_dtype(ref64 - delta, dtype)


def mask_bytes(v: torch.Tensor) -> torch.Tensor:
    """bn_apply's ReLU bitmask: one byte per 8 elements, bit e = (element 8i+e > 0)."""
    b = (v.reshape(-1, 8) > 0).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


# ------------------------------------------------------------------ the operations
def apply_pre(y, sc, sh, mode: int, r2=None, sc2=None, sh2=None):
    """mode 0: bn(y); 1: bn(y) + res; 2: bn(y) + bn2(y2) -- before the activation."""
    v = y * sc + sh
    if mode == 1:
        v = v + r2
    elif mode == 2:
        v = v + (r2 * sc2 + sh2)
    return v


def apply_ref(y, sc, sh, mode: int, relu: bool, r2=None, sc2=None, sh2=None):
    v = apply_pre(y, sc, sh, mode, r2, sc2, sh2)
    return v.clamp_min(0) if relu else v


def grad_ref(rows: int, g1=None, g2=None, gp=None, HW: int = 0):
    """The incoming gradient dA [rows][C]: g1 (+ g2), or the pooled gp[row // HW] / HW."""
    if gp is not None:
        return gp.repeat_interleave(HW, 0)[:rows] / HW
    return g1 if g2 is None else g1 + g2


def dz_ref(dA, mode: int, pre=None):
    """dz = dA where the forward's pre-activation was > 0 (modes 0-2); mode 3: no mask."""
    return dA if mode == 3 else torch.where(pre > 0, dA, torch.zeros_like(dA))


def block_rows(rows: int, G: int):
    """Row range of each of the G blocks: rows_per_block = ceil(rows / G); blocks past the rows
    own none."""
    rpb = -(-rows // G)
    return [(min(rows, b * rpb), min(rows, (b + 1) * rpb)) for b in range(G)]


def partials_ref(dz, y, y2, G: int, absolute: bool = False):
    """[G][nq][C]: q0 = sum dz, q1 = sum dz*y, q2 = sum dz*y2 (nq = 3 when y2 is given) over each
    block's rows. ``absolute``: sums of |term| (the summation bounds)."""
    terms = [dz, dz * y] + ([dz * y2] if y2 is not None else [])
    if absolute:
        terms = [t.abs() for t in terms]
    out = torch.zeros(G, len(terms), dz.shape[1], dtype=dz.dtype)
    for b, (r0, r1) in enumerate(block_rows(dz.shape[0], G)):
        for q, t in enumerate(terms):
            out[b, q] = t[r0:r1].sum(0)
    return out


def bwd_finalize_ref(sdz, sdzy, gamma, mean, invstd, count: float, gscale: float):
    """Totals (float64) -> the gamma / beta gradient terms and the apply coefficients of
    dy = k1*dz + k2*y + k3, in float64. ``k3_extra``: the cancellation allowance of k3."""
    mu, is_, ga = mean.to(F64), invstd.to(F64), gamma.to(F64)
    gs = f32c(gscale)
    sdzx = (sdzy - mu * sdz) * is_                      # sum dz * xhat
    a = ga * is_
    kk2 = -a * is_ * sdzx / count
    t1, t2 = -a * sdz / count, kk2 * mu
    return dict(dgamma=sdzx * gs, dbeta=sdz * gs, k1=a, k2=kk2, k3=t1 - t2,
                k3_extra=2.0 ** -50 * (t1.abs() + t2.abs()))


def bwd_apply_ref(dz, y, k1, k2, k3):
    return k1 * dz + (k2 * y + k3)


def fwd_tile_rows(T: int, bm: int, M: int) -> torch.Tensor:
    return torch.tensor([min(bm, M - t * bm) for t in range(T)], dtype=F64)[:, None]


def fwd_totals_ref(part, bm: int, M: int):
    """[2][C] (sum y, sum y^2) from shifted per-tile partials part[T][3][C] = (sum (y-s),
    sum (y-s)^2, s) over tiles of bm rows, the last one ragged."""
    p = part.to(F64)
    r = fwd_tile_rows(p.shape[0], bm, M)
    x, d1, s = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([(r * s + x).sum(0), (d1 + s * (2 * x + r * s)).sum(0)])


def fwd_finalize_ref(tot, count: float, eps: float):
    """mean, clamped biased variance, invstd, unbiased variance (the biased one at count 1) and
    the cancellation allowance of invstd, all float64."""
    mean = tot[0] / count
    ex2 = tot[1] / count
    var = (ex2 - mean * mean).clamp_min(0)
    e = f32c(eps)
    inv = 1.0 / torch.sqrt(var + e)
    unb = var * count / (count - 1.0) if count > 1 else var
    inv_extra = 0.5 * inv * 2.0 ** -50 * (ex2.abs() + mean * mean) / (var + e)
    return dict(mean=mean, var=var, invstd=inv, unb=unb, inv_extra=inv_extra)


# ------------------------------------------------------------------ exact cases: apply / reduce
def _coeffs(C: int, g: torch.Generator, fine: bool = True):
    """scale in {1/2, 1, 2}; even channels: shift = -scale * y0 with y0 a quarter step (so bn(y0)
    is exactly 0); odd channels (``fine``): shift = 8 + an odd multiple of 1/256 (c % 4 == 1) or
    of 1/32 (c % 4 == 3) within +-1 -- y * scale is a multiple of 1/8, so an output in [8, 16)
    keeps its lowest bit at 2^-8 (12 significant bits: a tie in fp16) or 2^-5 (9: a tie in bf16);
    otherwise quarter steps."""
    sc = _PICK[torch.randint(0, 3, (C,), generator=g)]
    y0 = quantised((C,), 0.25, 1.0, g)
    c = torch.arange(C)
    f16 = quantised((C,), 1.0 / 128, 1.0, g) + 1.0 / 256 + 8.0
    b16 = quantised((C,), 1.0 / 16, 1.0, g) + 1.0 / 32 + 8.0
    odd = torch.where(c % 4 == 1, f16, b16) if fine else quantised((C,), 0.25, 1.0, g)
    even = c % 2 == 0
    return sc, torch.where(even, -sc * y0, odd), y0, even


def _hits(rows: int, C: int) -> torch.Tensor:
    """Elements forced to pre == 0: even channels, every third (row + pair) -- one in six."""
    r, c = torch.arange(rows)[:, None], torch.arange(C)[None, :]
    return (c % 2 == 0) & ((r + c // 2) % 3 == 0)


@functools.lru_cache(maxsize=None)
def bn_case(rows: int, C: int, mode: int) -> dict:
    """Exact inputs of bn_apply / bn_bwd_reduce / bn_bwd_apply at [rows][C] for one mask mode, the
    float64 pre-activation, gradients (g1, g2, and gp for HW = 1 and 49) and dyadic apply
    coefficients k[6][C]."""
    assert C % 8 == 0
    g = _gen(100000 * mode + 1000 * rows + C)
    y = quantised((rows, C), 0.25, 4.0, g)
    sc, sh, y0, even = _coeffs(C, g)
    hit = _hits(rows, C)
    d = dict(mode=mode, rows=rows, C=C, sc=sc, sh=sh, r2=None, sc2=None, sh2=None)
    if mode in (0, 3):
        y = torch.where(hit, y0.expand(rows, C), y)
    else:
        r2 = quantised((rows, C), 0.25, 4.0, g)
        if mode == 1:
            r2 = torch.where(hit, -(y * sc + sh), r2)
        else:
            sc2, sh2, y02, _ = _coeffs(C, g, fine=False)
            sc2 = torch.where(even, sc, sc2)
            sh2 = torch.where(even, -sc2 * y02, sh2)
            r2 = torch.where(hit, y02 - (y - y0), r2)
            d.update(sc2=sc2, sh2=sh2)
        d["r2"] = r2
        assert representable(r2)
    d["y"] = y
    assert representable(y) and representable(sc) and representable(sh, (F32,))
    pre = apply_pre(y, sc, sh, min(mode, 2) if mode != 3 else 0, d["r2"], d["sc2"], d["sh2"])
    d["pre"] = pre
    f = {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    pre32 = apply_pre(f["y"], f["sc"], f["sh"], 0 if mode == 3 else mode, f["r2"], f["sc2"], f["sh2"])
    assert pre32.dtype == F32 and torch.equal(pre32.to(F64), pre), "apply is not exact in f32"
    if mode != 3:
        share = float((pre == 0).double().mean())
        assert share > 0.05, f"pre == 0 in only {share:.1%} of the elements"
    for dt in DT16:
        if rows * C >= 64:
            assert bool(ties(pre, dt).any()) and bool(ties(pre.clamp_min(0), dt).any()), dt
    # gradients: quarter steps; the pooled forms per HW
    d["g1"] = quantised((rows, C), 0.25, 2.0, g)
    d["g2"] = quantised((rows, C), 0.25, 2.0, g)
    d["gp"] = {HW: quantised((-(-rows // HW), C), 0.25, 2.0, g) for HW in (1, 49)}
    # dyadic coefficients of dy = k1*dz + k2*y + k3 (two branches)
    k = torch.stack([_PICK[torch.randint(0, 3, (C,), generator=g)] * s if i % 3 < 2
                     else quantised((C,), 1.0 / 64, 1.0, g) for i, s in
                     enumerate((1.0, -0.25, 0, 1.0, 0.125, 0))])
    d["k"] = k
    assert representable(k, (F32,))
    for b, ys in ((0, y), (1, d["r2"] if mode == 2 else y)):
        dz = d["g1"] + d["g2"]
        dy = bwd_apply_ref(dz, ys, *k[3 * b:3 * b + 3])
        dy32 = bwd_apply_ref(dz.float(), ys.float(), *k[3 * b:3 * b + 3].float())
        assert torch.equal(dy32.to(F64), dy), "dy = k1*dz + k2*y + k3 is not exact in f32"
    return d


GRAD_FORMS = ("g1", "g1+g2", "gp1", "gp49")


@functools.lru_cache(maxsize=None)
def reduce_case(rows: int, C: int, mode: int, form: str) -> dict:
    """bn_case plus the gradient form: dA, dz, the terms' exactness (forms without 1/49) or the
    float32 model of the kernel's dA = gp * (1.f / HW) held to the ulp bound (gp49)."""
    d = dict(bn_case(rows, C, mode))
    HW = {"gp1": 1, "gp49": 49}.get(form, 0)
    g1 = d["g1"] if HW == 0 else None
    g2 = d["g2"] if form == "g1+g2" else None
    gp = d["gp"][HW] if HW else None
    dA = grad_ref(rows, g1, g2, gp, HW)
    dz = dz_ref(dA, mode, d["pre"])
    y2 = d["r2"] if mode == 2 else None
    d.update(HW=HW, g1=g1, g2=g2, gp=gp, dz=dz, y2=y2, exact=form != "gp49")
    if d["exact"]:
        assert representable(dz)
        p1 = partials_ref(dz, d["y"], y2, 1)
        p32 = partials_ref(dz.float(), d["y"].float(), None if y2 is None else y2.float(), 1)
        assert torch.equal(p32.to(F64), p1), "partial sums are not exact in f32"
        # every term is a multiple of 2^-4: exact in any order while sum |term| / 2^-4 < 2^24
        assert float(partials_ref(dz, d["y"], y2, 1, absolute=True).max()) * 16 < 2 ** 24
    else:
        inv = np.float32(1.0) / np.float32(HW)
        got = gp.float().repeat_interleave(HW, 0)[:rows] * torch.tensor(inv)
        ok, _ = within_ulp(got, dA, F32)
        assert bool(ok.all()), "f32 gp * (1.f / HW) is outside one f32 spacing of gp / HW"
    return d


def tiled_case(block: int, rows: int, C: int, mode: int):
    """(bn_case(block, C, mode), the row of it that each of ``rows`` rows repeats): the large apply
    case, whose data and reference are the small block, tiled."""
    return bn_case(block, C, mode), torch.arange(rows) % block


# ------------------------------------------------------------------ exact cases: statistics
@functools.lru_cache(maxsize=None)
def bwd_stats_case(T: int, C: int, nq: int, dyadic: bool) -> dict:
    """Integer partials part[T][nq][C] (every f64 sum exact in any order) with generic or dyadic
    per-channel gamma / mean / invstd of both branches and non-zero old gradients."""
    g = _gen(7919 * T + 31 * C + nq + (5 if dyadic else 0))
    part = torch.randint(-8, 9, (T, nq, C), generator=g).to(F64)
    assert float(part.abs().sum(0).max()) < 2 ** 24
    d = dict(part=part, tot=part.sum(0))
    for b in range(nq - 1):
        if dyadic:
            ga = _PICK[torch.randint(0, 3, (C,), generator=g)]
            mu = quantised((C,), 0.25, 2.0, g)
            is_ = torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=F64)[torch.randint(0, 4, (C,), generator=g)]
        else:
            ga = (torch.rand(C, generator=g) + 0.5).to(F64)
            mu = torch.randn(C, generator=g).to(F64)
            is_ = (torch.rand(C, generator=g) * 3 + 0.25).to(F64)
        d[b] = dict(gamma=ga, mean=mu, invstd=is_,
                    dgamma=(torch.randn(C, generator=g) * 50).to(F64),
                    dbeta=(torch.randn(C, generator=g) * 50).to(F64))
        assert all(representable(v, (F32,)) for v in d[b].values())
    return d


@functools.lru_cache(maxsize=None)
def fwd_stats_case(T: int, C: int, bm: int, M: int) -> dict:
    """Integer shifted partials part[T][3][C] of valid tile moments (sum (y-s)^2 >= (sum (y-s))^2
    / rows in every tile, so the total variance is >= 0), totals, and generic gamma / beta /
    running statistics."""
    assert (T - 1) * bm < M <= T * bm
    g = _gen(104729 * T + 131 * C + M)
    r = fwd_tile_rows(T, bm, M)
    x = torch.randint(-50, 51, (T, C), generator=g).to(F64)
    x = torch.minimum(x.abs(), 8 * r).copysign(x)
    d1 = x * x + torch.randint(0, 101, (T, C), generator=g).to(F64)
    if M == 1:
        d1 = x * x                                   # one sample: its moments are its own
    s = torch.randint(-3, 4, (T, C), generator=g).to(F64)
    part = torch.stack([x, d1, s], 1)
    tot = fwd_totals_ref(part, bm, M)
    assert float((r * s.abs() + x.abs()).sum(0).max()) < 2 ** 24
    assert float((d1 + s.abs() * (2 * x.abs() + r * s.abs())).sum(0).max()) < 2 ** 24
    return dict(part=part, tot=tot, **stat_params(C, g))


def stat_params(C: int, g: torch.Generator) -> dict:
    return dict(gamma=(torch.rand(C, generator=g) + 0.5).to(F64),
                beta=torch.randn(C, generator=g).to(F64),
                rmean=torch.randn(C, generator=g).to(F64),
                rvar=(torch.rand(C, generator=g) + 0.5).to(F64))


def fwd_checks(got: dict, tot, count: float, p: dict, eps: float, momentum: float, update: bool):
    """Failures (strings) of the finalized forward statistics ``got`` (float32 CPU tensors mean,
    invstd, scale, shift, rmean, rvar) against float64. mean and invstd: one f32 spacing of the
    float64 value (invstd: plus the cancellation allowance of E[y^2] - mean^2). The derived
    outputs are f32 expressions of stored f32 values -- scale = gamma * invstd is one f32 product,
    bit-equal; shift = beta - mean * scale and the running averages round up to three times, each
    by at most half a spacing of its own term, so: one spacing of the result plus half a spacing
    of each product term -- evaluated in float64 from the stored values they read."""
    bad = []
    r = fwd_finalize_ref(tot, count, eps)

    def chk(name, g_, ref, extra=0.0):
        ok, worst = within_ulp(g_, ref, F32, extra)
        if not bool(ok.all()):
            bad.append(f"{name}: {int((~ok).sum())} of {ok.numel()} outside the bound, worst x{worst:.3g}")

    chk("mean", got["mean"], r["mean"])
    chk("invstd", got["invstd"], r["invstd"], r["inv_extra"])
    ga, be = p["gamma"].float(), p["beta"].float()
    if not torch.equal(got["scale"], ga * got["invstd"]):
        bad.append("scale != gamma * invstd (one f32 product)")
    prod = got["mean"].to(F64) * got["scale"].to(F64)
    chk("shift", got["shift"], be.to(F64) - prod, 0.5 * ulp_out(prod, F32))
    m = f32c(momentum)
    om = float(np.float32(1.0) - np.float32(momentum))
    for name, old, new in (("rmean", p["rmean"], got["mean"].to(F64)),
                           ("rvar", p["rvar"], r["unb"].float().to(F64))):
        if update:
            t1, t2 = om * old, m * new
            extra = 0.5 * (ulp_out(t1, F32) + ulp_out(t2, F32))
            if name == "rvar":                       # (float)unb itself within a spacing
                extra = extra + m * ulp_out(r["unb"], F32)
            chk(name, got[name], t1 + t2, extra)
        elif not torch.equal(got[name], old.float()):
            bad.append(f"{name} changed without update")
    return bad


# the shapes the GPU file uses (tests/test_bn_refs_cpu.py proves every builder's premises on them)
APPLY_SHAPES = [(1, 8), (37, 8), (203, 64), (171, 24), (50, 192), (5, 2048)]
STREAM_SHAPES = [(203, 64), (61, 256)]
BIG_BLOCK, BIG_ROWS, BIG_C = 1021, 699051, 24      # n8 = 2097153 = 8192 * 256 + 1
REDUCE_C = [8, 24, 64, 192, 2048, 4096]
REDUCE_ROWS = [1, 37, 203]
STATS_T = [1, 5, 97, 700]
STATS_C = [4, 12, 64, 192, 1028]
FWD_C = [4, 12, 192, 1028]
FWD_CASES = [(5, 128, 5 * 128 - 37), (97, 64, 97 * 64 - 1), (1, 128, 1)]   # (T, bm, M)
SLAB_G = [1, 3, 4, 5, 193, 1000]
SLAB_QC = [8, 255, 257, 6168]


# streaming configurations (unroll, memory policy, grid cap, auto threshold MiB): those of
# test_bn_streaming_apply_configs (tests/test_kernels_gpu.py) plus grid caps 1, 2 and 3
ONE_CHUNK = (0, 0, 8192, 100)
STREAM_CFGS = [ONE_CHUNK, (1, 0, 8192, 100), (2, 0, 8192, 100), (4, 3, 8192, 100), (2, 3, 7, 100),
               (4, 1, 3, 100), (-1, 3, 16384, 0), (4, 5, 8192, 100), (-1, 5, 7, 0),
               (2, 0, 1, 100), (4, 3, 2, 100), (2, 2, 3, 100), (1, 3, 1, 100)]


def reduce_G(rows: int):
    return [1, 3, rows, rows + 2]


def stream_grid(cfg, n8: int, C: int) -> int:
    """csrc/bn.hip stream_grid: blocks of the U-chunk kernels for configuration ``cfg`` =
    (unroll, ntm, cap, min_mb); 0 = the one-chunk kernel."""
    unroll, _, cap, min_mb = cfg
    if unroll == 0 or (unroll < 0 and n8 * 16 < (min_mb << 20)):
        return 0
    per_thread = -(-n8 // stream_chunks(cfg))
    g = max(1, min(cap, -(-per_thread // 256)))
    return g if (g * 256) % (C // 8) == 0 else 0


def stream_chunks(cfg) -> int:
    u = cfg[0]
    return u if u > 0 else (4 if u == -1 else -u)


def stream_loops(cfg, n8: int, C: int):
    """(threads whose whole-batch loop iterates, chunks left to the remainder loop) of the U-chunk
    kernels, from their loop bounds: ``for (; i + (U-1)*stride < n8; i += U*stride)`` then
    ``for (; i < n8; i += stride)``."""
    g, u = stream_grid(cfg, n8, C), stream_chunks(cfg)
    stride = g * 256
    batch = rem = 0
    for i0 in range(min(stride, n8)):
        i = i0
        if i + (u - 1) * stride < n8:
            batch += 1
        while i + (u - 1) * stride < n8:
            i += u * stride
        rem += len(range(i, n8, stride))
    return batch, rem


def slab_ref(x, G: int, S: int):
    """pda_slab_reduce: [G][QC] -> [s][QC] with rows_per = ceil(G / S), s = ceil(G / rows_per)."""
    rows_per = -(-G // S)
    s = -(-G // rows_per)
    return torch.stack([x[i * rows_per:min(G, (i + 1) * rows_per)].sum(0) for i in range(s)]), s
