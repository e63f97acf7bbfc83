"""References for the loss / optimizer / cast / pooling kernel tests (tests/test_head_kernels_gpu.py).

Everything here runs on the CPU in float64 or exact integer logic and uses no kernel of this
project; tests/test_head_refs_cpu.py checks these functions against torch where torch's behaviour
is defined, so the references themselves are verified on a machine without a GPU.
"""
import functools
import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -23          # f32 spacing at 1 (the summation bounds below use it)

# explicit mantissa bits, exponent of the smallest normal, largest finite value
_FMT = {
    torch.bfloat16: (7, -126, float.fromhex("0x1.fep127")),
    torch.float16: (10, -14, 65504.0),
    torch.float32: (23, -126, float.fromhex("0x1.fffffep127")),
}


def ulp_out(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of ``dtype`` at |ref| (float64 in, float64 out); below the smallest normal the
    (constant) subnormal spacing."""
    p, emin, _ = _FMT[dtype]
    r = ref.to(F64).abs()
    _, e = torch.frexp(r)                       # r = m * 2^e, m in [0.5, 1)
    e = torch.where(r == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(r), e - p)


def within_ulp(got: torch.Tensor, ref: torch.Tensor, dtype: torch.dtype, extra=0.0):
    """(ok mask, worst ratio err / bound) for |got - ref| <= ulp_out(ref) + extra, per element.
    Where ref lies beyond the dtype's overflow threshold (largest finite + half a spacing) the
    correctly rounded result is an infinity of ref's sign; within 1e-6 relative of that threshold
    either is accepted."""
    p, _, fmax = _FMT[dtype]
    g, r = got.to(F64), ref.to(F64)
    thr = fmax * (1 + 2.0 ** -(p + 2))          # fmax + half a spacing
    over = r.abs() > thr * (1 + 1e-6)
    near = (r.abs() > thr * (1 - 1e-6)) & ~over
    bound = ulp_out(r, dtype) + extra
    err = (g - r).abs()
    ok_fin = err <= bound                       # NaN in got compares False
    ok_over = torch.isinf(g) & (torch.sign(g) == torch.sign(r))
    ok = torch.where(over, ok_over, torch.where(near, ok_fin | ok_over, ok_fin))
    ratio = torch.where(over | near, torch.zeros_like(err), err / bound)
    return ok, float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0


def to_dtype(x64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Round float64 values that are exact in float32 to ``dtype`` (one rounding, nearest-even)."""
    x32 = x64.to(torch.float32)
    assert torch.equal(x32.to(F64), x64), "to_dtype: value not exact in float32"
    return x32.to(dtype)


def bits16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality of two tensors of one dtype (-0 != +0; NaN payloads compare)."""
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {2: torch.int16, 4: torch.int32, 1: torch.uint8, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def quantised(shape, step: float, lim: float, g: torch.Generator) -> torch.Tensor:
    """float64 multiples of ``step`` drawn uniformly from [-lim, lim]."""
    k = int(round(lim / step))
    return torch.randint(-k, k + 1, shape, generator=g).to(F64) * step


# ------------------------------------------------------------------ stem pool / max-pool backward
def pool_dims(H: int, W: int):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def pool_ref(y, sc, sh, dtype=F64):
    """r = max(y*sc+sh, 0), then 3x3 / stride 2 / pad 1 max-pool over NHWC. Returns (out, arg):
    arg (uint8) = dy*3+dx of the FIRST maximum in (dy, dx) scan order among the in-bounds taps.
    ``dtype``: the arithmetic's precision (the exact-input checks evaluate it in f32 and f64)."""
    N, H, W, C = y.shape
    Ho, Wo = pool_dims(H, W)
    r = (y.to(dtype) * sc.to(dtype) + sh.to(dtype)).clamp_min(0)
    pad = torch.full((N, H + 2, W + 2, C), float("-inf"), dtype=dtype)
    pad[:, 1:H + 1, 1:W + 1] = r
    best = torch.full((N, Ho, Wo, C), float("-inf"), dtype=dtype)
    arg = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8)
    for dy in range(3):
        for dx in range(3):
            cand = pad[:, dy:dy + 2 * Ho - 1:2, dx:dx + 2 * Wo - 1:2]
            upd = cand > best                   # strict: an equal later tap never replaces
            best = torch.where(upd, cand, best)
            arg = torch.where(upd, torch.full_like(arg, dy * 3 + dx), arg)
    return best, arg


def pool_scatter(dout, arg, H: int, W: int, dtype=F64):
    """din[n, 2*yo-1+a//3, 2*xo-1+a%3, c] += dout[n, yo, xo, c]: an explicit scatter, accumulated
    in ``dtype`` (float64; float32 for the exact-input checks)."""
    N, Ho, Wo, C = dout.shape
    n, yo, xo, c = torch.meshgrid(torch.arange(N), torch.arange(Ho), torch.arange(Wo),
                                  torch.arange(C), indexing="ij")
    a = arg.long()
    yy, xx = 2 * yo - 1 + a // 3, 2 * xo - 1 + a % 3
    assert int(a.max()) <= 8 and int(yy.min()) >= 0 and int(yy.max()) < H
    assert int(xx.min()) >= 0 and int(xx.max()) < W
    din = torch.zeros(N, H, W, C, dtype=dtype)
    din.index_put_((n.reshape(-1), yy.reshape(-1), xx.reshape(-1), c.reshape(-1)),
                   dout.to(dtype).reshape(-1), accumulate=True)
    return din


def random_valid_arg(N, H, W, C, g: torch.Generator) -> torch.Tensor:
    """Arbitrary in-bounds window taps (uint8 dy*3+dx): valid argmax bytes that are no argmax."""
    Ho, Wo = pool_dims(H, W)

    def taps(n_out, size):
        o = torch.arange(n_out)
        lo = (o == 0).long()                              # tap 0 of window 0 is the padding
        hi = torch.clamp(size - 1 - (2 * o - 1), max=2)   # last in-bounds tap
        return lo, hi
    ylo, yhi = taps(Ho, H)
    xlo, xhi = taps(Wo, W)
    ry = torch.randint(0, 6, (N, Ho, Wo, C), generator=g)
    rx = torch.randint(0, 6, (N, Ho, Wo, C), generator=g)
    dy = ylo[None, :, None, None] + ry % (yhi - ylo + 1)[None, :, None, None]
    dx = xlo[None, None, :, None] + rx % (xhi - xlo + 1)[None, None, :, None]
    return (dy * 3 + dx).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def pool_case(N: int, H: int, W: int, C: int) -> dict:
    """Exact-arithmetic inputs of section 1 and every reference derived from them (shared by the
    dtype cases: all values are representable in bf16, fp16 and fp32). Treat as read-only."""
    g = _gen(1000 * N + 100 * H + 10 * W + C)
    Ho, Wo = pool_dims(H, W)
    y = quantised((N, H, W, C), 0.25, 4.0, g)
    sc = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (C,), generator=g)]
    sh = quantised((C,), 0.125, 1.0, g)
    dout = quantised((N, Ho, Wo, C), 1.0 / 64, 4.0, g)
    dout2 = quantised((N, Ho, Wo, C), 1.0 / 64, 4.0, g)
    out, arg = pool_ref(y, sc, sh)
    # the inputs make the f32 arithmetic exact: the same reference in f32 is bit-identical
    out32, arg32 = pool_ref(y, sc, sh, torch.float32)
    assert torch.equal(out32.to(F64), out) and torch.equal(arg32, arg)
    fake = random_valid_arg(N, H, W, C, g)
    assert not torch.equal(fake, arg)
    mask = (sc * y + sh > 0).to(F64)
    assert torch.equal((sc.float() * y.float() + sh.float() > 0), mask.bool())
    case = dict(y=y, sc=sc, sh=sh, dout=dout, dout2=dout2, out=out, arg=arg, fake=fake, mask=mask)
    for an, a in (("arg", arg), ("fake", fake)):
        for two in (False, True):
            d = dout + dout2 if two else dout
            s = pool_scatter(d, a, H, W)
            s32 = pool_scatter(d, a, H, W, torch.float32)
            assert torch.equal(s32.to(F64), s)
            case[("scatter", an, two)] = s
    return case


# ------------------------------------------------------------------ tail pool
@functools.lru_cache(maxsize=None)
def tail_case(N: int, H: int, W: int, C: int) -> dict:
    """Inputs for which every term relu(y*sc+sh+s) is exact in f32 (y, res, y2: multiples of 1/4
    in [-4, 4]; sc, sc2 in {1/2, 1, 2}; sh, sh2 multiples of 1/64 in [-1, 1] -- terms need up to 11
    significant bits, more than bf16 holds), so only the summation and the output rounding remain."""
    g = _gen(7 * N + 13 * H + 17 * W + C)
    pick = torch.tensor([0.5, 1.0, 2.0], dtype=F64)
    d = dict(y=quantised((N, H, W, C), 0.25, 4.0, g), res=quantised((N, H, W, C), 0.25, 4.0, g),
             sc=pick[torch.randint(0, 3, (C,), generator=g)], sh=quantised((C,), 1.0 / 64, 1.0, g),
             sc2=pick[torch.randint(0, 3, (C,), generator=g)], sh2=quantised((C,), 1.0 / 64, 1.0, g))
    for mode in (1, 2):
        t = tail_terms(d, mode)
        t32 = tail_terms({k: v.float() for k, v in d.items()}, mode)
        assert t32.dtype == torch.float32 and torch.equal(t32.to(F64), t)
        d[("ref", mode)] = t.mean((1, 2))
        # summation bound with n = HW over the terms t/HW (all >= 0): n * 2^-23 * sum|t/HW|
        d[("sumbound", mode)] = H * W * EPS32 * t.mean((1, 2))
    return d


def tail_terms(d: dict, mode: int) -> torch.Tensor:
    s = d["res"] if mode == 1 else d["res"] * d["sc2"] + d["sh2"]
    return (d["y"] * d["sc"] + d["sh"] + s).clamp_min(0)


# ------------------------------------------------------------------ cross-entropy / top-k
def xent_ref(logits64: torch.Tensor, labels: torch.Tensor):
    """(loss_rows, dloss_rows/dlogits) in float64: lse(x) - x[label], softmax(x) - onehot."""
    x = logits64.to(F64)
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    rows = (m + torch.log(s)).squeeze(1) - x.gather(1, labels[:, None]).squeeze(1)
    grad = e / s
    grad[torch.arange(x.shape[0]), labels] -= 1.0
    return rows, grad


def topk_ref(logits: torch.Tensor, labels: torch.Tensor):
    """(top-1 hits, top-5 hits) by exact integer logic: a row's label ranks behind every strictly
    larger logit and every equal logit of lower index."""
    v = logits.gather(1, labels[:, None])
    k = torch.arange(logits.shape[1])[None, :]
    better = ((logits > v) | ((logits == v) & (k < labels[:, None]))).sum(1)
    return int((better < 1).sum()), int((better < 5).sum())


# ------------------------------------------------------------------ SGD / casts
def sgd_ref(p, g, steps: int, lr, momentum, wd, inv_scale=1.0):
    """float64 torch-SGD emulation (weight decay added to the gradient, first step buf = d_p, no
    dampening, no Nesterov). Returns [(p, buf) after each step]."""
    p, g = p.to(F64).clone(), g.to(F64)
    buf, out = None, []
    for _ in range(steps):
        d = g * inv_scale + wd * p
        buf = d.clone() if buf is None else momentum * buf + d
        p = p - lr * buf
        out.append((p.clone(), buf.clone()))
    return out


def _f32(bits) -> torch.Tensor:
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def cast_edge_values() -> torch.Tensor:
    """f32 edge cases of the 16-bit casts (no f32 subnormals): rounding ties of both parities in
    bf16 and fp16, signed zeros, the fp16 and bf16 overflow thresholds, infinities, NaN, and f32
    normals inside fp16's subnormal range with their ties."""
    bits = []
    for sign in (0, 0x80000000):
        # bf16 ties: low 16 bits = 0x8000 over an even / odd kept mantissa (1.0, 1.0078125, ...)
        bits += [sign | 0x3F808000, sign | 0x3F818000, sign | 0x40FE8000, sign | 0x40FF8000]
        # just beside the ties
        bits += [sign | 0x3F807FFF, sign | 0x3F808001, sign | 0x3F817FFF, sign | 0x3F818001]
        # fp16 ties: low 13 bits = 0x1000 over an even / odd kept mantissa
        bits += [sign | 0x3F801000, sign | 0x3F803000, sign | 0x477FD000, sign | 0x3F800FFF,
                 sign | 0x3F801001, sign | 0x3F802FFF, sign | 0x3F803001]
        bits += [sign]                                   # +-0
        bits += [sign | 0x7F800000]                      # +-inf
        # bf16 overflow: largest bf16, just below / at / above the tie to infinity, f32 max
        bits += [sign | 0x7F7F0000, sign | 0x7F7F7FFF, sign | 0x7F7F8000, sign | 0x7F7F8001,
                 sign | 0x7F7FFFFF]
    v = [_f32(bits)]
    def nxt(x, toward):                                  # neighbour in float32
        return float(np.nextafter(np.float32(x), np.float32(toward)))
    f = [65504.0, nxt(65520.0, 0.0), 65520.0, nxt(65520.0, 1e9), 65536.0, 1e5,
         65488.0, nxt(65488.0, 0.0), nxt(65488.0, 1e9)]  # 65488: tie between 65472 and 65504
    # fp16 subnormal range: spacing 2^-24. Exact subnormals, ties over even / odd, neighbours,
    # the tie between 0 and the smallest subnormal, the boundary to the normals
    u = 2.0 ** -24
    for k in (1, 2, 3, 5, 512, 1022, 1023):
        f += [k * u, (k + 0.5) * u, nxt((k + 0.5) * u, 0.0), nxt((k + 0.5) * u, 1.0)]
    f += [0.5 * u, nxt(0.5 * u, 1.0), nxt(0.5 * u, 0.0), 0.25 * u, 2.0 ** -14,
          nxt(2.0 ** -14, 0.0), 2.0 ** -14 - 0.5 * u]
    f = f + [-x for x in f]
    v.append(torch.tensor(f, dtype=F64).to(torch.float32))
    v.append(torch.tensor([float("nan")], dtype=torch.float32))
    out = torch.cat(v)
    tiny = torch.finfo(torch.float32).tiny
    assert bool(((out == 0) | (out.abs() >= tiny) | out.isnan()).all()), "f32 subnormal in edges"
    return out


def cast_input(n: int, seed: int = 5) -> torch.Tensor:
    """The edge values followed by random data of mixed magnitude (1e-7 .. 1e5), n elements."""
    e = cast_edge_values()
    g = _gen(seed)
    m = max(n - e.numel(), 0)
    r = torch.randn(m, generator=g) * torch.pow(10.0, torch.randint(-7, 6, (m,), generator=g).float())
    r = torch.where(r.abs() < torch.finfo(torch.float32).tiny, torch.ones_like(r), r)
    return torch.cat([e, r])[:n].contiguous()


def cast_matches(got16: torch.Tensor, src32: torch.Tensor) -> torch.Tensor:
    """Per-element: got16 == torch's CPU cast of src32, bit for bit; NaN compared as 'is NaN'."""
    want = src32.cpu().to(got16.dtype)
    got = got16.cpu()
    nan = want.isnan()
    return torch.where(nan, got.isnan(), bits16(got) == bits16(want))


# ------------------------------------------------------------------ BatchNorm eval coefficients
def bn_eval_ref(gamma, beta, mean, var, eps: float):
    sc = gamma.to(F64) / torch.sqrt(var.to(F64) + eps)
    return sc, beta.to(F64) - mean.to(F64) * sc


def rsqrt_yardstick(var32: torch.Tensor, eps: float) -> float:
    """Worst relative error of torch's float32 rsqrt(var + eps) (f32 add included) against
    float64, over the given inputs."""
    got = torch.rsqrt(var32.float() + torch.tensor(eps, dtype=torch.float32)).to(F64)
    ref = 1.0 / torch.sqrt(var32.to(F64) + eps)
    return float(((got - ref).abs() / ref).max())
