"""Exact-integer references for the convolution kernel tests (tests/test_conv_exact_gpu.py).

Everything here runs on the CPU in float64 and uses no kernel of this project;
tests/test_conv_refs_cpu.py checks these functions against naive loops and plain torch ops, and
runs :func:`assert_exact_conditions` on every case the GPU file parametrises.

The exactness argument: operands are small integers, so every product and every partial sum of an
MFMA accumulation is an integer below 2^24 and the f32 accumulator is exact whatever the summation
order, tile, split-K depth or pipeline. The stored result must therefore equal the integer
reference rounded once (nearest-even) to the storage dtype, bit for bit, at every element.

Roundings the kernels perform that the models below follow (all of them the identity on the
integer data of the cases, which :func:`assert_exact_conditions` proves per case):

* the operand prologue rounds relu(x*sc+sh) to the 16-bit dtype before the MFMA
  (csrc/conv_gemm.hip ``pro_apply``: ``pack2<DT>(fma2(u, psc[k], psh[k]))``);
* the fused dgrad epilogue reads the data gradient back from the 16-bit C tile
  (``pk.x = pack2<DT>(f32x2{v[0], v[1]})`` in the staging loop), i.e. dA is rounded to 16 bits
  BEFORE ``g2`` is added and the mask applied (:func:`dgrad_epi_ref` rounds it there too);
* WGRAD_BNA rounds dY = fma(k1, dz, fma(k2, y, k3)) to 16 bits while staging
  (``pack2<DT>(bnb_affine2(...))``).
"""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

F64 = torch.float64
LIM16 = 256.0            # |integer| <= 256 is exact in bf16 (8 significant bits) and f16
LIM_ACC = float(2 ** 24)  # integers below 2^24 are exact in an f32 accumulator


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """One geometry of the GPU file. ``Cout`` is the forward's channel count; ``cout_pad`` (the fc
    head) the padded row count its weights, data gradient and weight gradient use. ``passes`` lists
    the passes the kernels serve for it (the stems have no data gradient: their input is the
    image, and a 7x7 stride-2 class has more than the 9 taps the class tables hold)."""
    id: str
    Nb: int
    H: int
    W: int
    Cin: int
    Cout: int
    R: int
    S: int
    stride: int
    pad: int
    ho: Optional[int] = None
    wo: Optional[int] = None
    cin_real: Optional[int] = None
    kpad: Optional[int] = None         # forward weight row pitch (None: R*S*Cin)
    cout_pad: Optional[int] = None
    passes: Tuple[str, ...] = ("fwd", "dgrad", "wgrad")
    f32: bool = False                  # also runs the two f32 kernels

    @property
    def Ho(self):
        return self.ho if self.ho is not None else (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def Wo(self):
        return self.wo if self.wo is not None else (self.W + 2 * self.pad - self.S) // self.stride + 1

    @property
    def K(self):
        return self.R * self.S * self.Cin

    @property
    def M(self):
        return self.Nb * self.Ho * self.Wo

    @property
    def rows(self):          # weight rows / gradient channels (fc: padded)
        return self.cout_pad or self.Cout


CASES = {c.id: c for c in [
    Case("A", 3, 9, 7, 64, 192, 3, 3, 1, 1, f32=True),
    Case("B", 4, 11, 13, 64, 128, 3, 3, 1, 1),
    Case("C", 2, 8, 12, 128, 64, 3, 3, 2, 1, f32=True),
    Case("D", 2, 10, 6, 256, 128, 1, 1, 2, 0, f32=True),
    Case("E", 1, 7, 5, 512, 256, 3, 3, 1, 1),
    Case("F", 5, 6, 10, 64, 64, 1, 1, 1, 0, f32=True),
    Case("F2", 5, 6, 10, 64, 128, 1, 1, 1, 0, passes=("fwd",)),   # FWD_TAIL's 128-column tile
    Case("G", 5, 1, 1, 256, 100, 1, 1, 1, 0, cout_pad=128),
    Case("H1", 2, 8, 16, 16, 64, 4, 4, 1, 2, ho=8, wo=16, passes=("fwd", "wgrad")),
    Case("H2", 2, 12, 48, 16, 64, 4, 4, 1, 2, ho=12, wo=48, passes=("fwd", "wgrad")),
    Case("I", 2, 10, 14, 8, 64, 7, 7, 2, 3, cin_real=3, kpad=448, passes=("fwd", "wgrad")),
]}
DTYPES16 = {"bf16": torch.bfloat16, "f16": torch.float16}

# tile codes (pytorch_distributed_amd.ops.native_ops.tile_rows): bm < 0 single-stage register
# tile, bm > 1000 LDS-DMA, bm > 2000 tap reuse (HALO). The same lists as tests/test_conv_shapes_gpu.py
TILES = [(128, 128), (128, 64), (64, 128), (64, 64), (-128, 128), (-128, 64), (-64, 128)]
DMA_TILES = [(1256, 128), (1128, 256), (1128, 128)]
HALO_TILES = [(2256, 128), (2256, 64)]
WGRAD_ONLY_TILES = [(-256, 128), (1256, 256)]
FWD_ONLY_TILES = [(-256, 64)]
BNA_TILES = [(-64, 128), (64, 128), (-64, 256), (-128, 128), (128, 128), (-128, 64)]
PASS_TILES = {
    "fwd": TILES + DMA_TILES + HALO_TILES + FWD_ONLY_TILES,
    "dgrad": TILES + DMA_TILES + HALO_TILES,
    "wgrad": TILES + DMA_TILES + WGRAD_ONLY_TILES,
}


def tile_rows(bm: int) -> int:
    return bm - 2000 if bm > 2000 else bm - 1000 if bm > 1000 else abs(bm)


def _pow2(v: int) -> bool:
    return v > 0 and (v & (v - 1)) == 0


def accepts(pas: str, tile, c: Case) -> bool:
    """Whether the 16-bit dispatch takes (pass, tile) for this geometry -- the host-side rules of
    csrc/conv_gemm.hip (``dispatch``, ``halo_ok``, ``pda_conv_fwd``, ``dgrad_params``). The GPU
    tests launch exactly the accepted combinations; a launch this predicate accepts and the
    library rejects is a failure there."""
    bm, bn = tile
    if pas not in c.passes or tile not in PASS_TILES[pas]:
        return False
    if pas == "dgrad" and (c.stride not in (1, 2) or c.H % c.stride or c.W % c.stride or c.rows % 64):
        return False
    if bm > 2000:
        csz = c.Cin if pas == "fwd" else c.rows
        if not (c.R == 3 and c.S == 3 and c.stride == 1 and c.pad == 1 and c.W <= 63
                and csz % 64 == 0 and c.Ho == c.H and c.Wo == c.W):
            return False
    if bm > 1000 and pas == "fwd" and (c.Cin < 64 or not _pow2(c.Cin)):
        return False
    return True


def tail_ok(c: Case) -> bool:
    """Geometries the FWD_TAIL tests run: 1x1 stride-1 convs with a 16-bit output."""
    return (c.R == 1 and c.S == 1 and c.stride == 1 and c.pad == 0 and c.Cin % 64 == 0
            and c.Cout % 8 == 0 and c.H * c.W > 1)


def accepts_bna(tile, c: Case) -> bool:
    return "wgrad" in c.passes and tile in BNA_TILES and c.rows % 8 == 0


# ------------------------------------------------------------------ data
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def ints(shape, lim: int, seed: int) -> torch.Tensor:
    """float64 integers drawn uniformly from {-lim..lim}."""
    return torch.randint(-lim, lim + 1, tuple(shape), generator=_gen(seed)).to(F64)


def act_lim(c: Case) -> int:
    """Activations and gradients in {-2..2}; {-1, 0, 1} for K = R*S*Cin above 1200 (with {-2..2}
    at K = 4608 max|y| reaches ~313 > 256)."""
    return 1 if c.K > 1200 else 2


@functools.lru_cache(maxsize=None)
def case_data(cid: str):
    """(x [Nb,H,W,Cin], w [rows,R,S,Cin] OHWI, dy [Nb,Ho,Wo,rows]) float64 integers; channels past
    ``cin_real`` of x and w, and rows / channels past ``Cout`` of w and dy (the fc head's padding),
    are zero. Cached: do not modify."""
    c = CASES[cid]
    seed = 1000 + 17 * sorted(CASES).index(cid)
    x = ints((c.Nb, c.H, c.W, c.Cin), act_lim(c), seed)
    w = ints((c.rows, c.R, c.S, c.Cin), 1, seed + 1)
    dy = ints((c.Nb, c.Ho, c.Wo, c.rows), act_lim(c), seed + 2)
    if c.cin_real is not None:
        x[..., c.cin_real:] = 0
        w[..., c.cin_real:] = 0
    w[c.Cout:] = 0
    dy[..., c.Cout:] = 0
    return x, w, dy


def coeffs(n: int, seed: int, scales=(1.0, 2.0, -1.0, -2.0), shift_lim: int = 1):
    """Per-channel (scale, shift): scales powers of two (both signs), shifts small integers."""
    g = _gen(seed)
    sc = torch.tensor(scales, dtype=F64)[torch.randint(0, len(scales), (n,), generator=g)]
    sh = torch.randint(-shift_lim, shift_lim + 1, (n,), generator=g).to(F64)
    return sc, sh


# ------------------------------------------------------------------ float64 references
def _pads(c: Case):
    """(left, right, top, bottom) zero padding that gives exactly Ho x Wo outputs (the stem's
    explicit ho = H, wo = W: 2 top / left, 1 bottom / right)."""
    bottom = (c.Ho - 1) * c.stride + c.R - c.H - c.pad
    right = (c.Wo - 1) * c.stride + c.S - c.W - c.pad
    return (c.pad, right, c.pad, bottom)


def _conv_nchw(x_nchw, w_oihw, c: Case):
    return F.conv2d(F.pad(x_nchw, _pads(c)), w_oihw, stride=c.stride)


def conv_fwd_ref(x, w, c: Case) -> torch.Tensor:
    """y [Nb,Ho,Wo,rows] float64 = conv(x NHWC, w OHWI)."""
    y = _conv_nchw(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), c)
    assert y.shape[2:] == (c.Ho, c.Wo), (y.shape, c)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_bwd_ref(x, w, dy, c: Case):
    """(dx [Nb,H,W,Cin], dw [rows,R,S,Cin]) float64 by autograd of the same padded conv."""
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    _conv_nchw(xr, wr, c).backward(dy.permute(0, 3, 1, 2))
    return xr.grad.permute(0, 2, 3, 1).contiguous(), wr.grad.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def case_refs(cid: str):
    """(y, dx, dw) of :func:`case_data`, computed once per case. Cached: do not modify."""
    c = CASES[cid]
    x, w, dy = case_data(cid)
    dx, dw = conv_bwd_ref(x, w, dy, c)
    return conv_fwd_ref(x, w, c), dx, dw


def pack_stem_rows(w, kpad: int) -> torch.Tensor:
    """[rows, R, S, Cin] -> [rows, kpad]: taps x padded channels, zero behind (the packed stem
    image conv_fwd takes with ``Kpad`` = 448)."""
    out = torch.zeros(w.shape[0], kpad, dtype=w.dtype)
    out[:, :w[0].numel()] = w.reshape(w.shape[0], -1)
    return out


# ------------------------------------------------------------------ rounding
def round_to(v64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """float64 values that are exact in float32, rounded ONCE (nearest-even) to ``dtype``."""
    v32 = v64.to(torch.float32)
    assert torch.equal(v32.to(F64), v64), "round_to: value not exact in float32"
    return v32.to(dtype)


def r64(v64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return round_to(v64, dtype).to(F64)


# ------------------------------------------------------------------ models of the fused pieces
def pro_ref(x, sc, sh, dtype) -> torch.Tensor:
    """Operand prologue: relu(x*sc+sh) rounded once to the operand dtype (conv_fwd / conv_wgrad
    ``pro``; padding taps stay 0 because the conv pads the result, not x)."""
    return r64(torch.relu(x * sc + sh), dtype)


def stats_ref(y_stored: torch.Tensor) -> torch.Tensor:
    """[2][C] float64: per column sum y and sum y^2 of the STORED output (conv_fwd ``stats``)."""
    yb = y_stored.to(F64).reshape(-1, y_stored.shape[-1])
    return torch.stack([yb.sum(0), (yb * yb).sum(0)])


def mask_bytes(a: torch.Tensor) -> torch.Tensor:
    """ReLU bitmask of ``a`` (numel / 8 bytes): bit e of byte i is element 8i+e > 0 (bn_apply)."""
    b = (a.reshape(-1, 8) > 0).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


def tail_ref(y3, sc, sh, res, dtype, sc2=None, sh2=None):
    """FWD_TAIL: a = relu(y3*sc+sh + res) (mode 1) or relu(y3*sc+sh + res*sc2+sh2) (mode 2),
    rounded once; returns (a float64, its ReLU bitmask)."""
    r = res if sc2 is None else res * sc2 + sh2
    a = r64(torch.relu(y3 * sc + sh + r), dtype)
    return a, mask_bytes(a)


def dgrad_epi_ref(dA, mode, y, sc, sh, dtype, y2=None, sc2=None, sh2=None, g2=None, mask=None):
    """Fused BatchNorm-backward epilogue of conv_dgrad. dA is the transposed conv result; the
    kernel rounds it to the C tile's dtype, adds ``g2``, masks with the forward's ReLU
    (mode 0: bn(y) > 0; 1: bn(y) + y2 > 0; 2: bn(y) + bn2(y2) > 0; 3: the bit of ``mask``) and
    stores dz rounded. Returns (dz float64 as stored, totals [nq][C] float64): sum dz, sum dz*y
    and, mode 2, sum dz*y2 -- of the rounded dz when ``g2`` is given, else of the unrounded one
    (csrc/conv_gemm.hip rows(): ``if constexpr (G2) dz = unpack2<DT>(o)``)."""
    g = r64(dA, dtype)
    if g2 is not None:
        g = g + g2
    if mode == 3:
        bits = (mask.reshape(-1, 1).to(torch.int32) >> torch.arange(8, dtype=torch.int32)) & 1
        keep = bits.reshape(y.shape) > 0
    else:
        pre = y * sc + sh
        if mode == 1:
            pre = pre + y2
        elif mode == 2:
            pre = pre + (y2 * sc2 + sh2)
        keep = pre > 0
    dz = torch.where(keep, g, torch.zeros_like(g))
    stored = r64(dz, dtype)
    s = stored if g2 is not None else dz
    C = y.shape[-1]
    q = [s.reshape(-1, C).sum(0), (s * y).reshape(-1, C).sum(0)]
    if mode == 2:
        q.append((s * y2).reshape(-1, C).sum(0))
    return stored, torch.stack(q)


def bna_ref(dz, y, k1, k2, k3, dtype) -> torch.Tensor:
    """WGRAD_BNA operand dY = fma(k1, dz, fma(k2, y, k3)), rounded to the operand dtype."""
    return r64(k1 * dz + (k2 * y + k3), dtype)


# ------------------------------------------------------------------ exactness conditions
def abs_acc(x, w, dy, c: Case):
    """Sum of |terms| of every accumulation: (per y element, per dx element, per dw element)."""
    ya = conv_fwd_ref(x.abs(), w.abs(), c)
    dxa, dwa = conv_bwd_ref(x.abs(), w.abs(), dy.abs(), c)
    return ya, dxa, dwa


def stats_abs(y_stored: torch.Tensor, rows: int):
    """Per statistics tile (``rows`` consecutive rows of M) and column, upper bounds of
    sum |y - s| and sum (y - s)^2 for the worst shift s = ANY row of the tile: with
    m = max |y| of the tile and column, |y - s| <= |y| + m."""
    yb = y_stored.to(F64).reshape(-1, y_stored.shape[-1]).abs()
    out1, out2 = [], []
    for r0 in range(0, yb.shape[0], rows):
        t = yb[r0:r0 + rows]
        d = t + t.max(0, keepdim=True).values
        out1.append(d.sum(0))
        out2.append((d * d).sum(0))
    return torch.stack(out1), torch.stack(out2)


def assert_exact_conditions(name: str, stored16=(), acc_abs=(), stats_of=(), stat_rows=(64, 128, 256)):
    """The exactness argument's premises, checked on the reference alone. ``stored16``: tensors
    of values that pass through a 16-bit format (integers, |v| <= 256: exact in bf16 and f16);
    ``acc_abs``: tensors of sum |terms| of f32 accumulations (each < 2^24); ``stats_of``: stored
    outputs whose shifted statistics partials must stay below 2^24 for every tile height in
    ``stat_rows``. These are conditions on the inputs: a violation is a bug of the case, and it
    raises."""
    for i, t in enumerate(stored16):
        t = t.to(F64)
        assert torch.equal(t, t.round()), f"{name}: stored16[{i}] holds non-integers"
        assert float(t.abs().max()) <= LIM16, f"{name}: stored16[{i}] max |v| {float(t.abs().max())} > 256"
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(torch.float32).to(dt).to(F64), t), f"{name}: stored16[{i}] inexact in {dt}"
    for i, t in enumerate(acc_abs):
        assert float(t.max()) < LIM_ACC, f"{name}: acc_abs[{i}] sum |terms| {float(t.max())} >= 2^24"
    for i, t in enumerate(stats_of):
        for rows in stat_rows:
            s1, s2 = stats_abs(t, rows)
            assert float(s1.max()) < LIM_ACC and float(s2.max()) < LIM_ACC, \
                f"{name}: stats_of[{i}] at {rows} rows: {float(s1.max())}, {float(s2.max())} >= 2^24"


# ------------------------------------------------------------------ variants of a case (shared by the CPU and GPU files)
def fwd_variants(cid: str, dtype):
    """name -> dict(x=, y= the stored reference float64, plus the variant's operands) for the
    forward variants of a case; the references are float64, rounded where the kernel rounds."""
    c = CASES[cid]
    x, w, _ = case_data(cid)
    y = case_refs(cid)[0]
    out = {"plain": dict(x=x, y=r64(y, dtype)), "relu": dict(x=x, y=r64(torch.relu(y), dtype))}
    sc, sh = coeffs(c.Cin, 7 + c.K, scales=(1.0, -1.0) if c.K > 600 else (1.0, 2.0, -1.0, -2.0))
    a = pro_ref(x, sc, sh, dtype)
    if c.cin_real is None:      # (the padded stem image has no prologue: its padding would become relu(sh))
        out["pro"] = dict(x=x, sc=sc, sh=sh, a=a, y=r64(conv_fwd_ref(a, w, c), dtype))
    return out


def tail_variants(cid: str, dtype):
    """FWD_TAIL modes 1 and 2 on a 1x1 stride-1 case: y3 = the case's x."""
    c = CASES[cid]
    x, w, _ = case_data(cid)
    res = ints(x.shape, 2, 77)
    sc, sh = coeffs(c.Cin, 78)
    sc2, sh2 = coeffs(c.Cin, 79, scales=(1.0, -1.0))
    out = {}
    for mode in (1, 2):
        a, m = tail_ref(x, sc, sh, res, dtype, *((sc2, sh2) if mode == 2 else ()))
        out[mode] = dict(y3=x, res=res, sc=sc, sh=sh, sc2=sc2 if mode == 2 else None,
                         sh2=sh2 if mode == 2 else None, a=a, mask=m,
                         y=r64(conv_fwd_ref(a, w, c), dtype))
    return out


EPI_VARIANTS = [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]


@functools.lru_cache(maxsize=None)
def epi_operands(cid: str):
    c = CASES[cid]
    shp = (c.Nb, c.H, c.W, c.Cin)
    sc, sh = coeffs(c.Cin, 31)
    sc2, sh2 = coeffs(c.Cin, 32)
    return dict(y=ints(shp, 2, 33), y2=ints(shp, 2, 34), g2=ints(shp, 2, 35), sc=sc, sh=sh, sc2=sc2, sh2=sh2)


def dgrad_variants(cid: str, dtype):
    """(mode, with_g2) -> dict(dz=, tot=, mask=) for the fused dgrad epilogue; the mode-3 mask is
    the bitmask of a = relu(y*sc+sh + y2) built here on the CPU."""
    dA = case_refs(cid)[1]
    o = epi_operands(cid)
    a1, m1 = tail_ref(o["y"], o["sc"], o["sh"], o["y2"], dtype)
    out = {}
    for mode, wg in EPI_VARIANTS:
        dz, tot = dgrad_epi_ref(dA, mode, o["y"], o["sc"], o["sh"], dtype,
                                y2=o["y2"] if mode in (1, 2) else None,
                                sc2=o["sc2"] if mode == 2 else None, sh2=o["sh2"] if mode == 2 else None,
                                g2=o["g2"] if wg else None, mask=m1 if mode == 3 else None)
        out[(mode, wg)] = dict(dz=dz, tot=tot, mask=m1 if mode == 3 else None)
    return out


@functools.lru_cache(maxsize=None)
def bna_operands(cid: str):
    c = CASES[cid]
    g = _gen(91)
    k1 = torch.tensor([1.0, 2.0, -1.0], dtype=F64)[torch.randint(0, 3, (c.rows,), generator=g)]
    k2 = torch.tensor([1.0, -1.0, 0.5], dtype=F64)[torch.randint(0, 3, (c.rows,), generator=g)]
    k3 = torch.randint(-1, 2, (c.rows,), generator=g).to(F64)
    y = ints((c.Nb, c.Ho, c.Wo, c.rows), 1, 92) * 2     # even, so that k2 = 0.5 keeps integers
    return dict(y=y, k1=k1, k2=k2, k3=k3)


def wgrad_variants(cid: str, dtype):
    """name -> dict(dw=) float64 [rows,R,S,Cin]: plain, with the operand prologue, with the
    BN-backward operand (dy is dz there)."""
    c = CASES[cid]
    x, w, dy = case_data(cid)
    out = {"plain": dict(dw=case_refs(cid)[2])}
    if c.cin_real is None:
        sc, sh = coeffs(c.Cin, 51)
        a = pro_ref(x, sc, sh, dtype)
        out["pro"] = dict(sc=sc, sh=sh, a=a, dw=conv_bwd_ref(a, w, dy, c)[1])
    b = bna_operands(cid)
    dY = bna_ref(dy, b["y"], b["k1"], b["k2"], b["k3"], dtype)
    out["bna"] = dict(dY=dY, dw=conv_bwd_ref(x, w, dY, c)[1], **b)
    return out


def check_case_conditions(cid: str, dtype) -> None:
    """:func:`assert_exact_conditions` for every variant the GPU file runs on this case."""
    c = CASES[cid]
    x, w, dy = case_data(cid)
    y, dx, dw = case_refs(cid)
    ya, dxa, dwa = abs_acc(x, w, dy, c)
    rows = (64, 128, 256) + ((c.Wo,) if c.ho is not None else ())
    assert_exact_conditions(f"{cid}/plain", stored16=(x, w, dy, y, dx), acc_abs=(ya, dxa, dwa, 1024 + dwa),
                            stats_of=(y, torch.relu(y)), stat_rows=rows)
    for name, v in fwd_variants(cid, dtype).items():
        if name == "pro":
            assert_exact_conditions(f"{cid}/fwd/pro", stored16=(v["a"], v["y"]),
                                    acc_abs=(conv_fwd_ref(v["a"].abs(), w.abs(), c),), stats_of=(v["y"],))
    if tail_ok(c):
        for mode, v in tail_variants(cid, dtype).items():
            assert_exact_conditions(f"{cid}/tail{mode}", stored16=(v["res"], v["a"], v["y"]),
                                    acc_abs=(conv_fwd_ref(v["a"].abs(), w.abs(), c),), stats_of=(v["y"],))
    if "dgrad" in c.passes:
        o = epi_operands(cid)
        for key, v in dgrad_variants(cid, dtype).items():
            dz = v["dz"].abs().reshape(-1, c.Cin)
            assert_exact_conditions(
                f"{cid}/epi{key}", stored16=(o["y"], o["y2"], o["g2"], v["dz"], dx.abs() + o["g2"].abs()),
                acc_abs=(dz.sum(0), (dz * o["y"].abs().reshape(-1, c.Cin)).sum(0),
                         (dz * o["y2"].abs().reshape(-1, c.Cin)).sum(0)))
    for name, v in wgrad_variants(cid, dtype).items():
        if name == "pro":
            assert_exact_conditions(f"{cid}/wgrad/pro", stored16=(v["a"],),
                                    acc_abs=(conv_bwd_ref(v["a"].abs(), w.abs(), dy.abs(), c)[1],))
        elif name == "bna":
            assert_exact_conditions(f"{cid}/wgrad/bna", stored16=(v["y"], v["dY"]),
                                    acc_abs=(conv_bwd_ref(x.abs(), w.abs(), v["dY"].abs(), c)[1],))


# ------------------------------------------------------------------ guarded buffers
BAND = 1024   # bytes, a multiple of 256: the view keeps the alignment the kernels assume
_ES = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2, torch.uint8: 1, torch.float64: 8,
       torch.int32: 4, torch.int64: 8}


def guarded(shape, dtype, fill=None, device="cpu", band_byte: int = 0xA5):
    """(view, check): a contiguous ``shape`` view of ``dtype`` inside a larger byte buffer, with a
    poison band of ``band_byte`` bytes before it and one behind it (from the view's last byte to
    the buffer's end); ``check()`` is True while both bands are bit-unchanged. ``fill``: a tensor
    (copied in) or a scalar; None leaves NaN (float dtypes) inside. Inputs use ``band_byte`` 0xFF
    (NaN in every float format), outputs the 0xA5 sentinel."""
    n = 1
    for s in shape:
        n *= int(s)
    nbytes = n * _ES[dtype]
    total = BAND + (nbytes + 255) // 256 * 256 + BAND
    buf = torch.full((total,), band_byte, dtype=torch.uint8, device=device)
    view = buf[BAND:BAND + nbytes].view(dtype).view(*shape)
    if fill is None:
        if dtype.is_floating_point:
            view.fill_(float("nan"))
        else:
            view.zero_()
    elif isinstance(fill, torch.Tensor):
        view.copy_(fill.to(dtype) if fill.dtype != dtype else fill)
    else:
        view.fill_(fill)

    def check() -> bool:
        return bool((buf[:BAND] == band_byte).all()) and bool((buf[BAND + nbytes:] == band_byte).all())

    return view, check
