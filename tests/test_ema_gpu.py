"""The EMA kernel on the GPU (csrc/ema.hip, ops.native_ops.ema_update) against tests/ema_refs.py.

One buffer holds ranges of 1, 3, 4, 5, EMA_CHUNK - 1, EMA_CHUNK, EMA_CHUNK + 1 and 3 * EMA_CHUNK + 5
elements with gaps of at least 4 elements around each; the gaps of e, p and the shadow hold NaN
canaries. One ema_update call covers all eight ranges.

LERP bound, per element: |e - ref64| <= 3 * 2^-24 * (|p| + |e_old|) -- one rounding of the difference
p - e and one of the fused multiply-add under the shared float32 w (derivation in tests/ema_refs.py).
COPY, SWAP, everything outside the ranges, and p under LERP are compared bit for bit; the shadow
bit-equals torch's cast of the p the kernel stored.
"""
import functools

import pytest
import torch

import ema_refs as R
import head_refs as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
SHADOWS = {"none": None, "bf16": torch.bfloat16, "fp16": torch.float16}
WS = [0.0, 1.0, R.weight(0.9, 0, False), R.weight(0.9999, 0, False), R.weight(0.9, 0, True)]


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


@functools.lru_cache(maxsize=None)
def _layout():
    S = _k().EMA_CHUNK
    assert S == 4096
    off, spans = 4, []
    for size in (1, 3, 4, 5, S - 1, S, S + 1, 3 * S + 5):
        spans.append((off, size))
        off = (off + size + 3) // 4 * 4 + 4
    return off, spans


def _canary(n, dtype):
    if dtype == torch.float32:
        return torch.full((n,), 0x7FC0BEEF, dtype=torch.int64).to(torch.int32).view(torch.float32)
    bits = 0x7FC5 if dtype == torch.bfloat16 else 0x7E05
    return torch.full((n,), bits, dtype=torch.int16).view(dtype)


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


@functools.lru_cache(maxsize=None)
def _inputs(special: bool):
    """(n, e, p, inside): normal draws in the ranges, every 5th element with p == e and every 11th
    with e = 0; `special` (COPY / SWAP: bit moves) adds infinities, -0, a NaN and values past the
    fp16 range. Outside the ranges: canaries."""
    n, spans = _layout()
    g = H._gen(41)
    e, p = _canary(n, torch.float32).clone(), _canary(n, torch.float32).clone()
    inside = torch.zeros(n, dtype=torch.bool)
    for off, size in spans:
        ev, pv = torch.randn(size, generator=g), torch.randn(size, generator=g)
        ev[::11] = 0.0
        pv[::5] = ev[::5]
        if special and size > 8:
            ev[1:7] = torch.tensor([float("inf"), -0.0, 1e30, float("nan"), -float("inf"), 70000.0])
            pv[2:6] = torch.tensor([-0.0, float("inf"), -1e30, 65520.0])
        e[off:off + size], p[off:off + size] = ev, pv
        inside[off:off + size] = True
    assert int((~inside).sum()) >= 4 * (len(spans) + 1)
    return n, e, p, inside


@functools.lru_cache(maxsize=None)
def _run(mode_name, shadow_name, w=0.0, repeat=0):
    """One ema_update over the eight ranges; CPU copies (e, p, shadow) before and after."""
    K = _k()
    mode = getattr(K, "EMA_" + mode_name)
    sdt = SHADOWS[shadow_name]
    n, e0, p0, inside = _inputs(mode_name != "LERP")
    e, p = e0.to(DEV), p0.to(DEV)
    sh = _canary(n, sdt).to(DEV) if sdt is not None else None
    before = tuple(t.cpu() if t is not None else None for t in (e, p, sh))
    ranges = [(e[o:o + s], p[o:o + s]) + ((sh[o:o + s],) if sh is not None else ())
              for o, s in _layout()[1]]
    K.ema_update(ranges, mode, w)
    torch.cuda.synchronize()
    return before, tuple(t.cpu() if t is not None else None for t in (e, p, sh)), inside


def _assert_outside_intact(before, after, inside, tag):
    for name, a, b in zip(("e", "p", "shadow"), after, before):
        if a is None:
            continue
        bad = ((_bits(a) != _bits(b)) & ~inside).nonzero().flatten()[:8].tolist()
        assert not bad, f"{tag}: {name} written outside the ranges at {bad}"


@pytest.mark.parametrize("shadow", list(SHADOWS))
@pytest.mark.parametrize("w", WS, ids=[f"w{i}" for i in range(len(WS))])
def test_lerp_matches_the_float64_reference(shadow, w):
    before, after, inside = _run("LERP", shadow, w)
    (e0, p0, s0), (e1, p1, s1) = before, after
    ref = R.lerp64(e0, p0, w)           # (w = 1 too: against the reference, not against p)
    bound = R.lerp_bound(e0, p0)
    err = (e1.to(F64) - ref).abs()
    for off, size in _layout()[1]:
        sl = slice(off, off + size)
        assert bool(e1[sl].isfinite().all()), f"range at {off} of {size}"
        worst = float((err[sl] - bound[sl]).max())
        assert worst <= 0, f"range at {off} of {size}: {worst} over the bound"
    assert torch.equal(_bits(p1), _bits(p0)), "LERP must not write p"
    if s1 is not None:
        assert torch.equal(_bits(s1), _bits(s0)), "LERP must not write the shadow"
    same = inside & (p0 == e0)
    assert int(same.sum()) > 3000
    assert torch.equal(_bits(e1)[same], _bits(e0)[same]), "p == e must keep e's bits"
    if w == 0.0:
        assert torch.equal(_bits(e1), _bits(e0)), "w = 0 must keep e's bits"
    else:
        moved = inside & (p0 != e0)
        assert int((_bits(e1)[moved] != _bits(e0)[moved]).sum()) > 0.9 * int(moved.sum())
    _assert_outside_intact(before, after, inside, f"LERP {shadow} w={w}")


@pytest.mark.parametrize("shadow", list(SHADOWS))
def test_copy_is_bit_exact(shadow):
    before, after, inside = _run("COPY", shadow)
    (e0, p0, s0), (e1, p1, s1) = before, after
    we, wp = R.copy(e0, p0)
    assert torch.equal(_bits(e1)[inside], _bits(we)[inside])
    assert torch.equal(_bits(p1), _bits(wp))
    if s1 is not None:
        assert torch.equal(_bits(s1), _bits(s0)), "COPY must not write the shadow"
    _assert_outside_intact(before, after, inside, f"COPY {shadow}")


@pytest.mark.parametrize("shadow", list(SHADOWS))
def test_swap_is_bit_exact_and_refreshes_the_shadow(shadow):
    before, after, inside = _run("SWAP", shadow)
    (e0, p0, s0), (e1, p1, s1) = before, after
    we, wp = R.swap(e0, p0)
    assert torch.equal(_bits(e1)[inside], _bits(we)[inside])
    assert torch.equal(_bits(p1)[inside], _bits(wp)[inside])
    assert not torch.equal(_bits(e1)[inside], _bits(e0)[inside])
    if s1 is not None:
        assert bool(H.cast_matches(s1[inside], p1[inside]).all()), "shadow != torch's cast of the stored p"
        assert bool(s1[inside].isinf().any()) and bool(s1[inside].isnan().any())
    _assert_outside_intact(before, after, inside, f"SWAP {shadow}")


def test_two_runs_are_bit_equal():
    for mode, w in (("LERP", WS[2]), ("SWAP", 0.0)):
        a, b = _run(mode, "bf16", w), _run(mode, "bf16", w, repeat=1)
        assert a is not b
        for x, y in zip(a[1], b[1]):
            assert torch.equal(_bits(x), _bits(y)), mode


def test_a_swap_back_restores_every_bit():
    K = _k()
    n, e0, p0, inside = _inputs(True)
    e, p = e0.to(DEV), p0.to(DEV)
    sh = _canary(n, torch.float16).to(DEV)
    ranges = K.EmaRanges([(e[o:o + s], p[o:o + s], sh[o:o + s]) for o, s in _layout()[1]])
    K.ema_update(ranges, K.EMA_SWAP)
    first = sh.clone()
    K.ema_update(ranges, K.EMA_SWAP)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e), _bits(e0)) and torch.equal(_bits(p), _bits(p0))
    assert bool(H.cast_matches(sh.cpu()[inside], p0[inside]).all())
    assert not torch.equal(_bits(first), _bits(sh))


def test_more_ranges_than_one_launch_holds_and_empty_ones():
    """20 ranges (the launcher sends them out in groups) with two empty ones among them."""
    K = _k()
    g = H._gen(42)
    n = 20 * 16
    e0, p0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    e, p = e0.to(DEV), p0.to(DEV)
    sizes = [0 if i in (3, 8) else 5 + (i % 4) for i in range(20)]
    ranges = [(e[16 * i:16 * i + s], p[16 * i:16 * i + s]) for i, s in enumerate(sizes)]
    K.ema_update(ranges, K.EMA_COPY)
    torch.cuda.synchronize()
    inside = torch.zeros(n, dtype=torch.bool)
    for i, s in enumerate(sizes):
        inside[16 * i:16 * i + s] = True
    assert torch.equal(_bits(e)[inside], _bits(p0)[inside])
    assert torch.equal(_bits(e)[~inside], _bits(e0)[~inside]) and torch.equal(_bits(p), _bits(p0))
    K.ema_update([], K.EMA_COPY)


def test_refusals_launch_nothing():
    """A start offset by 4 bytes (e, p, and 2 bytes for the shadow), e aliasing p, overlapping rows,
    an f16 e, w = nan, w = 1.5, w < 0 and a bad mode: ValueError, and every buffer keeps its bits."""
    K = _k()
    g = H._gen(43)
    n = 64
    e, p = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    before = [t.clone() for t in (e, p, sh)]
    nan = float("nan")
    bad = {
        "e off by 4 bytes": ([(e[1:9], p[0:8])], K.EMA_LERP, 0.5),
        "p off by 4 bytes": ([(e[0:8], p[1:9])], K.EMA_COPY, 0.0),
        "shadow off by 2 bytes": ([(e[0:8], p[0:8], sh[1:9])], K.EMA_SWAP, 0.0),
        "e aliases p": ([(e[0:8], e[0:8])], K.EMA_LERP, 0.5),
        "e overlaps p": ([(e[0:8], e[4:12])], K.EMA_SWAP, 0.0),
        "two rows share e": ([(e[0:8], p[0:8]), (e[4:12], p[16:24])], K.EMA_LERP, 0.5),
        "f16 e": ([(e[0:8].half(), p[0:8])], K.EMA_LERP, 0.5),
        "f16 p": ([(e[0:8], p[0:8].half())], K.EMA_LERP, 0.5),
        "w nan": ([(e[0:8], p[0:8])], K.EMA_LERP, nan),
        "w 1.5": ([(e[0:8], p[0:8])], K.EMA_LERP, 1.5),
        "w negative": ([(e[0:8], p[0:8])], K.EMA_LERP, -0.25),
        "w inf": ([(e[0:8], p[0:8])], K.EMA_LERP, float("inf")),
        "mode": ([(e[0:8], p[0:8])], 3, 0.5),
    }
    for name, (ranges, mode, w) in bad.items():
        with pytest.raises(ValueError):
            K.ema_update(ranges, mode, w)
        torch.cuda.synchronize()
        for a, b in zip(before, (e, p, sh)):
            assert torch.equal(_bits(a), _bits(b)), name
    K.ema_update([(e[0:8], p[0:8], sh[0:8])], K.EMA_SWAP)      # (the good ranges do launch)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e[0:8]), _bits(before[1][0:8]))
    assert torch.equal(_bits(e[8:]), _bits(before[0][8:])) and torch.equal(_bits(p[8:]), _bits(before[1][8:]))
