"""The stand-alone train-time BatchNorm kernels of csrc/bn.hip -- apply, backward reduce, the two
backward finalizes, backward apply (one and two branches), forward statistics, finalize from
totals, slab reduce -- pinned element by element.

Every comparison is made on the CPU against tests/bn_refs.py (plain float64 torch; premises proven
in tests/test_bn_refs_cpu.py). The activation kernels run on exact dyadic data: each stored value
must equal the float64 reference rounded once to the storage dtype (``==`` per element, so +0 and
-0 agree -- fmaxf(-0, 0) may return either), masks and integer sums must be equal, and the poison
bands around every output must be untouched. The statistics kernels sum integer partials in f64
(exact), so their two implementations must agree bit for bit, and each output lies within one
f32 spacing of the float64 formula.

Parameter values are combined as covering designs, not full cross products: inside a test every
listed value of every parameter occurs, rotated against the others by the loop indices, and the
mismatches are collected in a ``bad`` list."""
import itertools
import math

import pytest
import torch

import bn_refs as B
import conv_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
DTS = sorted(B.DTYPES)
DTS16 = ["bf16", "f16"]


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K, ext, ext.lib()


def _in(t64, dtype):
    """Device operand (the float64 value, exact in ``dtype``) behind NaN bands; None stays None."""
    if t64 is None:
        return None
    v = B.to_dtype(t64, dtype)
    assert torch.equal(v.to(F64), t64), "operand not representable"
    return R.guarded(t64.shape, dtype, fill=v, device=DEV, band_byte=0xFF)[0]


def _out(shape, dtype, fill=None):
    """Device output: NaN (or ``fill``) inside, sentinel bands; (view, band check)."""
    return R.guarded(shape, dtype, fill=fill, device=DEV)


def _eq(bad, tag, got, ref):
    """``got`` (device) == ``ref`` (CPU, same dtype) per element: bit equality except +0 == -0."""
    g = got.detach().cpu()
    assert g.dtype == ref.dtype and g.shape == ref.shape, (tag, g.dtype, ref.dtype, g.shape, ref.shape)
    ne = ~(g.to(F64) == ref.to(F64)) if g.dtype.is_floating_point else g != ref
    if bool(ne.any()):
        i = tuple(ne.nonzero()[0].tolist())
        bad.append((tag, f"{int(ne.sum())} of {ne.numel()} differ, first at {i}: {g[i].item()} != {ref[i].item()}"))


def _ulp(bad, tag, got, ref64, extra=0.0):
    ok, worst = B.within_ulp(got.detach().cpu(), ref64, F32, extra)
    if not bool(ok.all()):
        bad.append((tag, f"{int((~ok).sum())} of {ok.numel()} beyond one f32 spacing, worst x{worst:.4g}"))


def _guards(bad, tag, *checks):
    for i, chk in enumerate(checks):
        if not chk():
            bad.append((tag, f"guard band {i} overwritten"))


def _apply_args(d, dtype):
    dev = {k: _in(d[k], dtype) for k in ("y", "r2")}
    dev.update({k: _in(d[k], F32) for k in ("sc", "sh", "sc2", "sh2")})
    return dev


def _run_apply(K, bad, tag, d, dev, dtype, relu, with_mask, rows=None, idx=None):
    """One bn_apply launch of case ``d`` (optionally tiled by ``idx``) checked against the
    reference: out == ref rounded once, mask == (ref > 0) from the reference, bands intact."""
    mode, C = d["mode"], d["C"]
    rows = rows or d["rows"]
    ref = B.apply_ref(d["y"], d["sc"], d["sh"], mode, relu, d["r2"], d["sc2"], d["sh2"])
    ref16, mref = B.to_dtype(ref, dtype), B.mask_bytes(ref).view(-1, C // 8)
    if idx is not None:
        ref16, mref = ref16[idx], mref[idx]
    out, c1 = _out((rows, C), dtype)
    mask, c2 = _out((rows * C // 8,), torch.uint8, fill=0xEE)
    K.bn_apply(dev["y"], dev["sc"], dev["sh"], out, res=dev["r2"] if mode == 1 else None,
               y2=dev["r2"] if mode == 2 else None, scale2=dev["sc2"], shift2=dev["sh2"], relu=relu,
               mask=mask if with_mask else None)
    torch.cuda.synchronize()
    _eq(bad, tag + ("out",), out, ref16)
    _eq(bad, tag + ("mask",), mask, mref.reshape(-1) if with_mask else torch.full_like(mref.reshape(-1), 0xEE))
    _guards(bad, tag, c1, c2)


# ------------------------------------------------------------------ bn_apply
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_bn_apply_exact(dt, mode):
    """The one-chunk kernel: every shape (one row, ragged rows, a stride that is a multiple of a
    non-power-of-two C/8, several blocks, C = 2048), ReLU on and off, mask given and null."""
    K, ext, L = _k()
    dtype, bad = B.DTYPES[dt], []
    try:
        L.pda_set_stream_cfg(*B.ONE_CHUNK)
        for rows, C in B.APPLY_SHAPES:
            d = B.bn_case(rows, C, mode)
            dev = _apply_args(d, dtype)
            for relu, with_mask in itertools.product((True, False), (True, False)):
                _run_apply(K, bad, (rows, C, relu, with_mask), d, dev, dtype, relu, with_mask)
    finally:
        L.pda_set_stream_cfg(*ext.stream_cfg())
    assert not bad, bad


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("cfg", B.STREAM_CFGS)
def test_bn_apply_streaming_exact(cfg, dt):
    """The U-chunk kernels under every streaming configuration; for U > 1 the loop bounds say that
    the whole-batch loop iterates and that the remainder loop gets chunks."""
    K, ext, L = _k()
    dtype, bad = B.DTYPES[dt], []
    try:
        L.pda_set_stream_cfg(*cfg)
        for (rows, C), mode in itertools.product(B.STREAM_SHAPES, (0, 1, 2)):
            if cfg[0] != 0 and B.stream_chunks(cfg) > 1:
                batch, rem = B.stream_loops(cfg, rows * C // 8, C)
                assert batch > 0 and rem > 0, (cfg, rows, C)
            d = B.bn_case(rows, C, mode)
            _run_apply(K, bad, (rows, C, mode), d, _apply_args(d, dtype), dtype, True, True)
    finally:
        L.pda_set_stream_cfg(*ext.stream_cfg())
    assert not bad, bad


@pytest.mark.parametrize("mode", [0, 2])
def test_bn_apply_second_trip_other_channels(mode):
    """bf16, C = 24, n8 = 8192 * 256 + 1: the one-chunk kernel's grid is capped, its stride is no
    multiple of C/8, and the chunk past the stride needs other channels' coefficients than its
    thread's first one (the per-trip reload). ~34 MB per tensor, a small exact block tiled. The
    read-back backward apply shares the loop form and runs on the same data."""
    K, ext, L = _k()
    dtype, bad = torch.bfloat16, []
    rows, C = B.BIG_ROWS, B.BIG_C
    d, idx = B.tiled_case(B.BIG_BLOCK, rows, C, mode)
    assert rows * C // 8 > 8192 * 256 and (8192 * 256) % (C // 8) != 0
    dev = {k: (None if d[k] is None else B.to_dtype(d[k], dtype)[idx].to(DEV)) for k in ("y", "r2")}
    dev.update({k: _in(d[k], F32) for k in ("sc", "sh", "sc2", "sh2")})
    try:
        L.pda_set_stream_cfg(*B.ONE_CHUNK)
        _run_apply(K, bad, ("apply",), d, dev, dtype, True, True, rows=rows, idx=idx)
        if mode == 0:
            dz = B.dz_ref(d["g1"], 0, d["pre"])
            k = d["k"]
            dzd = B.to_dtype(dz, dtype)[idx].to(DEV)
            dy, chk = _out((rows, C), dtype)
            a = K.BwdArgs(None, None, None, 0, K.ptr(dev["y"]), None, None, None, None, None, 1, None,
                          None, 2, rows, C)
            kd = _in(k, F32)
            K.check(L.pda_bn_bwd_apply(ext.C.byref(a), K.ptr(dzd), K.ptr(dev["y"]), K.ptr(kd[0]),
                                       K.ptr(kd[1]), K.ptr(kd[2]), K.ptr(dy), ext.dt_of(dtype),
                                       K.stream(torch.device(DEV))), "bn_bwd_apply")
            torch.cuda.synchronize()
            _eq(bad, ("bwd_apply",), dy, B.to_dtype(B.bwd_apply_ref(dz, d["y"], *k[:3]), dtype)[idx])
            _guards(bad, ("bwd_apply",), chk)
    finally:
        L.pda_set_stream_cfg(*ext.stream_cfg())
    assert not bad, bad


# ------------------------------------------------------------------ bn_bwd_reduce
def _bwd_args(K, d, dev, mode, nq, dz_out, part):
    rows, C = d["rows"], d["C"]
    y2 = dev["r2"] if mode in (1, 2) else None
    masked = mode != 3
    return K.BwdArgs(K.ptr(dev.get("g1")), K.ptr(dev.get("g2")), K.ptr(dev.get("gp")), d.get("HW", 0),
                     K.ptr(dev["y"]), K.ptr(dev["sc"]) if masked else None,
                     K.ptr(dev["sh"]) if masked else None, K.ptr(y2),
                     K.ptr(dev["sc2"]) if mode == 2 else None, K.ptr(dev["sh2"]) if mode == 2 else None,
                     mode, K.ptr(dz_out), K.ptr(part), nq, rows, C)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dt", DTS)
def test_bn_bwd_reduce_exact(dt, mode):
    """pda_bn_bwd_reduce with the block count chosen here: every C (24 and 192 leave idle threads,
    4096 takes a second channel pass) x rows x G (one block, several, one row each, more blocks
    than rows -- whose partials are zero) x the gradient forms g1, g1 + g2, gp with HW 1 and gp
    with HW 49 (C >= 2048: one form per (rows, G), rotated). Partials == the float64 sums per block and q, dz == the reference
    rounded once; HW = 49 (1/49 is no dyadic value): each partial within n * 2^-23 * sum |terms| of
    the float64 sum over its n rows, dz within one spacing of the storage dtype."""
    K, ext, L = _k()
    dtype, bad = B.DTYPES[dt], []
    nq = 3 if mode == 2 else 2
    st = K.stream(torch.device(DEV))
    for (ci, C), (ri, rows) in itertools.product(enumerate(B.REDUCE_C), enumerate(B.REDUCE_ROWS)):
        for G, form in itertools.product(B.reduce_G(rows), B.GRAD_FORMS):
            if C >= 2048 and form != B.GRAD_FORMS[(ci + ri + B.reduce_G(rows).index(G)) % 4]:
                continue                          # the wide rows: one form per (rows, G), rotated
            d = B.reduce_case(rows, C, mode, form)
            tag = (C, rows, G, form)
            dev = _apply_args(d, dtype)
            dev.update({k: _in(d[k], dtype) for k in ("g1", "g2", "gp")})
            dz, c1 = _out((rows, C), dtype)
            part, c2 = _out((G, nq, C), F32)
            a = _bwd_args(K, d, dev, mode, nq, dz, part)
            K.check(L.pda_bn_bwd_reduce(ext.C.byref(a), G, ext.dt_of(dtype), st), "bn_bwd_reduce")
            torch.cuda.synchronize()
            pref = B.partials_ref(d["dz"], d["y"], d["y2"], G)
            if d["exact"]:
                _eq(bad, tag + ("part",), part, pref.float())
                assert torch.equal(pref.float().to(F64), pref)
                _eq(bad, tag + ("dz",), dz, B.to_dtype(d["dz"], dtype))
            else:
                n = torch.tensor([max(r1 - r0, 1) for r0, r1 in B.block_rows(rows, G)], dtype=F64)
                bound = n[:, None, None] * B.EPS32 * B.partials_ref(d["dz"], d["y"], d["y2"], G, absolute=True)
                err = (part.cpu().to(F64) - pref).abs()
                if not bool((err <= bound).all()):
                    bad.append((tag + ("part",), f"worst error / bound {float((err / bound).nan_to_num(0).max()):.3g}"))
                ok, worst = B.within_ulp(dz.cpu(), d["dz"], dtype)
                if not bool(ok.all()):
                    bad.append((tag + ("dz",), f"worst x{worst:.3g} of one spacing"))
            for b, (r0, r1) in enumerate(B.block_rows(rows, G)):
                if r1 <= r0 and not bool((part[b] == 0).all()):
                    bad.append((tag, f"block {b} owns no row but wrote non-zero partials"))
            _guards(bad, tag, c1, c2)
    assert not bad, bad[:8]


# ------------------------------------------------------------------ bn_bwd_finalize / bn_bwd_stats
def _cg(C, cg):
    if cg <= 0 or cg > 256 or (cg & (cg - 1)) or cg < 4:
        cg = 256
    return min(C, cg)


_BWD_CFGS = list(itertools.product((0, 1), (1.0, 0.5, 1.0 / 3), (1, 2)))   # accumulate, gscale, count / rows


@pytest.mark.parametrize("C", B.STATS_C)
@pytest.mark.parametrize("T", B.STATS_T)
def test_bn_bwd_finalize_and_stats_agree(T, C):
    """bn_bwd_finalize (two launches for two branches) and bn_bwd_stats (one launch: f64 slabs,
    last arriver) on the same integer partials, nq 2 and 3, S in {1, 8, T} x cg in {0, 4, 64, 256}
    (a C below cg that is no power of two, one quad per group, ragged last groups), with
    (accumulate, gscale, count = rows or 2 rows) rotated and generic / dyadic coefficients
    alternating: the two kernels' outputs are torch.equal; each lies within one f32 spacing of the
    float64 formula (k3: plus its cancellation allowance) and is bit-equal to it where everything
    is dyadic; accumulate adds the same f32 term to the old gradient; the arrival counters are zero
    afterwards and a second launch on the same workspace repeats every bit."""
    K, ext, L = _k()
    bad = []
    st = K.stream(torch.device(DEV))
    combos = [(S, cg) for S in sorted({1, 8, T}) for cg in (0, 4, 64, 256)]
    for nq, (j, (S, cg)) in itertools.product((2, 3), enumerate(combos)):
        nb = nq - 1
        acc, gscale, cmul = _BWD_CFGS[(j + 5 * nq + T + C // 4) % len(_BWD_CFGS)]
        dyadic = (j + nq + T) % 2 == 0
        d = B.bwd_stats_case(T, C, nq, dyadic)
        count = float((1024 if dyadic else 1000) * cmul)
        tag = (nq, S, cg, acc, round(gscale, 3), count, dyadic)
        part = _in(d["part"], F32)
        prm = [{k: _in(v, F32) for k, v in d[b].items()} for b in range(nb)]
        groups = -(-C // _cg(C, cg))
        slabs, cs = _out((max(S, 1) * nq * C,), F64)
        cnt, cc = _out((groups,), torch.int32, fill=0)

        def stats(kbuf, gbuf, accumulate):
            o = ext.BnBwdOut(count, gscale, accumulate)
            for b in range(nb):
                o.gamma[b], o.mean[b], o.invstd[b] = (K.ptr(prm[b][n]) for n in ("gamma", "mean", "invstd"))
                o.dgamma[b], o.dbeta[b] = K.ptr(gbuf[b][0]), K.ptr(gbuf[b][1])
            o.k = K.ptr(kbuf)
            return L.pda_bn_bwd_stats(K.ptr(part), T, nq, C, S, K.ptr(slabs), K.ptr(cnt), ext.C.byref(o), cg, st)

        def finalize(kbuf, gbuf, accumulate):
            for b in range(nb):
                K.check(L.pda_bn_bwd_finalize(K.ptr(part), T, nq, 1 + b, C, count, K.ptr(prm[b]["gamma"]),
                                              K.ptr(prm[b]["mean"]), K.ptr(prm[b]["invstd"]),
                                              K.ptr(gbuf[b][0]), K.ptr(gbuf[b][1]), K.ptr(kbuf[b][0]),
                                              K.ptr(kbuf[b][1]), K.ptr(kbuf[b][2]), gscale, accumulate, st),
                        "bn_bwd_finalize")
            return 0

        if S > T:
            kb, c1 = _out((nb, 3, C), F32)
            gb, c2 = _out((nb, 2, C), F32)
            rc = stats(kb, gb, 0)
            torch.cuda.synchronize()
            if rc != -2 or not bool(kb.isnan().all()) or not bool(gb.isnan().all()):
                bad.append((tag, f"S > T: rc {rc}, or something written"))
            continue
        runs = {}
        for name, fn in (("finalize", finalize), ("stats", stats), ("stats again", stats)):
            kb, c1 = _out((nb, 3, C), F32)
            gb, c2 = _out((nb, 2, C), F32)
            K.check(fn(kb, gb, 0), name)
            torch.cuda.synchronize()
            _guards(bad, tag + (name,), c1, c2, cs, cc)
            runs[name] = (kb.cpu(), gb.cpu())
            if int(cnt.abs().sum()) != 0:
                bad.append((tag + (name,), "arrival counters not zero"))
        for other in ("stats", "stats again"):
            if not (torch.equal(runs["finalize"][0], runs[other][0]) and torch.equal(runs["finalize"][1], runs[other][1])):
                bad.append((tag, f"finalize and '{other}' differ"))
        kb, gb = runs["stats"]
        exact = dyadic and gscale != 1.0 / 3
        for b in range(nb):
            p = d[b]
            r = B.bwd_finalize_ref(d["tot"][0], d["tot"][1 + b], p["gamma"], p["mean"], p["invstd"], count, gscale)
            for name, got, extra in (("dgamma", gb[b][0], 0.0), ("dbeta", gb[b][1], 0.0), ("k1", kb[b][0], 0.0),
                                     ("k2", kb[b][1], 0.0), ("k3", kb[b][2], r["k3_extra"])):
                _ulp(bad, tag + (b, name), got, r[name], extra)
                if exact:
                    _eq(bad, tag + (b, name, "dyadic"), got, r[name].float())
        if acc:
            for name, fn in (("finalize", finalize), ("stats", stats)):
                kb2, c1 = _out((nb, 3, C), F32)
                old = torch.stack([torch.stack([d[b]["dgamma"], d[b]["dbeta"]]) for b in range(nb)]).float()
                gb2, c2 = _out((nb, 2, C), F32, fill=old)
                K.check(fn(kb2, gb2, 1), name)
                torch.cuda.synchronize()
                _eq(bad, tag + (name, "accumulate"), gb2, gb + old)     # one f32 add of the same term
                _eq(bad, tag + (name, "accumulate k"), kb2, kb)
                _guards(bad, tag + (name, "accumulate"), c1, c2)
    assert not bad, bad[:8]


# ------------------------------------------------------------------ bn_bwd_apply / bn_bwd_apply2
@pytest.mark.parametrize("form", ["dz_in", "recompute0", "recompute3"])
@pytest.mark.parametrize("dt", DTS)
def test_bn_bwd_apply_exact(dt, form):
    """dy = k1*dz + k2*y + k3 with dz read back (bn_bwd_apply_dz_kernel) or recomputed from the
    gradient and the mask (bn_bwd_apply_kernel: mode 0, and mode 3 without a mask)."""
    K, ext, L = _k()
    dtype, bad = B.DTYPES[dt], []
    mode = 3 if form == "recompute3" else 0
    st = K.stream(torch.device(DEV))
    try:
        L.pda_set_stream_cfg(*B.ONE_CHUNK)
        for rows, C in B.APPLY_SHAPES:
            d = B.reduce_case(rows, C, mode, "g1")
            dev = _apply_args(d, dtype)
            dev["g1"] = _in(d["g1"], dtype)
            kd = _in(d["k"], F32)
            dy, chk = _out((rows, C), dtype)
            if form == "dz_in":
                a = K.BwdArgs(None, None, None, 0, K.ptr(dev["y"]), None, None, None, None, None, 1, None,
                              None, 2, rows, C)
                dz_in = _in(d["dz"], dtype)
            else:
                a, dz_in = _bwd_args(K, d, dev, mode, 2, None, None), None
            K.check(L.pda_bn_bwd_apply(ext.C.byref(a), K.ptr(dz_in), K.ptr(dev["y"]), K.ptr(kd[0]),
                                       K.ptr(kd[1]), K.ptr(kd[2]), K.ptr(dy), ext.dt_of(dtype), st),
                    "bn_bwd_apply")
            torch.cuda.synchronize()
            _eq(bad, (rows, C), dy, B.to_dtype(B.bwd_apply_ref(d["dz"], d["y"], *d["k"][:3]), dtype))
            _guards(bad, (rows, C), chk)
    finally:
        L.pda_set_stream_cfg(*ext.stream_cfg())
    assert not bad, bad


def _apply2(K, ext, L, d, dtype, rows, C):
    dz, y, y2 = (_in(d[k], dtype) for k in ("dz", "y", "r2"))
    kd = _in(d["k"], F32)
    dy, c1 = _out((rows, C), dtype)
    dy2, c2 = _out((rows, C), dtype)
    rc = L.pda_bn_bwd_apply2(K.ptr(dz), K.ptr(y), K.ptr(y2), K.ptr(kd), K.ptr(dy), K.ptr(dy2), rows, C,
                             ext.dt_of(dtype), K.stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, dy, dy2, (c1, c2), (dz, y, y2, kd)


@pytest.mark.parametrize("dt", DTS16)
@pytest.mark.parametrize("cfg", B.STREAM_CFGS)
def test_bn_bwd_apply_streaming_exact(cfg, dt):
    """bn_bwd_apply2 (both branches of a downsample tail in one pass over dz) and the read-back
    bn_bwd_apply under every streaming configuration."""
    K, ext, L = _k()
    dtype, bad = B.DTYPES[dt], []
    try:
        L.pda_set_stream_cfg(*cfg)
        for rows, C in B.STREAM_SHAPES:
            d = B.reduce_case(rows, C, 2, "g1")
            k = d["k"]
            ref = [B.to_dtype(B.bwd_apply_ref(d["dz"], ys, *k[3 * b:3 * b + 3]), dtype)
                   for b, ys in ((0, d["y"]), (1, d["r2"]))]
            rc, dy, dy2, chks, (dz, y, _, kd) = _apply2(K, ext, L, d, dtype, rows, C)
            assert rc == 0, (cfg, rows, C, rc)
            _eq(bad, (rows, C, "dy"), dy, ref[0])
            _eq(bad, (rows, C, "dy2"), dy2, ref[1])
            _guards(bad, (rows, C), *chks)
            dy1, chk = _out((rows, C), dtype)
            a = K.BwdArgs(None, None, None, 0, K.ptr(y), None, None, None, None, None, 1, None, None, 2,
                          rows, C)
            K.check(L.pda_bn_bwd_apply(ext.C.byref(a), K.ptr(dz), K.ptr(y), K.ptr(kd[0]), K.ptr(kd[1]),
                                       K.ptr(kd[2]), K.ptr(dy1), ext.dt_of(dtype),
                                       K.stream(torch.device(DEV))), "bn_bwd_apply")
            torch.cuda.synchronize()
            _eq(bad, (rows, C, "one branch"), dy1, ref[0])
            _guards(bad, (rows, C, "one branch"), chk)
    finally:
        L.pda_set_stream_cfg(*ext.stream_cfg())
    assert not bad, bad


def test_bn_bwd_apply2_falls_back():
    """-1 and nothing written for f32 and for a C whose channel chunk would change along a thread's
    trips (grid * 256 % (C/8) != 0); native_ops.bn_bwd_finish then gives the same bits through
    its two one-branch passes, from coefficients the statistics kernel computed (dyadic, so the
    float64 formula is exact)."""
    K, ext, L = _k()
    bad = []
    rows, C = 128, 24
    assert (-(-rows * C // 8 // 256) * 256) % (C // 8) != 0
    d = B.reduce_case(rows, C, 2, "g1")
    for dtype, r_, c_ in ((torch.float32, 203, 64), (torch.bfloat16, rows, C), (torch.float16, rows, C)):
        dd = B.reduce_case(r_, c_, 2, "g1")
        rc, dy, dy2, chks, _ = _apply2(K, ext, L, dd, dtype, r_, c_)
        if rc != -1 or not bool(dy.isnan().all()) or not bool(dy2.isnan().all()):
            bad.append((dtype, f"rc {rc}, or something written"))
        _guards(bad, (dtype,), *chks)
    s = B.bwd_stats_case(1, C, 3, True)
    refs = [B.bwd_finalize_ref(s["tot"][0], s["tot"][1 + b], s[b]["gamma"], s[b]["mean"], s[b]["invstd"],
                               float(rows), 1.0) for b in range(2)]
    kref = torch.stack([r[n] for r in refs for n in ("k1", "k2", "k3")])
    assert B.representable(kref, (F32,))
    dyref = [B.bwd_apply_ref(d["dz"], ys, *kref[3 * b:3 * b + 3]) for b, ys in ((0, d["y"]), (1, d["r2"]))]
    for b, ys in ((0, d["y"]), (1, d["r2"])):       # the premise: exact in f32
        dy32 = B.bwd_apply_ref(d["dz"].float(), ys.float(), *kref[3 * b:3 * b + 3].float())
        assert torch.equal(dy32.to(F64), dyref[b])
    for dtype in (torch.bfloat16, torch.float16):
        ws = K.Workspace(torch.device(DEV))
        dz, y, y2 = (_in(d[k], dtype).view(1, rows, 1, C) for k in ("dz", "y", "r2"))
        prm = [{k: _in(v, F32) for k, v in s[b].items()} for b in range(2)]
        gb, c0 = _out((2, 2, C), F32)
        kb, c1 = _out((6 * C,), F32)
        dy, c2 = _out((1, rows, 1, C), dtype)
        dy2, c3 = _out((1, rows, 1, C), dtype)
        K.bn_bwd_finish(ws, _in(s["part"], F32), 1, 3, y, prm[0]["mean"], prm[0]["invstd"], prm[0]["gamma"],
                        gb[0][0], gb[0][1], dz, dy, y2=y2, mean2=prm[1]["mean"], invstd2=prm[1]["invstd"],
                        gamma2=prm[1]["gamma"], dgamma2=gb[1][0], dbeta2=gb[1][1], dy2_out=dy2, k_out=kb)
        torch.cuda.synchronize()
        _eq(bad, (dtype, "k"), kb.view(6, C), kref.float())
        _eq(bad, (dtype, "dy"), dy.view(rows, C), B.to_dtype(dyref[0], dtype))
        _eq(bad, (dtype, "dy2"), dy2.view(rows, C), B.to_dtype(dyref[1], dtype))
        _eq(bad, (dtype, "dgamma"), gb[:, 0], torch.stack([r["dgamma"] for r in refs]).float())
        _eq(bad, (dtype, "dbeta"), gb[:, 1], torch.stack([r["dbeta"] for r in refs]).float())
        _guards(bad, (dtype,), c0, c1, c2, c3)
    assert not bad, bad


# ------------------------------------------------------------------ forward statistics
EPS, MOM = 1e-5, 0.1
_FWD_OUT = ("mean", "invstd", "scale", "shift", "rmean", "rvar")


def _fwd_bufs(p):
    """Guarded outputs: mean / invstd / scale / shift (NaN), running statistics (the old ones),
    num_batches_tracked (7)."""
    o = {n: _out(p["gamma"].shape, F32, fill=(B.to_dtype(p[n], F32) if n in p else None)) for n in _FWD_OUT}
    o["nbt"] = _out((1,), torch.int64, fill=7)
    return o


def _fwd_verify(bad, tag, o, tot, count, p, update, nbt_given=True):
    got = {n: o[n][0].cpu() for n in _FWD_OUT}
    bad += [(tag, m) for m in B.fwd_checks(got, tot, count, p, EPS, MOM, update)]
    want = 8 if (update and nbt_given) else 7
    if int(o["nbt"][0].item()) != want:
        bad.append((tag, f"num_batches_tracked {int(o['nbt'][0].item())} != {want}"))
    _guards(bad, tag, *(v[1] for v in o.values()))


@pytest.mark.parametrize("C", B.FWD_C)
@pytest.mark.parametrize("T,bm,M", B.FWD_CASES)
def test_bn_fwd_stats(T, bm, M, C):
    """bn_fwd_stats on integer shifted partials with a ragged last tile (and M = 1: the biased
    variance feeds the running one): cg in {0, 4, 32, 256} x S in {1, T}; ``tot`` == the integer
    totals with nothing else written; finalized outputs within the bounds of bn_refs.fwd_checks;
    update = 0 leaves rmean, rvar and num_batches_tracked bit-untouched; counters end at zero."""
    K, ext, L = _k()
    bad = []
    d = B.fwd_stats_case(T, C, bm, M)
    part = _in(d["part"], F32)
    gamma, beta = _in(d["gamma"], F32), _in(d["beta"], F32)
    st = K.stream(torch.device(DEV))
    for j, (cg, S) in enumerate(itertools.product((0, 4, 32, 256), sorted({1, T}))):
        slabs, cs = _out((S * 2 * C,), F64)
        cnt, cc = _out((-(-C // _cg(C, cg)),), torch.int32, fill=0)
        for variant in ("tot", "update", "keep"):
            if variant == "keep" and j % 2:
                continue
            tag = (cg, S, variant)
            o = _fwd_bufs(d)
            tot, ct = _out((2, C), F64)
            fo = ext.BnFwdOut(K.ptr(gamma), K.ptr(beta), EPS, MOM, *(K.ptr(o[n][0]) for n in _FWD_OUT),
                              K.ptr(o["nbt"][0]), int(variant != "keep"), K.ptr(tot) if variant == "tot" else None)
            K.check(L.pda_bn_fwd_stats(K.ptr(part), T, C, bm, M, S, K.ptr(slabs), K.ptr(cnt),
                                       ext.C.byref(fo), cg, st), "bn_fwd_stats")
            torch.cuda.synchronize()
            if variant == "tot":
                _eq(bad, tag, tot, d["tot"])
                if not all(bool(o[n][0].isnan().all()) for n in _FWD_OUT[:4]) or int(o["nbt"][0].item()) != 7 \
                        or not torch.equal(o["rmean"][0].cpu(), d["rmean"].float()):
                    bad.append((tag, "the totals form wrote a finalized output"))
                _guards(bad, tag, ct, *(v[1] for v in o.values()))
            else:
                _fwd_verify(bad, tag, o, d["tot"], float(M), d, variant == "update")
            if int(cnt.abs().sum()) != 0:
                bad.append((tag, "arrival counters not zero"))
            _guards(bad, tag, cs, cc)
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", ["totals", "clamp", "count1"])
def test_bn_finalize_tot(case):
    """bn_finalize_tot (the SyncBatchNorm finalize from all-reduced f64 totals): same bounds as
    bn_fwd_stats; update_running = 0 leaves the running statistics untouched; a null
    num_batches_tracked is accepted; totals with E[y^2] < mean^2 clamp to invstd ==
    (float)(1 / sqrt(eps)); count = 1 keeps the biased variance."""
    K, ext, L = _k()
    bad = []
    st = K.stream(torch.device(DEV))
    for C in (4, 192, 1028):
        if case == "totals":
            d = B.fwd_stats_case(97, C, 64, 97 * 64 - 1)
            tot, count = d["tot"], 2.0 * (97 * 64 - 1)        # two ranks: doubled count
            tot = 2 * tot
        else:
            g = B._gen(C)
            d = B.stat_params(C, g)
            s1 = torch.randint(-40, 41, (C,), generator=g).to(F64)
            if case == "clamp":
                count, tot = 4.0, torch.stack([s1 * 4 + 2, 4 * s1 * s1])   # E[y^2] = s1^2 < (s1 + 1/2)^2
                tot = torch.where(s1 >= 0, tot, torch.stack([s1 * 4 - 2, 4 * s1 * s1]))
            else:
                count, tot = 1.0, torch.stack([s1, s1 * s1])
        gamma, beta, totd = _in(d["gamma"], F32), _in(d["beta"], F32), _in(tot, F64)
        for update, nbt_given in ((1, True), (0, True), (1, False)):
            tag = (C, update, nbt_given)
            o = _fwd_bufs(d)
            K.check(L.pda_bn_finalize_tot(K.ptr(totd), C, count, K.ptr(gamma), K.ptr(beta), EPS, MOM,
                                          *(K.ptr(o[n][0]) for n in _FWD_OUT),
                                          K.ptr(o["nbt"][0]) if nbt_given else None, update, st),
                    "bn_finalize_tot")
            torch.cuda.synchronize()
            _fwd_verify(bad, tag, o, tot, count, d, bool(update), nbt_given)
            if case != "totals":
                want = torch.full((C,), 1.0 / math.sqrt(B.f32c(EPS)), dtype=F64).float()
                _eq(bad, tag + ("invstd",), o["invstd"][0], want)
    assert not bad, bad[:8]


# ------------------------------------------------------------------ slab_reduce
@pytest.mark.parametrize("G", B.SLAB_G)
def test_slab_reduce(G):
    """[G][QC] -> [s][QC] on integer data: ``==``, the returned slab count s = ceil(G / ceil(G / S)),
    G % 4 tails, S above G, QC across the 256-thread block edge."""
    K, ext, L = _k()
    bad = []
    for QC, S in itertools.product(B.SLAB_QC, (1, 96, G + 5)):
        x = torch.randint(-8, 9, (G, QC), generator=B._gen(G * 7 + QC + S)).to(F64)
        ref, s = B.slab_ref(x, G, S)
        out, chk = _out((s, QC), F32)
        xd = _in(x, F32)
        rc = L.pda_slab_reduce(K.ptr(xd), G, QC, S, K.ptr(out), K.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        if rc != s:
            bad.append(((QC, S), f"returned {rc} slabs, not {s}"))
        _eq(bad, (QC, S), out, ref.float())
        _guards(bad, (QC, S), chk)
    assert not bad, bad[:8]


# ------------------------------------------------------------------ refused shapes
def test_bn_shape_refusals():
    """Shapes the kernels cannot walk are refused with -2 before any launch (outputs and bands
    stay as they were), and native_ops raises ValueError naming the shape: C % 8 != 0, C < 8, an
    element count that is no multiple of C; for the reduce also C > 2048 that is no multiple of
    2048 (its channel passes have no tail check), G <= 0 and rows <= 0."""
    K, ext, L = _k()
    st = K.stream(torch.device(DEV))
    dtype, dt = torch.bfloat16, ext.dt_of(torch.bfloat16)
    n = 4 * 2056
    x = torch.ones(n, dtype=dtype, device=DEV)
    co = torch.ones(2056 * 6, dtype=F32, device=DEV)
    out, c1 = _out((n,), dtype)
    out2, c2 = _out((n,), dtype)
    part, c3 = _out((4 * 3 * 2056,), F32)
    mask, c4 = _out((n // 8,), torch.uint8, fill=0xEE)
    P = K.ptr
    for numel, C in ((36, 12), (16, 4), (64 * 3 + 8, 64), (0, 0)):
        assert L.pda_bn_apply(P(x), P(co), P(co), P(x), P(co), P(co), P(out), numel, C, 2, 1, P(mask), dt, st) == -2
    for rows, C, G in ((3, 12, 1), (3, 4, 1), (2, 2056, 1), (2, 4104, 2), (3, 64, 0), (0, 64, 1), (3, 0, 1)):
        a = K.BwdArgs(P(x), None, None, 0, P(x), P(co), P(co), P(x), P(co), P(co), 2, P(out), P(part), 3, rows, C)
        assert L.pda_bn_bwd_reduce(ext.C.byref(a), G, dt, st) == -2, (rows, C, G)
        if G == 1 and rows > 0 and C not in (2056, 4104):
            assert L.pda_bn_bwd_apply(ext.C.byref(a), P(x), P(x), P(co), P(co), P(co), P(out), dt, st) == -2
            assert L.pda_bn_bwd_apply(ext.C.byref(a), None, P(x), P(co), P(co), P(co), P(out), dt, st) == -2
            assert L.pda_bn_bwd_apply2(P(x), P(x), P(x), P(co), P(out), P(out2), rows, C, dt, st) == -2
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(out2.isnan().all()) and bool(part.isnan().all())
    assert bool((mask == 0xEE).all()) and c1() and c2() and c3() and c4()
    ws = K.Workspace(torch.device(DEV))
    v = torch.ones(4104, device=DEV)
    for shape in ((3, 12), (1, 3, 1, 4), (2, 2, 1, 12)):
        y = x[:math.prod(shape)].view(shape)
        with pytest.raises(ValueError, match=str(tuple(shape)).replace("(", r"\(").replace(")", r"\)")):
            K.bn_apply(y, v, v, torch.empty_like(y))
    for shape in ((1, 3, 1, 12), (1, 1, 1, 2056), (1, 2, 1, 4104), (0, 1, 1, 64)):
        y = x[:math.prod(shape)].view(shape)
        with pytest.raises(ValueError, match=str(tuple(shape)).replace("(", r"\(").replace(")", r"\)")):
            K.bn_bwd(ws, y, v, v, v, v, v, v, v, torch.empty_like(y), g1=y)
    y = x[:36].view(1, 3, 1, 12)
    with pytest.raises(ValueError, match=r"\(1, 3, 1, 12\)"):
        K.bn_bwd_finish(ws, part, 1, 2, y, v, v, v, v, v, y, torch.empty_like(y))
