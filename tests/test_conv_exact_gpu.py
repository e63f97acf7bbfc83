"""The convolution kernels (csrc/conv_gemm.hip, csrc/wgrad_tap.hip, csrc/stem.hip) pinned element
by element on exact integer data.

Operands are small integers (tests/conv_refs.py), so every MFMA accumulation is exact in f32
whatever its order, tile, split-K depth or pipeline: each stored value must equal the float64
CPU reference rounded once to the storage dtype, bit for bit (``torch.equal``), statistics and
partial sums must equal the integer sums (``==`` in float64), and the poison bands around every
output must be untouched. The geometries are non-square, ragged in M and N, and small; the
premises of the exactness argument are proven per case on the CPU (tests/test_conv_refs_cpu.py).

Each test loops the compiled tiles its geometry is dispatched (``conv_refs.accepts``) and collects
mismatches in a ``bad`` list; a launch the predicate accepts and the library rejects (-1 / -5) is
a mismatch, any other launch error ends the test at once."""
import math

import pytest
import torch

import conv_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
DT16 = sorted(R.DTYPES16)


def _k():
    from pytorch_distributed_amd.ops import ext
    ext.load(required=True)
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _geom(K, c, cout=None):
    return K.ConvGeom(c.Nb, c.H, c.W, c.Cin, cout or c.rows, c.R, c.S, c.stride, c.pad, c.ho, c.wo)


def _in(t64, dtype):
    """Device operand behind NaN bands."""
    fill = R.round_to(t64, dtype) if t64.dtype == F64 else t64
    return R.guarded(t64.shape, dtype, fill=fill, device=DEV, band_byte=0xFF)[0]


def _out(shape, dtype, fill=None):
    """Device output: NaN inside, sentinel bands; (view, band check)."""
    return R.guarded(shape, dtype, fill=fill, device=DEV)


def _f32(t64):
    return t64.to(torch.float32).to(DEV)


def _run(bad, tag, fn) -> bool:
    try:
        fn()
        return True
    except RuntimeError as e:
        if str(e).rstrip().endswith(("error -1", "error -5")):
            bad.append((tag, "rejected by the dispatch", str(e)))
            return False
        raise


def _cmp(bad, tag, got, ref):
    """Bit-for-bit: ``got`` (device) against ``ref`` (CPU, same dtype)."""
    g = got.detach().cpu()
    assert g.dtype == ref.dtype and g.shape == ref.shape, (tag, g.dtype, ref.dtype, g.shape, ref.shape)
    if not torch.equal(g, ref):
        ne = ~(g.to(F64) == ref.to(F64))
        idx = ne.nonzero()[0].tolist()
        bad.append((tag, f"{int(ne.sum())} of {ne.numel()} differ, first at {idx}: "
                         f"{g[tuple(idx)].item()} != {ref[tuple(idx)].item()}"))


def _guards(bad, tag, *checks):
    for i, chk in enumerate(checks):
        if not chk():
            bad.append((tag, f"guard band {i} overwritten"))


class _GuardedWorkspace:
    """Workspace whose every buffer is a fresh guarded one (NaN inside): split-K slabs included."""

    def __new__(cls, K):
        class W(K.Workspace):
            def __init__(self):
                super().__init__(torch.device(DEV))
                self.checks = []

            def get(self, name, numel, dtype=torch.float32):
                v, chk = R.guarded((max(numel, 1),), dtype, device=DEV)
                self.checks.append(chk)
                self._retired.append(v)
                return v[:numel]
        return W()


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", sorted(R.CASES))
def test_fwd_exact(cid, dt):
    """conv_fwd on every accepted tile: plain, ReLU, operand prologue -- each with statistics --
    the packed stem weights (I), and the fc head's bias + f32 output at a row pitch above Cout (G,
    whose 100 output channels only the f32 store takes)."""
    K = _k()
    c, dtype = R.CASES[cid], R.DTYPES16[dt]
    g = _geom(K, c, c.Cout)
    x, w, _ = R.case_data(cid)
    w2 = w.reshape(c.rows, -1) if c.kpad is None else R.pack_stem_rows(w, c.kpad)
    wd = _in(w2, dtype)
    V = R.fwd_variants(cid, dtype)
    xd = _in(x.reshape(c.Nb, -1) if cid == "G" else x, dtype)
    bad, ran = [], 0
    for t in R.PASS_TILES["fwd"]:
        if not R.accepts("fwd", t, c):
            continue
        ran += 1
        if cid == "G":
            bias = R.ints((c.Cout,), 3, 5)
            buf, chk = _out((c.Nb, 104), torch.float32)
            out = buf[:, :c.Cout]
            if _run(bad, (t, "bias"), lambda: K.conv_fwd(xd, wd, g, out, bias=_f32(bias), tile=t)):
                ref = (R.case_refs(cid)[0].reshape(c.Nb, -1)[:, :c.Cout] + bias).to(torch.float32)
                _cmp(bad, (t, "bias"), out, ref)
                if not torch.isnan(buf[:, c.Cout:]).all().item():
                    bad.append((t, "bias", "wrote between the rows"))
                _guards(bad, (t, "bias"), chk)
            continue
        for name, v in V.items():
            if name == "pro" and t[0] > 1000:     # the LDS-DMA tiles take no prologue
                continue
            kbm = K._ktile(t[0], t[1], K.dt_of(dtype), name == "pro" or c.Cin < 64)[0]
            T = math.ceil(c.M / K.tile_rows(kbm))
            y, ychk = _out((c.Nb, c.Ho, c.Wo, c.Cout), dtype)
            st, schk = _out((T * 3 * c.Cout,), torch.float32)
            kw = dict(relu=True) if name == "relu" else \
                dict(pro=(_f32(v["sc"]), _f32(v["sh"]))) if name == "pro" else {}
            if not _run(bad, (t, name), lambda: K.conv_fwd(xd, wd, g, y, stats=st, tile=t, **kw)):
                continue
            ref = R.round_to(v["y"][..., :c.Cout], dtype)
            _cmp(bad, (t, name), y, ref)
            tot = K.stats_totals(st, c.M, c.Cout, kbm).cpu()
            if not torch.equal(tot, R.stats_ref(ref)):
                bad.append((t, name, "statistics", (tot - R.stats_ref(ref)).abs().max().item()))
            _guards(bad, (t, name), ychk, schk)
    assert ran, "no forward tile accepted this geometry"
    assert not bad, bad


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", [i for i in sorted(R.CASES) if R.tail_ok(R.CASES[i])])
def test_fwd_tail_exact(cid, dt):
    """FWD_TAIL modes 1 and 2: the conv output, its statistics, the written activation a and (mode
    1) its ReLU bitmask, against the CPU model of relu(bn(y3) + r)."""
    K = _k()
    c, dtype = R.CASES[cid], R.DTYPES16[dt]
    g = _geom(K, c, c.Cout)
    assert K.tail_fuse_ok(g, dtype)
    wd = _in(R.case_data(cid)[1].reshape(c.rows, -1), dtype)
    T = math.ceil(c.M / 128)
    bad = []
    for mode, v in R.tail_variants(cid, dtype).items():
        y3, res = _in(v["y3"], dtype), _in(v["res"], dtype)
        a, achk = _out(v["y3"].shape, dtype)
        m, mchk = _out((v["y3"].numel() // 8,), torch.uint8, fill=0x5A)
        y, ychk = _out((c.Nb, c.Ho, c.Wo, c.Cout), dtype)
        st, schk = _out((T * 3 * c.Cout,), torch.float32)
        tail = K.TailIn(res, a, mask=m if mode == 1 else None,
                        sc2=_f32(v["sc2"]) if mode == 2 else None, sh2=_f32(v["sh2"]) if mode == 2 else None)
        K.conv_fwd(y3, wd, g, y, stats=st, pro=(_f32(v["sc"]), _f32(v["sh"])), tail=tail)
        ref = R.round_to(v["y"], dtype)
        _cmp(bad, (mode, "y"), y, ref)
        _cmp(bad, (mode, "a"), a, R.round_to(v["a"], dtype))
        if mode == 1:
            _cmp(bad, (mode, "mask"), m, v["mask"])
        tot = K.stats_totals(st, c.M, c.Cout, 128).cpu()
        if not torch.equal(tot, R.stats_ref(ref)):
            bad.append((mode, "statistics"))
        _guards(bad, mode, achk, mchk, ychk, schk)
    assert not bad, bad


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", ["H1", "H2"])
def test_stem_fwd_exact(cid, dt, monkeypatch):
    """csrc/stem.hip with its per-output-row statistics, the same launch through conv_fwd's own
    dispatch, and the generic fallback of that dispatch with ``_STEM_FWD`` off."""
    K = _k()
    c, dtype = R.CASES[cid], R.DTYPES16[dt]
    g = _geom(K, c)
    assert K.stem_fwd_ok(g, dtype), "the stem kernel must run for this geometry"
    x, w, _ = R.case_data(cid)
    xd, wd = _in(x, dtype), _in(w.reshape(c.rows, -1), dtype)
    ref = R.round_to(R.case_refs(cid)[0], dtype)
    rows = K.stem_stats_rows(g)
    assert rows == c.Wo and c.M % rows == 0
    bad = []
    y, ychk = _out(ref.shape, dtype)
    st, schk = _out((c.M // rows * 3 * 64,), torch.float32)
    K.stem_fwd(xd, wd, g, y, st)
    _cmp(bad, "stem", y, ref)
    tot = K.stats_totals(st, c.M, 64, rows).cpu()
    if not torch.equal(tot, R.stats_ref(ref)):
        bad.append(("stem", "statistics"))
    _guards(bad, "stem", ychk, schk)
    for name, on in (("dispatch", True), ("generic", False)):
        monkeypatch.setattr(K, "_STEM_FWD", on)
        y, ychk = _out(ref.shape, dtype)
        K.conv_fwd(xd, wd, g, y)
        _cmp(bad, name, y, ref)
        _guards(bad, name, ychk)
    assert not bad, bad


# ------------------------------------------------------------------ data gradient
def _dgrad_case(K, cid, dtype, tiles, bad):
    c = R.CASES[cid]
    g = _geom(K, c)
    _, w, dy = R.case_data(cid)
    dyd, wd = _in(dy, dtype), _in(w, dtype)
    ref = R.round_to(R.case_refs(cid)[1], dtype)
    o = R.epi_operands(cid)
    od = {k: (_in(v, dtype) if v.dim() == 4 else _f32(v)) for k, v in o.items()}
    V = R.dgrad_variants(cid, dtype)
    maskd = _in(V[(3, False)]["mask"], torch.uint8)
    ran = 0
    for t in tiles:
        ran += 1
        dx, chk = _out(ref.shape, dtype)
        if not _run(bad, (t, "plain"), lambda: K.conv_dgrad(dyd, wd, g, dx, tile=t)):
            continue
        _cmp(bad, (t, "plain"), dx, ref)
        _guards(bad, (t, "plain"), chk)
        G = K.dgrad_slabs(g, c.Nb, tile=t, dtype=dtype)
        for (mode, wg), v in V.items():
            nq = 3 if mode == 2 else 2
            part, pchk = _out((G * nq * c.Cin,), torch.float32)
            dz, zchk = _out(ref.shape, dtype)
            y2 = od["y2"] if mode in (1, 2) else None
            epi = K.ext.BnEpi(mode, nq, K.ptr(od["y"]), K.ptr(od["sc"]), K.ptr(od["sh"]), K.ptr(y2),
                              K.ptr(od["sc2"] if mode == 2 else None), K.ptr(od["sh2"] if mode == 2 else None),
                              K.ptr(od["g2"] if wg else None), K.ptr(part), K.ptr(maskd if mode == 3 else None))
            tag = (t, f"epi{mode}" + ("+g2" if wg else ""))
            if not _run(bad, tag, lambda: K.conv_dgrad(dyd, wd, g, dz, tile=t, epi=epi)):
                continue
            _cmp(bad, tag, dz, R.round_to(v["dz"], dtype))
            tot = part.view(G, nq, c.Cin).double().sum(0).cpu()
            if not torch.equal(tot, v["tot"]):
                bad.append((tag, "partial sums", (tot - v["tot"]).abs().max().item()))
            _guards(bad, tag, zchk, pchk)
    return ran


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", [i for i in sorted(R.CASES) if "dgrad" in R.CASES[i].passes])
def test_dgrad_exact(cid, dt):
    """conv_dgrad on every accepted tile: plain dx (classes without a tap write exact zeros) and
    the fused BatchNorm-backward epilogue, modes 0-3 with and without g2: dz and the partial sums
    over the slabs; the mode-3 mask comes from the CPU reference."""
    K = _k()
    bad = []
    tiles = [t for t in R.PASS_TILES["dgrad"] if R.accepts("dgrad", t, R.CASES[cid])]
    assert _dgrad_case(K, cid, R.DTYPES16[dt], tiles, bad), "no dgrad tile accepted this geometry"
    assert not bad, bad


# ------------------------------------------------------------------ weight gradient
def _wgrad_direct(K, dyd, xd, g, grad, ws, tile, k_chunk):
    """The launch of conv_wgrad at an explicit split depth (conv_wgrad caps splits at K / 256)."""
    import ctypes as C
    Nb = dyd.shape[0]
    Kr = Nb * g.Ho * g.Wo
    splits = math.ceil(Kr / k_chunk)
    M, N = g.Cout, g.R * g.S * g.Cin
    slab = ws.get("wgrad_slab", splits * M * N)
    d = g.desc(Nb)
    st = K.stream(dyd.device)
    kbm, kbn = K._ktile(tile[0], tile[1], K._kdt(dyd))
    K.check(K.ext.lib().pda_conv_wgrad(C.byref(d), K.ptr(dyd), K.ptr(xd), K.ptr(slab), splits, k_chunk,
                                       None, None, K._kdt(dyd), kbm, kbn, st), "conv_wgrad")
    K.check(K.ext.lib().pda_wgrad_reduce(K.ptr(slab), K.ptr(grad), splits, M, N, int(math.log2(g.Cin)),
                                         g.Cin, N, 1.0, 0, None, None, None, st), "wgrad_reduce")


def _wgrad_case(K, cid, dtype, tiles, bna_tiles, bad, depths=(1, 64, 4096)):
    c = R.CASES[cid]
    g = _geom(K, c)
    x, _, dy = R.case_data(cid)
    xd, dyd = _in(x, dtype), _in(dy, dtype)
    V = R.wgrad_variants(cid, dtype)
    cr = c.cin_real or c.Cin
    shape = (c.rows, c.R, c.S, cr)
    ref = V["plain"]["dw"][..., :cr].contiguous().to(torch.float32)
    ws = _GuardedWorkspace(K)

    def one(tag, fn, want):
        dw, chk = _out(shape, torch.float32)
        if _run(bad, tag, lambda: fn(dw.view(-1))):
            _cmp(bad, tag, dw, want)
            _guards(bad, tag, chk)

    ran = 0
    for t in tiles:
        ran += 1
        for tb in depths:
            one((t, f"tb{tb}"), lambda gr: K.conv_wgrad(dyd, xd, g, gr, ws, tile=t, target_blocks=tb,
                                                        cin_real=c.cin_real), ref)
        if c.cin_real is None:     # one split per 64 rows of K: the deepest split-K
            one((t, "k64"), lambda gr: _wgrad_direct(K, dyd, xd, g, gr, ws, t, 64), ref)
        if "pro" in V and t[0] < 1000:
            v = V["pro"]
            one((t, "pro"), lambda gr: K.conv_wgrad(dyd, xd, g, gr, ws, tile=t, target_blocks=64,
                                                    pro=(_f32(v["sc"]), _f32(v["sh"]))),
                v["dw"].to(torch.float32))
    if tiles and dtype != torch.float32:
        t = tiles[0]
        pre = R.ints(shape, 9, 61)
        dw, chk = _out(shape, torch.float32, fill=pre)
        if _run(bad, "accumulate", lambda: K.conv_wgrad(dyd, xd, g, dw.view(-1), ws, tile=t, scale=0.25,
                                                        accumulate=True, cin_real=c.cin_real)):
            _cmp(bad, "accumulate", dw, (pre + 0.25 * ref.to(F64)).to(torch.float32))
            _guards(bad, "accumulate", chk)
        # two queued reductions, one launch
        ws.reduce_batch = K.ReduceBatch(ws)
        outs = [_out(shape, torch.float32) for _ in tiles[:2]]
        for (dw, _), tt in zip(outs, tiles[:2]):
            K.conv_wgrad(dyd, xd, g, dw.view(-1), ws, tile=tt, target_blocks=64, cin_real=c.cin_real)
        ws.reduce_batch.flush()
        ws.reduce_batch = None
        for (dw, chk), tt in zip(outs, tiles[:2]):
            _cmp(bad, (tt, "batch"), dw, ref)
            _guards(bad, (tt, "batch"), chk)
    if bna_tiles:
        v = V["bna"]
        yd = _in(v["y"], dtype)
        kk = _f32(torch.cat([v["k1"], v["k2"], v["k3"]]))
        for t in bna_tiles:
            for tb in (1, 4096):
                one((t, f"bna/tb{tb}"), lambda gr: K.conv_wgrad(dyd, xd, g, gr, ws, tile=t, target_blocks=tb,
                                                               bna=(yd, kk)), v["dw"].to(torch.float32))
    _guards(bad, "workspace", *ws.checks)
    return ran


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", [i for i in sorted(R.CASES) if "wgrad" in R.CASES[i].passes])
def test_wgrad_exact(cid, dt):
    """conv_wgrad on every accepted tile at split-K depths from 1 to K / 64, with the operand
    prologue, with the BN-backward operand (the WGRAD_BNA tiles), scaled accumulation onto an
    integer prefill, ``cin_real`` (I) and through a ReduceBatch: dW bit-equal as f32 for every
    (o, r, s, c), every slab's guard bands intact."""
    K = _k()
    c = R.CASES[cid]
    bad = []
    tiles = [t for t in R.PASS_TILES["wgrad"] if R.accepts("wgrad", t, c)]
    bna = [t for t in R.BNA_TILES if R.accepts_bna(t, c)] if c.cin_real is None else []
    assert _wgrad_case(K, cid, R.DTYPES16[dt], tiles, bna, bad), "no wgrad tile accepted this geometry"
    assert not bad, bad


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", ["A", "B"])
def test_wgrad_tap_exact(cid, dt):
    """csrc/wgrad_tap.hip called directly (it takes any W <= 59) at 1, 7 and 96 blocks, with and
    without the operand prologue."""
    K = _k()
    c, dtype = R.CASES[cid], R.DTYPES16[dt]
    x, _, dy = R.case_data(cid)
    xd, dyd = _in(x, dtype), _in(dy, dtype)
    g = _geom(K, c)
    V = R.wgrad_variants(cid, dtype)
    N = 9 * c.Cin
    L, st = K.ext.lib(), K.stream(torch.device(DEV))
    bad = []
    for name in ("plain", "pro"):
        v = V[name]
        sc, sh = (_f32(v["sc"]), _f32(v["sh"])) if name == "pro" else (None, None)
        for blocks in (1, 7, 96):
            kb, splits = K.wgrad_tap_plan(g, c.Nb, blocks)
            slab, schk = _out((splits * c.Cout * N,), torch.float32)
            dw, chk = _out((c.Cout, 3, 3, c.Cin), torch.float32)
            K.check(L.pda_wgrad_tap(K.ptr(dyd), K.ptr(xd), K.ptr(slab), K.ptr(sc), K.ptr(sh), c.Nb, c.H, c.W,
                                    c.Cin, c.Cout, kb, splits, K.dt_of(dtype), st), "wgrad_tap")
            K.check(L.pda_wgrad_reduce(K.ptr(slab), K.ptr(dw), splits, c.Cout, N, int(math.log2(c.Cin)),
                                       c.Cin, N, 1.0, 0, None, None, None, st), "wgrad_reduce")
            _cmp(bad, (name, blocks, splits), dw, v["dw"].to(torch.float32))
            _guards(bad, (name, blocks), chk, schk)
    assert not bad, bad


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("cid", ["H1", "H2"])
def test_wgrad_stem_tap_exact(cid, dt):
    """csrc/wgrad_tap.hip wgrad_stem_tap_kernel (dY = k1*dz + k2*y + k3 formed in LDS) at several
    block counts."""
    K = _k()
    c, dtype = R.CASES[cid], R.DTYPES16[dt]
    g = _geom(K, c)
    assert K.stem_wgrad_tap_ok(g, dtype, force=True)
    x, _, dy = R.case_data(cid)
    v = R.wgrad_variants(cid, dtype)["bna"]
    xd, dzd, yd = _in(x, dtype), _in(dy, dtype), _in(v["y"], dtype)
    kk = _f32(torch.cat([v["k1"], v["k2"], v["k3"]]))
    ws = _GuardedWorkspace(K)
    bad = []
    for blocks in (1, 5, 512):
        dw, chk = _out((64, 4, 4, 16), torch.float32)
        K.conv_wgrad_stem_tap(dzd, yd, kk, xd, g, dw.view(-1), ws, blocks=blocks)
        _cmp(bad, blocks, dw, v["dw"].to(torch.float32))
        _guards(bad, blocks, chk)
    _guards(bad, "workspace", *ws.checks)
    assert not bad, bad


# ------------------------------------------------------------------ the f32 kernels
@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("cid", [i for i in sorted(R.CASES) if R.CASES[i].f32])
def test_f32_kernels_exact(cid, mode, monkeypatch):
    """The exact-f32 (MFMA 16x16x4 f32) and split-f32 (bf16 hi/lo MFMA, (64, 64) included) kernels
    on f32 tensors of the same integers: forward with statistics, ReLU and prologue, the data
    gradient with its fused epilogue, the weight gradient."""
    K = _k()
    monkeypatch.setattr(K, "_F32_CONV", mode)
    c, dtype = R.CASES[cid], torch.float32
    g = _geom(K, c)
    x, w, _ = R.case_data(cid)
    xd, wd = _in(x, dtype), _in(w.reshape(c.rows, -1), dtype)
    kdt = K._kdt(xd)
    assert kdt == (3 if mode == "split" else 0)
    seen, tiles = set(), []
    for t in R.TILES:       # (the split kernels run single-stage: several codes share a kernel)
        kt = K._ktile(t[0], t[1], kdt)
        if kt not in seen:
            seen.add(kt)
            tiles.append(t)
    assert (-64, 64) in seen or mode == "exact"
    bad = []
    for t in tiles:
        kbm = K._ktile(t[0], t[1], kdt)[0]
        T = math.ceil(c.M / K.tile_rows(kbm))
        for name, v in R.fwd_variants(cid, dtype).items():
            y, ychk = _out((c.Nb, c.Ho, c.Wo, c.Cout), dtype)
            st, schk = _out((T * 3 * c.Cout,), torch.float32)
            kw = dict(relu=True) if name == "relu" else \
                dict(pro=(_f32(v["sc"]), _f32(v["sh"]))) if name == "pro" else {}
            if not _run(bad, (t, name), lambda: K.conv_fwd(xd, wd, g, y, stats=st, tile=t, **kw)):
                continue
            ref = R.round_to(v["y"], dtype)
            _cmp(bad, (t, name), y, ref)
            if not torch.equal(K.stats_totals(st, c.M, c.Cout, kbm).cpu(), R.stats_ref(ref)):
                bad.append((t, name, "statistics"))
            _guards(bad, (t, name), ychk, schk)
    _dgrad_case(K, cid, dtype, tiles, bad)
    _wgrad_case(K, cid, dtype, tiles, [], bad, depths=(1, 4096))
    assert not bad, bad


# ------------------------------------------------------------------ no silent gaps
def test_every_compiled_tile_ran_somewhere():
    """Host-only: the tile lists are those of tests/test_conv_shapes_gpu.py and native_ops, every
    compiled (pass, tile) is dispatched for at least one geometry (both 16-bit dtypes run all of
    them), and every geometry runs at least one tile of each of its passes."""
    import test_conv_shapes_gpu as S
    from pytorch_distributed_amd.ops import native_ops as K
    assert (R.TILES, R.DMA_TILES, R.HALO_TILES) == (S.TILES, S.DMA_TILES, S.HALO_TILES)
    assert R.PASS_TILES["wgrad"] == S.WGRAD_TILES
    assert {(abs(bm), bn) for bm, bn in R.BNA_TILES} == K._BNA_TILES
    assert all(R.tile_rows(bm) == K.tile_rows(bm) for p in R.PASS_TILES.values() for bm, _ in p)
    for pas, tiles in R.PASS_TILES.items():
        for t in tiles:
            assert any(R.accepts(pas, t, c) for c in R.CASES.values()), (pas, t)
    for t in R.BNA_TILES:
        assert any(R.accepts_bna(t, c) and c.cin_real is None for c in R.CASES.values()), t
    for c in R.CASES.values():
        for pas in c.passes:
            assert any(R.accepts(pas, t, c) for t in R.PASS_TILES[pas]), (c.id, pas)
    assert {R.CASES[i].Cout for i in R.CASES if R.tail_ok(R.CASES[i])} >= {64, 128}   # both FWD_TAIL tiles
