"""CPU self-checks of tests/conv_refs.py: the float64 references against naive loops, the models
of the fused pieces against plain torch ops, and the exactness conditions of EVERY case the GPU
file (tests/test_conv_exact_gpu.py) parametrises -- so that "the reference alone stays within the
conditions" is proven on a machine without a GPU."""
import numpy as np
import pytest
import torch

import conv_refs as R

F64 = torch.float64


def _naive(x, w, dy, c):
    """Explicit loops over (n, ho, wo, r, s): y, dx, dw in NHWC / OHWI."""
    x, w, dy = x.numpy(), w.numpy(), dy.numpy()
    y = np.zeros((c.Nb, c.Ho, c.Wo, w.shape[0]))
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    for n in range(c.Nb):
        for ho in range(c.Ho):
            for wo in range(c.Wo):
                for r in range(c.R):
                    for s in range(c.S):
                        h, q = ho * c.stride - c.pad + r, wo * c.stride - c.pad + s
                        if not (0 <= h < c.H and 0 <= q < c.W):
                            continue
                        y[n, ho, wo] += w[:, r, s] @ x[n, h, q]
                        dx[n, h, q] += dy[n, ho, wo] @ w[:, r, s]
                        dw[:, r, s] += np.outer(dy[n, ho, wo], x[n, h, q])
    return torch.from_numpy(y), torch.from_numpy(dx), torch.from_numpy(dw)


TINY = [
    R.Case("s1", 2, 5, 4, 3, 4, 3, 3, 1, 1),
    R.Case("s2", 2, 6, 4, 3, 5, 3, 3, 2, 1),
    R.Case("s2-1x1", 2, 6, 4, 3, 5, 1, 1, 2, 0),
    R.Case("stem-s2d", 2, 4, 6, 2, 3, 4, 4, 1, 2, ho=4, wo=6),
    R.Case("stem-7x7", 1, 10, 6, 8, 4, 7, 7, 2, 3, cin_real=3),
]


@pytest.mark.parametrize("c", TINY, ids=[c.id for c in TINY])
def test_references_match_naive_loops(c):
    x = R.ints((c.Nb, c.H, c.W, c.Cin), 2, 1)
    w = R.ints((c.Cout, c.R, c.S, c.Cin), 1, 2)
    dy = R.ints((c.Nb, c.Ho, c.Wo, c.Cout), 2, 3)
    if c.cin_real:
        x[..., c.cin_real:] = 0
        w[..., c.cin_real:] = 0
    y, dx, dw = _naive(x, w, dy, c)
    assert torch.equal(R.conv_fwd_ref(x, w, c), y)
    rdx, rdw = R.conv_bwd_ref(x, w, dy, c)
    assert torch.equal(rdx, dx) and torch.equal(rdw, dw)
    assert y.abs().max() > 0 and dx.abs().max() > 0 and dw.abs().max() > 0
    if c.stride == 2 and c.R == 1:      # the classes no tap lands on
        assert dx[:, 1::2].abs().max() == 0 and dx[:, :, 1::2].abs().max() == 0


def test_stem_padding_is_two_before_one_behind():
    c = TINY[3]
    assert R._pads(c) == (2, 1, 2, 1)
    assert R._pads(R.CASES["A"]) == (1, 1, 1, 1) and R._pads(R.CASES["C"]) == (1, 0, 1, 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_fused_models_against_torch(dtype):
    C = 16
    x = R.ints((2, 3, 5, C), 2, 4)
    r = R.ints(x.shape, 2, 5)
    sc, sh = R.coeffs(C, 6)
    sc2, sh2 = R.coeffs(C, 7)
    # prologue and tail: torch in float32 on the same values, rounded by torch
    xf, rf = x.float(), r.float()
    a = torch.relu(xf * sc.float() + sh.float()).to(dtype)
    assert torch.equal(R.pro_ref(x, sc, sh, dtype), a.to(F64))
    a1 = torch.relu(xf * sc.float() + sh.float() + rf).to(dtype)
    a2 = torch.relu(xf * sc.float() + sh.float() + (rf * sc2.float() + sh2.float())).to(dtype)
    m1 = R.tail_ref(x, sc, sh, r, dtype)
    m2 = R.tail_ref(x, sc, sh, r, dtype, sc2, sh2)
    assert torch.equal(m1[0], a1.to(F64)) and torch.equal(m2[0], a2.to(F64))
    # bitmask: bit e of byte i/8
    bits = np.unpackbits(m1[1].numpy(), bitorder="little")
    assert np.array_equal(bits.astype(bool), (a1.float().reshape(-1) > 0).numpy())
    # statistics
    st = R.stats_ref(a1)
    assert torch.equal(st[0], a1.to(F64).reshape(-1, C).sum(0))
    assert torch.equal(st[1], (a1.to(F64) ** 2).reshape(-1, C).sum(0))
    # dgrad epilogue, every mode, against torch.where on the same masks
    dA, g2 = R.ints(x.shape, 50, 8), R.ints(x.shape, 2, 9)
    masks = {0: x * sc + sh > 0, 1: x * sc + sh + r > 0, 2: x * sc + sh + r * sc2 + sh2 > 0, 3: a1 > 0}
    for mode in (0, 1, 2, 3):
        for g in (None, g2):
            dz, tot = R.dgrad_epi_ref(dA, mode, x, sc, sh, dtype, y2=r, sc2=sc2, sh2=sh2, g2=g, mask=m1[1])
            want = torch.where(masks[mode], dA + (g if g is not None else 0), torch.zeros_like(dA))
            assert torch.equal(dz, want)
            assert torch.equal(tot[0], want.reshape(-1, C).sum(0))
            assert torch.equal(tot[1], (want * x).reshape(-1, C).sum(0))
            assert tot.shape[0] == (3 if mode == 2 else 2)
            if mode == 2:
                assert torch.equal(tot[2], (want * r).reshape(-1, C).sum(0))
    # BN-backward operand: torch's own fused multiply-adds
    k1, k2, k3 = sc, sc2, sh
    dY = torch.addcmul(torch.addcmul(k3.float(), k2.float(), rf), k1.float(), xf).to(dtype)
    assert torch.equal(R.bna_ref(x, r, k1, k2, k3, dtype), dY.to(F64))


def test_rounding_is_once_and_nearest_even():
    v = torch.tensor([257.0, 259.0, 2049.0, 2051.0, -257.0], dtype=F64)
    assert R.round_to(v, torch.bfloat16).tolist() == [256.0, 260.0, 2048.0, 2048.0, -256.0]
    assert R.round_to(v, torch.float16).tolist() == [257.0, 259.0, 2048.0, 2052.0, -257.0]
    with pytest.raises(AssertionError):
        R.round_to(torch.tensor([1.0 + 2.0 ** -30], dtype=F64), torch.float32)


def test_exact_conditions_fail_loudly():
    ok = torch.tensor([[3.0, -256.0]], dtype=F64)
    R.assert_exact_conditions("ok", stored16=(ok,), acc_abs=(ok.abs(),), stats_of=(ok,))
    with pytest.raises(AssertionError):
        R.assert_exact_conditions("big", stored16=(torch.tensor([257.0], dtype=F64),))
    with pytest.raises(AssertionError):
        R.assert_exact_conditions("frac", stored16=(torch.tensor([0.5], dtype=F64),))
    with pytest.raises(AssertionError):
        R.assert_exact_conditions("acc", acc_abs=(torch.tensor([2.0 ** 24], dtype=F64),))
    with pytest.raises(AssertionError):   # 256 rows of (256 + 256)^2 = 2^26
        R.assert_exact_conditions("stats", stats_of=(torch.full((256, 1), 256.0, dtype=F64),))


def test_guarded_buffer_bands():
    v, check = R.guarded((3, 5), torch.bfloat16)
    assert v.is_contiguous() and v.shape == (3, 5) and torch.isnan(v.float()).all()
    assert v.data_ptr() % 256 == v.untyped_storage().data_ptr() % 256 and R.BAND % 256 == 0
    assert check()
    v.fill_(1.0)
    assert check()
    flat = torch.as_strided(v, (16,), (1,))      # one element past the end
    flat[15] = 2.0
    assert not check()
    v2, check2 = R.guarded((4,), torch.float32, fill=torch.arange(4.0), band_byte=0xFF)
    assert v2.tolist() == [0.0, 1.0, 2.0, 3.0] and check2()
    torch.as_strided(v2, (1,), (1,), v2.storage_offset() - 1).fill_(0.0)   # one element before
    assert not check2()


@pytest.mark.parametrize("dt", sorted(R.DTYPES16))
@pytest.mark.parametrize("cid", sorted(R.CASES))
def test_gpu_cases_stay_within_exact_conditions(cid, dt):
    R.check_case_conditions(cid, R.DTYPES16[dt])


def test_generators_cover_their_ranges():
    for cid, c in R.CASES.items():
        x, w, dy = R.case_data(cid)
        lim = R.act_lim(c)
        assert lim == (1 if c.K > 1200 else 2)
        assert set(x.unique().tolist()) == set(float(v) for v in range(-lim, lim + 1))
        assert set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
        if c.cin_real:
            assert x[..., c.cin_real:].abs().max() == 0 and w[..., c.cin_real:].abs().max() == 0


def test_every_compiled_tile_and_geometry_is_covered():
    """The coverage table of the GPU file, from the host-side dispatch rules alone: every compiled
    (pass, tile) is accepted by at least one geometry, every geometry by at least one tile per
    pass it has (both 16-bit dtypes run every accepted combination)."""
    for pas, tiles in R.PASS_TILES.items():
        for t in tiles:
            assert any(R.accepts(pas, t, c) for c in R.CASES.values()), (pas, t)
    for t in R.BNA_TILES:
        assert any(R.accepts_bna(t, c) for c in R.CASES.values()), t
    for c in R.CASES.values():
        for pas in c.passes:
            assert any(R.accepts(pas, t, c) for t in R.PASS_TILES[pas]), (c.id, pas)
    assert {c.id for c in R.CASES.values() if c.f32} == {"A", "C", "D", "F"}
