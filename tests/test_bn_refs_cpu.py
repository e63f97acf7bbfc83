"""The references of tests/bn_refs.py verified on the CPU: the case builders' exactness premises for
every case tests/test_bn_kernels_gpu.py uses, the composition reduce -> finalize -> apply against
torch autograd in float64, and the forward-statistics reference against torch's mean / var."""
import itertools

import pytest
import torch

import bn_refs as B

F64 = torch.float64


# ------------------------------------------------------------------ premises of the exact cases
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_apply_cases_are_exact(mode):
    """Building a case runs its assertions (f32 == f64, pre == 0 share, ties, representability)."""
    for rows, C in B.APPLY_SHAPES + B.STREAM_SHAPES + [(B.BIG_BLOCK, B.BIG_C)]:
        d = B.bn_case(rows, C, mode)
        assert d["pre"].shape == (rows, C)
        if rows * C >= 64:
            assert float((d["pre"] == 0).double().mean()) > 0.05


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_reduce_cases_are_exact(mode):
    for C, rows, form in itertools.product(B.REDUCE_C, B.REDUCE_ROWS, B.GRAD_FORMS):
        d = B.reduce_case(rows, C, mode, form)
        for G in B.reduce_G(rows):
            p = B.partials_ref(d["dz"], d["y"], d["y2"], G)
            assert p.shape == (G, 3 if mode == 2 else 2, C)
            if d["exact"]:      # the blocks' sums add up to the one-block sums, exactly
                assert torch.equal(p.sum(0), B.partials_ref(d["dz"], d["y"], d["y2"], 1)[0])
            own = [r1 > r0 for r0, r1 in B.block_rows(rows, G)]
            assert all(bool((p[b] == 0).all()) for b in range(G) if not own[b])


def test_big_case_takes_a_second_trip_with_other_channels():
    """The large apply case: the one-chunk kernel's grid is capped at 8192 blocks, its stride is no
    multiple of C/8, and exactly the chunks past the stride take a second trip."""
    n8 = B.BIG_ROWS * B.BIG_C // 8
    stride = 8192 * 256
    assert stride < n8 <= stride + 256 and stride % (B.BIG_C // 8) != 0
    assert (n8 - 1) % (B.BIG_C // 8) != 0          # the second trip's chunk: other channels
    d = B.bn_case(B.BIG_BLOCK, B.BIG_C, 0)
    c0, c1 = 0, ((n8 - 1) % 3) * 8
    assert not torch.equal(d["sc"][c0:c0 + 8], d["sc"][c1:c1 + 8]) or \
        not torch.equal(d["sh"][c0:c0 + 8], d["sh"][c1:c1 + 8])


def test_stats_cases_are_exact():
    for T, C, nq in itertools.product(B.STATS_T, B.STATS_C, (2, 3)):
        for dyadic in (False, True):
            d = B.bwd_stats_case(T, C, nq, dyadic)
            assert torch.equal(d["tot"], d["part"].flip(0).sum(0))
        # dyadic coefficients and a power-of-two count: the float64 finalize is exact, so a
        # differently associated evaluation gives the same bits
        d = B.bwd_stats_case(T, C, nq, True)
        for b in range(nq - 1):
            p = d[b]
            r = B.bwd_finalize_ref(d["tot"][0], d["tot"][1 + b], p["gamma"], p["mean"], p["invstd"], 1024.0, 0.5)
            a = p["gamma"] * p["invstd"]
            sdzx = d["tot"][1 + b] * p["invstd"] - p["mean"] * p["invstd"] * d["tot"][0]
            assert torch.equal(r["dgamma"], 0.5 * sdzx)
            assert torch.equal(r["k2"], -(a * p["invstd"] / 1024.0) * sdzx)
            assert torch.equal(r["k3"], -(r["k2"] * p["mean"]) - (a / 1024.0) * d["tot"][0])
    for (T, bm, M), C in itertools.product(B.FWD_CASES, B.FWD_C):
        d = B.fwd_stats_case(T, C, bm, M)
        assert torch.equal(d["tot"], B.fwd_totals_ref(d["part"].float(), bm, M))
        assert bool((d["tot"][1] * M >= d["tot"][0] ** 2).all())


def test_stream_loop_model():
    """Every multi-chunk streaming configuration of the GPU file makes the whole-batch loop iterate
    and leaves chunks to the remainder loop, at both streaming shapes."""
    for cfg, (rows, C) in itertools.product(B.STREAM_CFGS, B.STREAM_SHAPES):
        n8 = rows * C // 8
        if B.stream_chunks(cfg) > 1 and cfg[0] != 0:
            assert B.stream_grid(cfg, n8, C) > 0, (cfg, rows, C)
            batch, rem = B.stream_loops(cfg, n8, C)
            assert batch > 0 and rem > 0, (cfg, rows, C, batch, rem)


# ------------------------------------------------------------------ composition == autograd
def _bn(y, gamma, beta, eps):
    mean, var = y.mean(0), y.var(0, unbiased=False)
    return (y - mean) / torch.sqrt(var + eps) * gamma + beta, mean, 1 / torch.sqrt(var + eps)


@pytest.mark.parametrize("form", ["g1", "g1+g2", "gp"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_composition_matches_autograd(mode, form):
    """reduce -> finalize -> apply (bn_refs) equals torch autograd of relu(bn(y) [+ res | + bn2(y2)])
    (mode 3: of bn(y), no mask) on generic float64 data -- with an average pool in front for the
    ``gp`` form and a sum of two upstream gradients for ``g2`` -- including the gamma / beta
    gradients with gscale and accumulate, a count of rows, and dres = dz."""
    g = torch.Generator().manual_seed(10 * mode + len(form))
    N, HW, C, eps, G = 3, 7, 16, 1e-5, 4
    rows = N * HW
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    y, r2 = (rnd(rows, C) + 0.3).requires_grad_(), (rnd(rows, C) - 0.2).requires_grad_()
    ga, be, ga2, be2 = ((rnd(C).abs() + 0.5).requires_grad_() for _ in range(4))
    z, mean, inv = _bn(y, ga, be, eps)
    if mode == 1:
        z = z + r2
    elif mode == 2:
        z2, mean2, inv2 = _bn(r2, ga2, be2, eps)
        z = z + z2
    out = z if mode == 3 else torch.relu(z)
    g1, g2, gp = rnd(rows, C), rnd(rows, C), rnd(N, C)
    if form == "gp":
        out.view(N, HW, C).mean(1).backward(gp)
    else:
        out.backward(g1 + g2 if form == "g1+g2" else g1)
    # the kernels' pipeline
    with torch.no_grad():
        sc, sh = ga * inv, be - mean * ga * inv
        sc2, sh2 = (ga2 * inv2, be2 - mean2 * ga2 * inv2) if mode == 2 else (None, None)
        pre = B.apply_pre(y, sc, sh, 0 if mode == 3 else mode, r2, sc2, sh2)
        dA = B.grad_ref(rows, g1, g2 if form == "g1+g2" else None, gp if form == "gp" else None, HW)
        dz = B.dz_ref(dA, mode, pre)
        tot = B.partials_ref(dz, y, r2 if mode == 2 else None, G).sum(0)
        old = rnd(2, C)
        branches = [(y, ga, be, mean, inv, 1)] + ([(r2, ga2, be2, mean2, inv2, 2)] if mode == 2 else [])
        for ys, gam, bet, mu, is_, qy in branches:
            r = B.bwd_finalize_ref(tot[0], tot[qy], gam, mu, is_, float(rows), 0.5)
            dy = B.bwd_apply_ref(dz, ys, r["k1"], r["k2"], r["k3"])
            torch.testing.assert_close(dy, ys.grad, rtol=1e-10, atol=1e-10)
            torch.testing.assert_close(r["dgamma"] + old[0], 0.5 * gam.grad + old[0], rtol=1e-10, atol=1e-10)
            torch.testing.assert_close(r["dbeta"] + old[1], 0.5 * bet.grad + old[1], rtol=1e-10, atol=1e-10)
            assert float(r["k3_extra"].max()) < 1e-12
        if mode == 1:
            torch.testing.assert_close(dz, r2.grad, rtol=1e-10, atol=1e-10)


def test_sync_count_halves_the_coefficients():
    """count = 2 * rows (two identical SyncBatchNorm ranks summing their partials): the doubled
    totals over the doubled count give the single-rank coefficients."""
    d = B.bwd_stats_case(5, 12, 2, False)
    p = d[0]
    one = B.bwd_finalize_ref(d["tot"][0], d["tot"][1], p["gamma"], p["mean"], p["invstd"], 64.0, 1.0)
    two = B.bwd_finalize_ref(2 * d["tot"][0], 2 * d["tot"][1], p["gamma"], p["mean"], p["invstd"], 128.0, 0.5)
    for k in ("dgamma", "dbeta", "k1", "k2", "k3"):
        torch.testing.assert_close(one[k], two[k], rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------ forward statistics
@pytest.mark.parametrize("T,bm,M", [(5, 16, 5 * 16 - 3), (1, 8, 1), (3, 4, 12)])
def test_forward_statistics_match_torch(T, bm, M):
    """Shifted per-tile partials of generic rows -> totals -> mean / var equal torch's mean and
    var(unbiased=False) of those rows; invstd and the unbiased variance follow."""
    g = torch.Generator().manual_seed(T * 100 + M)
    C, eps = 12, 1e-5
    y = torch.randn(M, C, generator=g, dtype=F64) * 2 + 5
    part = torch.zeros(T, 3, C, dtype=F64)
    for t in range(T):
        rows = y[t * bm:(t + 1) * bm]
        s = rows[0]
        part[t] = torch.stack([(rows - s).sum(0), ((rows - s) ** 2).sum(0), s])
    tot = B.fwd_totals_ref(part, bm, M)
    torch.testing.assert_close(tot, torch.stack([y.sum(0), (y * y).sum(0)]), rtol=1e-12, atol=1e-10)
    r = B.fwd_finalize_ref(tot, float(M), eps)
    torch.testing.assert_close(r["mean"], y.mean(0), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(r["var"], y.var(0, unbiased=False), rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(r["invstd"], 1 / torch.sqrt(y.var(0, unbiased=False) + B.f32c(eps)),
                               rtol=1e-10, atol=1e-10)
    if M > 1:
        torch.testing.assert_close(r["unb"], y.var(0, unbiased=True), rtol=1e-10, atol=1e-10)
    else:
        assert torch.equal(r["unb"], r["var"])


def test_clamp_and_slab_reference():
    tot = torch.tensor([[10.0, -6.0], [24.0, 8.0]], dtype=F64)     # E[y^2] < mean^2 at count 4
    r = B.fwd_finalize_ref(tot, 4.0, 1e-5)
    assert torch.equal(r["var"], torch.zeros(2, dtype=F64))
    assert torch.equal(r["invstd"].float(), torch.full((2,), 1 / B.f32c(1e-5) ** 0.5).float())
    x = torch.arange(5 * 3, dtype=F64).view(5, 3)
    out, s = B.slab_ref(x, 5, 2)
    assert s == 2 and torch.equal(out, torch.stack([x[:3].sum(0), x[3:].sum(0)]))
    assert B.slab_ref(x, 5, 96)[1] == 5 and B.slab_ref(x, 5, 1)[1] == 1
