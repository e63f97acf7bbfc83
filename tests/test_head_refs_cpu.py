"""The references of tests/test_head_kernels_gpu.py (tests/head_refs.py) against torch on the CPU,
where torch's behaviour is defined -- so a wrong reference fails here, without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import head_refs as R

F64 = torch.float64


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_ulp_out_is_the_dtype_spacing(dtype):
    """ulp_out(x) == distance from x to the next representable value of larger magnitude, for
    normals, subnormals, zero and powers of two."""
    it = torch.int16 if dtype != torch.float32 else torch.int32
    x = torch.tensor([0.0, 1.0, 1.5, 1.9990234375, 2.0, 3.0, 1000.0, 6.1035e-5, 6.0e-5, 5.96e-8,
                      1.0e-6, 0.3333, 1.2e-38, 1.0e-38, 1.0e-40, 255.0], dtype=F64).float().to(dtype)
    nxt = (x.view(it) + 1).view(dtype)
    assert bool(nxt.isfinite().all())
    assert torch.equal(R.ulp_out(x.to(F64), dtype), nxt.to(F64) - x.to(F64))
    # a reference between two representable values gets the spacing of the one below
    mid = (x.to(F64) + nxt.to(F64)) / 2
    assert torch.equal(R.ulp_out(mid, dtype), nxt.to(F64) - x.to(F64))


def test_within_ulp_overflow_and_nan():
    ref = torch.tensor([1.0, 70000.0, -70000.0, 65504.0, 1.0], dtype=F64)
    got = torch.tensor([1.0, float("inf"), float("-inf"), 65504.0, float("nan")]).half()
    ok, _ = R.within_ulp(got, ref, torch.float16)
    assert ok.tolist() == [True, True, True, True, False]
    got = torch.tensor([1.002, 65504.0, float("inf"), float("inf"), 1.0]).half()
    ok, _ = R.within_ulp(got, ref, torch.float16)
    assert ok.tolist() == [False, False, False, False, True]


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 5, 7, 8), (1, 9, 4, 16), (2, 12, 12, 8)])
def test_pool_ref_and_scatter_match_torch_on_tie_free_data(shape):
    N, H, W, C = shape
    g = R._gen(sum(shape))
    y = torch.rand(shape, generator=g, dtype=F64) + 0.5       # positive: relu clips nothing, no ties
    sc = torch.rand(C, generator=g, dtype=F64) + 0.5
    sh = torch.rand(C, generator=g, dtype=F64)
    out, arg = R.pool_ref(y, sc, sh)
    a = (y * sc + sh).permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref, idx = F.max_pool2d(torch.relu(a), 3, 2, 1, return_indices=True)
    assert torch.equal(out, ref.permute(0, 2, 3, 1))
    Ho, Wo = R.pool_dims(H, W)
    assert (Ho, Wo) == tuple(ref.shape[2:])
    yo = torch.arange(Ho)[None, :, None, None]
    xo = torch.arange(Wo)[None, None, :, None]
    flat = (2 * yo - 1 + arg.long() // 3) * W + (2 * xo - 1 + arg.long() % 3)
    assert torch.equal(flat, idx.permute(0, 2, 3, 1))
    dout = torch.randn(N, Ho, Wo, C, generator=g, dtype=F64)
    ref.backward(dout.permute(0, 3, 1, 2))
    assert torch.equal(R.pool_scatter(dout, arg, H, W), a.grad.permute(0, 2, 3, 1))


def test_pool_ref_takes_the_first_maximum():
    y = torch.zeros(1, 4, 4, 8, dtype=F64)                    # everything ties
    _, arg = R.pool_ref(y, torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64))
    # window (0,0): first in-bounds tap is (1,1); (0,1): (1,0); (1,0): (0,1); (1,1): (0,0)
    assert arg[0, :, :, 0].tolist() == [[4, 3], [1, 0]]
    y[0, 1, 1, :] = 1.0
    y[0, 2, 2, :] = 1.0                                       # two equal maxima in window (1,1)
    _, arg = R.pool_ref(y, torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64))
    assert arg[0, 1, 1, 0].item() == 0 and arg[0, 0, 0, 0].item() == 8


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 5, 7, 8), (1, 9, 4, 72), (3, 12, 12, 64)])
def test_pool_case_inputs_are_exact_and_tie(shape):
    """pool_case asserts its f32 / f64 bit-identity itself; here: the data does tie, the hand-made
    argmax bytes are in bounds, and every value fits all three dtypes."""
    c = R.pool_case(*shape)
    N, H, W, C = shape
    for k in ("y", "dout", "dout2", "out"):
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(c[k].float().to(dt).to(F64), c[k])
    R.pool_scatter(c["dout"], c["fake"], H, W)                # asserts bounds
    if N * H * W > 4:
        # ties are present: a last-maximum scan would choose differently somewhere
        r = (c["y"] * c["sc"] + c["sh"]).clamp_min(0)
        pad = torch.full((N, H + 2, W + 2, C), float("-inf"), dtype=F64)
        pad[:, 1:H + 1, 1:W + 1] = r
        Ho, Wo = R.pool_dims(H, W)
        best, arg_last = c["out"], torch.zeros_like(c["arg"])
        for t in range(9):
            cand = pad[:, t // 3:t // 3 + 2 * Ho - 1:2, t % 3:t % 3 + 2 * Wo - 1:2]
            arg_last = torch.where(cand == best, torch.full_like(arg_last, t), arg_last)
        assert not torch.equal(arg_last, c["arg"])


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (3, 7, 7, 512), (2, 5, 10, 2056)])
def test_tail_case_matches_torch(shape):
    c = R.tail_case(*shape)
    a = (c["y"] * c["sc"] + c["sh"]).permute(0, 3, 1, 2)
    s2 = (c["res"] * c["sc2"] + c["sh2"]).permute(0, 3, 1, 2)
    ref1 = F.adaptive_avg_pool2d(torch.relu(a + c["res"].permute(0, 3, 1, 2)), 1).flatten(1)
    ref2 = F.adaptive_avg_pool2d(torch.relu(a + s2), 1).flatten(1)
    torch.testing.assert_close(c[("ref", 1)], ref1, rtol=1e-14, atol=1e-14)
    torch.testing.assert_close(c[("ref", 2)], ref2, rtol=1e-14, atol=1e-14)
    assert not torch.equal(ref1, ref2)
    assert bool((torch.relu(a + s2) == 0).any()) and bool((c[("ref", 2)] > 0).any())


@pytest.mark.parametrize("K", [10, 65, 1000])
def test_xent_ref_matches_torch(K):
    g = R._gen(K)
    x = (torch.randn(5, K, generator=g, dtype=F64) * 30).requires_grad_(True)
    lab = torch.randint(0, K, (5,), generator=g)
    rows, grad = R.xent_ref(x.detach(), lab)
    ce = F.cross_entropy(x, lab, reduction="none")
    ce.sum().backward()
    torch.testing.assert_close(rows, ce.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(grad, x.grad, rtol=1e-13, atol=1e-300)


def test_topk_ref_matches_validate_form_on_tie_free_data():
    g = R._gen(11)
    for B, K in ((1, 5), (5, 65), (257, 1000)):
        # every row a permutation of K distinct values: no ties within a row
        x = torch.stack([torch.randperm(K, generator=g).float() * 0.37 - 3 for _ in range(B)])
        lab = torch.randint(0, K, (B,), generator=g)
        _, preds = x.topk(5, -1, True, True)
        hit = torch.eq(preds, lab.unsqueeze(1))
        assert R.topk_ref(x, lab) == (int(hit[:, :1].sum()), int(hit.sum()))


def test_topk_ref_breaks_ties_towards_the_lower_index():
    x = torch.full((7, 9), 2.0)
    assert R.topk_ref(x, torch.arange(7)) == (1, 5)          # labels 0..6: top-1 only 0, top-5 0..4
    x = torch.tensor([[5.0, 1.0, 5.0, 5.0, 5.0, 5.0, 5.0]])
    assert R.topk_ref(x, torch.tensor([5])) == (0, 1)        # four equal entries before it
    assert R.topk_ref(x, torch.tensor([6])) == (0, 0)        # five


@pytest.mark.parametrize("momentum,wd", [(0.9, 1e-4), (0.0, 1e-4), (0.9, 0.0)])
def test_sgd_ref_matches_torch_sgd(momentum, wd):
    g = R._gen(2)
    p0, g0 = torch.randn(37, generator=g, dtype=F64), torch.randn(37, generator=g, dtype=F64)
    ref = R.sgd_ref(p0, g0, 3, 0.1, momentum, wd, inv_scale=0.25)
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([pr], lr=0.1, momentum=momentum, weight_decay=wd)
    for it in range(3):
        pr.grad = g0 * 0.25
        opt.step()
        torch.testing.assert_close(ref[it][0], pr.detach(), rtol=1e-14, atol=1e-14)
        if momentum:
            torch.testing.assert_close(ref[it][1], opt.state[pr]["momentum_buffer"], rtol=1e-14,
                                       atol=1e-14)


def test_cast_edge_values_cover_the_edges():
    e = R.cast_edge_values()
    h, b = e.to(torch.float16), e.to(torch.bfloat16)
    tiny32 = torch.finfo(torch.float32).tiny
    assert not bool(((e != 0) & (e.abs() < tiny32)).any())                 # no f32 subnormals
    assert bool(e.isnan().any()) and bool(e.isinf().sum() == 2)
    assert bool(((e == 0) & (torch.signbit(e))).any()) and bool(((e == 0) & ~torch.signbit(e)).any())
    # fp16: overflow by rounding, largest finite, subnormals, flush of the half-smallest tie
    assert bool((h.isinf() & e.isfinite()).any()) and bool((h == 65504).any())
    sub = (h != 0) & (h.abs() < 2.0 ** -14)
    assert int(sub.sum()) >= 20
    assert bool(((h == 0) & (e != 0)).any())
    assert float(torch.tensor(65520.0).half()) == float("inf")
    assert float(torch.tensor([R.cast_edge_values()[0]]).bfloat16()) == 1.0   # 0x3F808000: tie -> even
    # bf16: overflow by rounding from finite f32
    assert bool((b.isinf() & e.isfinite()).any())
    # ties of both parities, in both formats: the value lies exactly between two neighbours and the
    # cast went once down and once up
    for t, it_bits in ((h, 13), (b, 16)):
        fin = e.isfinite() & t.isfinite() & (t.abs().float() >= 2.0 ** -14)
        low = e.view(torch.int32) & ((1 << it_bits) - 1)
        tie = fin & (low == (1 << (it_bits - 1)))
        up = tie & (t.float().abs() > e.abs())
        down = tie & (t.float().abs() < e.abs())
        assert bool(up.any()) and bool(down.any())
    # cast_matches: NaN by class, everything else by bits
    assert bool(R.cast_matches(h, e).all())
    wrong = h.clone()
    wrong[3] = wrong[3] + 1
    assert not bool(R.cast_matches(wrong, e).all())
    assert R.cast_input(1).numel() == 1 and R.cast_input(255).numel() == 255
    big = R.cast_input(1000)
    assert torch.equal(big[:e.numel()][~e.isnan()], e[~e.isnan()])
    assert not bool(((big != 0) & (big.abs() < tiny32)).any())


def test_bn_eval_ref_matches_torch_and_yardstick_is_small():
    g = R._gen(9)
    C = 257
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    mean, var = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64)
    var[0], var[1] = 0.0, 1e4
    sc, sh = R.bn_eval_ref(gamma, beta, mean, var, 1e-5)
    x = torch.randn(4, C, 3, 3, generator=g, dtype=F64)
    ref = F.batch_norm(x, mean, var, gamma, beta, training=False, eps=1e-5)
    torch.testing.assert_close(x * sc[None, :, None, None] + sh[None, :, None, None], ref,
                               rtol=1e-12, atol=1e-12)
    yard = R.rsqrt_yardstick(var.float(), 1e-5)
    print(f"f32 rsqrt(var + eps) yardstick: {yard:.3g}")
    assert 0 < yard < 2.0 ** -22
