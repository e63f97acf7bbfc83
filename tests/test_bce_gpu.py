"""bce_soft (csrc/bce.hip) against tests/bce_refs.py. f32 outputs: at most 4x the error of torch's own
float32 binary_cross_entropy_with_logits + autograd on the same device, inputs and dense target (other
summation order, exp, log1p) + one f32 ulp of the largest reference magnitude; 16-bit dlog: 1 ulp."""
import pytest
import torch
import torch.nn.functional as F

import bce_refs as R
import head_refs as H
from pytorch_distributed_amd.ops import ext, native_ops as K_

pytestmark = pytest.mark.gpu
DEV, F64 = "cuda", torch.float64
# (B, K, ld_in, ld_out): one element; a second block with one live wave, unaligned rows; whole units;
# whole units plus a tail behind padded strides; a half unit (K/4 odd) plus a tail; the ResNet head;
# unaligned plus tail; a second pass over the row (K > 1024) that ends in a half unit
SHAPES = [(1, 1, 1, 8), (5, 63, 63, 64), (4, 64, 64, 64), (3, 65, 68, 72), (3, 69, 72, 72),
          (2, 1000, 1024, 1024), (2, 1003, 1003, 1008), (1, 2052, 2052, 2056)]
GS, GD = 0.5, 4.0      # gscale and the device scalar: powers of two, so their product is exact


@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_bce_soft_matches_the_float64_reference(shape, sum_classes):
    B, K, ld_in, ld_out = shape
    for ci, (name, eps, second, lam, thresh) in enumerate(R.CASES):
        g = torch.Generator().manual_seed(1000 * K + 10 * ci + B)
        a, b = R.labels_for(B, K, second, g)
        xc = R.logits_for(B, K, a, b, g)
        rows64, t, d = R.bce_soft_ref(xc, a, b, R.f32(lam), R.f32(eps), R.f32(thresh), sum_classes)
        ref = {"rows": rows64, "loss": rows64.mean(), "grad": d * (GS * GD)}
        x = torch.full((B, ld_in), float("nan")).to(DEV)[:, :K].copy_(xc)      # NaN beyond the row
        zt = x.clone().requires_grad_()
        lt = F.binary_cross_entropy_with_logits(zt, t.float().to(DEV), reduction="none")
        rows_t = lt.sum(1) if sum_classes else lt.mean(1)
        rows_t.mean().backward(torch.tensor(GS * GD, device=DEV))
        yard = {"rows": rows_t.detach(), "loss": rows_t.mean().detach(), "grad": zt.grad}
        yerr = {k: float((yard[k].cpu().to(F64) - ref[k]).abs().max()) for k in ref}
        bar = {k: 4 * yerr[k] + float(H.ulp_out(ref[k].abs().max(), torch.float32)) for k in ref}
        kw = dict(labels_b=None if b is None else b.to(DEV), lam=lam, eps=eps, thresh=thresh,
                  sum_classes=sum_classes, gscale=GS, gdev=torch.tensor([GD], device=DEV))
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            runs = []
            for _ in range(2):
                rows, loss = torch.full((B,), -5.0, device=DEV), torch.full((), -5.0, device=DEV)
                dlog = torch.full((B, ld_out), 7.0, dtype=dtype, device=DEV)
                K_.bce_soft(x, a.to(DEV), rows, loss, dlog=dlog, **kw)
                runs.append((rows.cpu(), loss.cpu(), dlog.cpu()))
            rows, loss, dlog = runs[0]
            # runs repeat bit for bit; the padding columns are 0
            assert all(H.same_bits(p, q) for p, q in zip(*runs)) and bool((dlog[:, K:] == 0).all()), name
            got = {"rows": rows.to(F64), "loss": loss.to(F64), "grad": dlog[:, :K].to(F64)}
            err = {k: float((got[k] - ref[k]).abs().max()) for k in got}
            assert err["rows"] <= bar["rows"] and err["loss"] <= bar["loss"], (name, err, bar)
            # f32: the bar, against the reference; 16-bit: 1 ulp, against the reference rounded to the dtype
            tol = bar["grad"] if dtype == torch.float32 else H.ulp_out(ref["grad"], dtype)
            refg = ref["grad"] if dtype == torch.float32 else ref["grad"].to(dtype).to(F64)
            assert bool(((got["grad"] - refg).abs() <= tol).all()), (name, err, bar)
            if thresh is not None or name == "hard":      # t in {0, 1}: at z = +-100 exactly (1-t or -t) * scale
                want = ((xc > 0).to(F64) - t) * (GS * GD / (B if sum_classes else B * K))
                assert bool(((got["grad"] - want.to(dtype).to(F64))[xc.abs() == 100.0].abs() <= 1e-43).all()), name


def test_bce_soft_refusals_and_want_grad_off():
    """Refused: ValueError (the launcher itself: -2), the sentinels stay. want_grad = 0: dlog stays."""
    z = lambda *shape, **kw: torch.zeros(*shape, device=DEV, **kw)
    x, lab, rows, loss, nan = z(4, 10), z(4, dtype=torch.long), z(4) - 5, z(()) - 5, float("nan")
    dlog = z(4, 16) + 7
    for kw in (dict(eps=1.0), dict(eps=-0.1), dict(eps=nan), dict(lam=1.5), dict(lam=-0.25), dict(lam=nan),
               dict(thresh=1.0), dict(thresh=-0.5), dict(thresh=nan), dict(labels_b=lab[:3]),
               dict(dlog=z(4, 8, dtype=torch.bfloat16)), dict(dlog=z(4, 16, dtype=F64)),   # ld_out < K, dtype
               dict(logits=z(0, 10)), dict(logits=z(4, 0)), dict(logits=z(40).as_strided((4, 10), (5, 1)))):
        with pytest.raises(ValueError):
            K_.bce_soft(kw.pop("logits", x), lab, rows, loss, **kw)
    good = dict(logits=x.data_ptr(), B=4, K=10, ld_in=10, labels=lab.data_ptr(), labels_b=None, lam=1.0, eps=0.0,
                thresh=-1.0, mode=0, loss_rows=rows.data_ptr(), loss=loss.data_ptr(), dlog=dlog.data_ptr(), ld_out=16,
                gscale=1.0, gdev=None, dt=0, want_grad=1, st=ext.stream(x.device))    # pda_bce_soft's parameters
    for bad in (dict(mode=2), dict(B=0), dict(K=0), dict(ld_in=9), dict(ld_out=9), dict(dt=7), dict(thresh=nan)):
        assert ext.lib().pda_bce_soft(*{**good, **bad}.values()) == -2, bad
    assert bool((rows == -5.0).all()) and float(loss) == -5.0 and bool((dlog == 7.0).all())
    assert ext.lib().pda_bce_soft(*{**good, "want_grad": 0}.values()) == 0     # (the good call launches)
    assert abs(float(loss) - 0.6931472) < 1e-6 and bool((dlog == 7.0).all())
