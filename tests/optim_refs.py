"""float64 reference of the segmented optimizer update (csrc/optim.hip, pytorch_distributed_amd/optim.py).

Per segment (one parameter tensor), with the gradient unscaled by ``inv``::

    q = trust * |p| / (inv |g| + wd |p| + eps)   if trust > 0 and |p| > 0 and inv |g| > 0, else 1
    d = q * (g inv + wd p);  b = momentum b + d (first step b = d)
    p -= lr * (d + momentum b if nesterov else b)

q is rounded to float32 once (as every implementation hands it to its f32 update); everything else is
float64, carried in float64 across the steps. Checked against torch.optim.SGD in
tests/test_optim_refs_cpu.py.
"""
import torch

F64 = torch.float64
HYPER_DEFAULTS = dict(momentum=0.0, weight_decay=0.0, nesterov=False, lars=0.0, lars_eps=1e-8)


def trust_ratio(p64, g64, h, inv=1.0):
    """The trust ratio of one tensor as a Python float (float32-rounded); 1.0 when off or degenerate."""
    trust = h.get("lars", 0.0)
    if not trust > 0:
        return 1.0
    wd, eps = h.get("weight_decay", 0.0), h.get("lars_eps", 1e-8)
    wn = float(p64.pow(2).sum().sqrt())
    gn = float(inv) * float(g64.pow(2).sum().sqrt())
    if not (wn > 0 and gn > 0):
        return 1.0
    return float(torch.tensor(trust * wn / (gn + wd * wn + eps), dtype=F64).to(torch.float32))


def seg_sgd_ref(p, g, segments, hyper, steps: int, inv=1.0, shadow_dtype=None):
    """``p``, ``g``: flat float32 CPU tensors; ``segments``: [(offset, numel)]; ``hyper``: one dict per
    segment (``lr`` and optionally the HYPER_DEFAULTS keys). Returns one (p32, buf32, shadow) per
    step: flat float32 roundings of the float64 state (elements in no segment: p as given, buf 0) and
    torch's cast of that p32 to ``shadow_dtype`` (None without one). The gradient is reused."""
    p64 = p.to(F64).clone()
    g64 = g.to(F64)
    buf = torch.zeros_like(p64)
    out = []
    for it in range(steps):
        for (off, n), h in zip(segments, hyper):
            h = {**HYPER_DEFAULTS, **h}
            sl = slice(off, off + n)
            ps, gs = p64[sl], g64[sl]
            q = trust_ratio(ps, gs, h, inv)
            d = q * (gs * inv + h["weight_decay"] * ps)
            b = d.clone() if it == 0 else h["momentum"] * buf[sl] + d
            buf[sl] = b
            step = d + h["momentum"] * b if h["nesterov"] else b
            p64[sl] = ps - h["lr"] * step
        p32 = p64.to(torch.float32)
        out.append((p32, buf.to(torch.float32), None if shadow_dtype is None else p32.to(shadow_dtype)))
    return out


def param_segments(params):
    """[(offset, numel)] of tensors laid end to end in one flat buffer."""
    segs, off = [], 0
    for t in params:
        segs.append((off, t.numel()))
        off += t.numel()
    return segs
