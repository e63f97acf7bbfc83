"""float64 reference of the AdamW / LAMB update (csrc/adam.hip, pytorch_distributed_amd/optim.py spell it
out), per segment, with the gradient unscaled by ``inv`` and t the step number. c1, c2 and r are
rounded to float32 once (as every implementation hands them to its f32 update); everything else is
float64, carried in float64 across the steps. Checked against torch.optim.AdamW in
tests/test_adam_cpu.py."""
import torch

F64 = torch.float64
HYPER_DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, lamb=False)
_f32 = lambda x: float(torch.tensor(x, dtype=F64).to(torch.float32))      # noqa: E731


def adam_ref(p, g, segments, hyper, steps: int, inv=1.0, shadow_dtype=None):
    """``p``, ``g``: flat float32 CPU tensors; ``segments``: [(offset, numel)]; ``hyper``: one dict per
    segment (``lr`` and optionally the HYPER_DEFAULTS keys). Returns one (p32, m32, v32, shadow) per
    step: flat float32 roundings of the float64 state (elements in no segment: p as given, m and v 0)
    and torch's cast of that p32 to ``shadow_dtype`` (None without one). The gradient is reused."""
    p64 = p.to(F64).clone()
    gs = g.to(F64) * inv
    m, v = torch.zeros_like(p64), torch.zeros_like(p64)
    out = []
    for t in range(1, steps + 1):
        for (off, n), h in zip(segments, hyper):
            h = {**HYPER_DEFAULTS, **h}
            sl = slice(off, off + n)
            (b1, b2), lr, wd = h["betas"], h["lr"], h["weight_decay"]
            m[sl] = b1 * m[sl] + (1 - b1) * gs[sl]
            v[sl] = b2 * v[sl] + (1 - b2) * gs[sl] ** 2
            c1, c2 = _f32(1 / (1 - b1 ** t)), _f32(1 / (1 - b2 ** t) ** 0.5)
            a = (m[sl] * c1) / (v[sl].sqrt() * c2 + h["eps"])
            if h["lamb"]:
                u = a + wd * p64[sl]
                wn, un = float(p64[sl].pow(2).sum().sqrt()), float(u.pow(2).sum().sqrt())
                r = _f32(wn / un) if wn > 0 and un > 0 else 1.0
                p64[sl] = p64[sl] - lr * r * u
            else:
                p64[sl] = p64[sl] * (1 - lr * wd) - lr * a
        p32 = p64.to(torch.float32)
        out.append((p32, m.to(torch.float32), v.to(torch.float32),
                    None if shadow_dtype is None else p32.to(shadow_dtype)))
    return out


def torch_steps(opt, params, grads, steps: int):
    """``steps`` steps of a torch optimizer over ``params`` with ``grads`` held fixed. Returns one
    (p, m, v) per step, each the parameters' tensors flattened and joined in order."""
    for p, g in zip(params, grads):
        p.grad = g.clone()
    out = []
    for _ in range(steps):
        opt.step()
        out.append(tuple(torch.cat([x.detach().flatten() for x in xs]) for xs in
                         (params, *([opt.state[p][k] for p in params] for k in ("exp_avg", "exp_avg_sq")))))
    return out
