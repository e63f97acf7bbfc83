"""float64 reference of the sigmoid cross-entropy on soft targets (csrc/bce.hip, mix.soft_bce),
written out from its definition. Runs on the CPU and uses no code of this project."""
import torch

F64 = torch.float64
# target cases (name, eps, second labels: None | "other" (a != b where K > 1) | "same", lam, thresh)
CASES = [("hard", 0.0, None, 1.0, None), ("smoothed", 0.1, None, 1.0, None),
         ("mixed", 0.1, "other", 0.3, None), ("mixed-same", 0.1, "same", 0.3, None),
         ("lam0", 0.1, "other", 0.0, None), ("lam1", 0.1, "other", 1.0, None),
         ("thresh", 0.1, "other", 0.9, 0.2),          # b's q = eps/K + 0.09 lies below 0.2
         ("thresh-equal", 0.0, "other", 0.25, 0.25)]  # a's q = 0.25 exactly: not above -> t = 0


def f32(v):
    """``v`` as the kernel receives it (a C float); None stays None."""
    return None if v is None else float(torch.tensor(v, dtype=torch.float32))


def labels_for(B: int, K: int, second, g: torch.Generator):
    a = torch.randint(0, K, (B,), generator=g)
    other = (a + 1 + torch.randint(0, max(K - 1, 1), (B,), generator=g)) % K
    return a, {None: None, "same": a.clone(), "other": other}[second]


def logits_for(B: int, K: int, a, b, g: torch.Generator, dtype=torch.float32):
    """3 * N(0, 1) with 0, +-30 and +-100 planted where K > 1 (a single element keeps its random
    logit), +100 under row B-1's first label and -100 under its second: 1 - t and -t with t > 0."""
    x = 3.0 * torch.randn(B, K, generator=g, dtype=dtype)
    if K > 1:
        for i, v in enumerate((0.0, 30.0, -30.0, 100.0, -100.0)):
            x[i % B, (7 * i) % K] = v
        x[B - 1, a[B - 1]] = 100.0
        if b is not None:
            x[B - 1, b[B - 1]] = -100.0
    return x


def bce_soft_ref(x, a, b, lam: float, eps: float, thresh=None, sum_classes: bool = False):
    """(loss_rows, t, d mean(loss_rows) / dz) in float64. q = eps/K + (1-eps)*lam*[k==a] +
    (1-eps)*(1-lam)*[k==b], added in that order (``b`` None: b = a); t = q, or [q > thresh];
    l = max(z,0) - z*t + log1p(exp(-|z|)); rows = mean (``sum_classes``: sum) of l over the
    classes; dl = sigmoid(z) - t."""
    z = x.to(F64)
    B, K = z.shape
    k = torch.arange(K)[None, :]
    q = eps / K + ((1.0 - eps) * lam) * (k == a[:, None]).to(F64)
    q = q + ((1.0 - eps) * (1.0 - lam)) * (k == (a if b is None else b)[:, None]).to(F64)
    t = q if thresh is None else (q > thresh).to(F64)
    e = torch.exp(-z.abs())
    l = z.clamp_min(0) - z * t + torch.log1p(e)
    s = torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return (l.sum(1) if sum_classes else l.sum(1) / K), t, (s - t) / (B if sum_classes else B * K)
