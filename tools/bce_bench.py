"""Cost of the sigmoid loss on the ResNet-50 head (B x 1000 f32 logits, bf16 gradient of the padded
width):

  (a) xent_soft : softmax loss + gradient, eps = 0.1, lam = 0.3, two label sets (csrc/mix.hip)
  (b) bce_soft  : the sigmoid loss + gradient on the same arguments (csrc/bce.hip)
  (c) bce_soft with target threshold 0.2

timed with device events around ``--iters`` back-to-back launches after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round (the spread is printed), and the end-to-end step of
the native bf16 trainer with the ``ce`` and the ``bce`` criterion on the same eager calls (smoothing
0.1, a second label set, lam 0.3), alternating on one trainer. Bytes are what the launch must move:
the logits once and the gradient once. Writes markdown to ``--out`` (the accuracy figures of
profiles/bce.md come from the tests' own output, not from here).

    python tools/bce_bench.py --out profiles/bce_bench.md
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _round(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bce_bench.md")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import native_ops as K
    dev = torch.device("cuda", 0)
    B, NC = args.batch, 1000
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    m = tr.model
    tr.step(0)
    torch.cuda.synchronize()

    # ---- the kernels alone
    g = torch.Generator(device="cpu").manual_seed(0)
    logits = (torch.randn(B, NC, generator=g) * 3).to(dev)
    y = torch.randint(0, NC, (B,), generator=g).to(dev)
    yb = y.roll(1, 0).contiguous()
    rows, loss = torch.empty(B, device=dev), torch.empty((), device=dev)
    dlog = torch.empty(B, m.fc_rows, dtype=torch.bfloat16, device=dev)
    soft = dict(labels_b=yb, lam=0.3, eps=0.1, dlog=dlog)
    runs = {
        "(a) xent_soft": lambda: K.xent_soft(logits, y, rows, loss, gscale=1.0 / B, **soft),
        "(b) bce_soft": lambda: K.bce_soft(logits, y, rows, loss, **soft),
        "(c) bce_soft, thresh 0.2": lambda: K.bce_soft(logits, y, rows, loss, thresh=0.2, **soft),
    }
    nbytes = B * NC * 4 + dlog.numel() * 2
    for fn in runs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            times[k].append(_round(fn, args.iters))
    lines = ["# Sigmoid loss: kernel and step cost (ResNet-50 head, bf16 gradient)", "",
             f"`tools/bce_bench.py`: logits {B} x {NC} f32, bf16 gradient of {m.fc_rows} columns, loss rows "
             f"and the mean launch included; device events around {args.iters} back-to-back launches, "
             f"{args.rounds} rounds, the variants taking turns inside every round.", "",
             "| variant | us / call (median) | min .. max | bytes moved | GB/s |", "|---|---|---|---|---|"]
    for k, t in times.items():
        med = statistics.median(t)
        lines.append(f"| {k} | {med:.2f} | {min(t):.2f} .. {max(t):.2f} | {nbytes} | {nbytes / med / 1e3:.0f} |")
        print(lines[-1], flush=True)

    # ---- end to end: one trainer, the same eager calls, the two criteria alternating
    crits = {"ce": m.make_criterion(label_smoothing=0.1),
             "bce": m.make_criterion(label_smoothing=0.1, loss="bce")}

    def step(crit, i):
        xs, ys = tr.gen(torch.arange(B, dtype=torch.int64) + i * B)
        l = crit(tr.net(xs), ys, ys.roll(1, 0), 0.3)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        return l

    step_ms = {k: [] for k in crits}
    i, last = 1, None
    for r in range(args.step_rounds + 1):
        for name, crit in crits.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                last = step(crit, i)
                i += 1
            b.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms both up
                step_ms[name].append(a.elapsed_time(b) / args.steps)
    lines += ["", f"End to end: native bf16 training step, batch {B}, smoothing 0.1, a second label set, lam "
              f"0.3; {args.steps} steps per round, the two criteria alternating on one trainer, "
              f"{args.step_rounds} rounds after a warm-up round.", "",
              "| criterion | ms / step (median) | min .. max |", "|---|---|---|"]
    for name, t in step_ms.items():
        lines.append(f"| {name} | {statistics.median(t):.3f} | {min(t):.3f} .. {max(t):.3f} |")
        print(lines[-1], flush=True)
    assert bool(last.isfinite()), "non-finite loss"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
