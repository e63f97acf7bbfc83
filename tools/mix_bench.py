"""Cost of label smoothing, mixup and CutMix on the ResNet-50 shapes (head: B x 1000 logits; batch:
B x 224 px, s2d bf16):

  (a) xent        : the hard-label loss + gradient launch (loss, rows, bf16 dlog)
  (b) xent_soft   : the same with eps = 0.1, lam = 0.3 and a second label set
  (c) batch_mix, mixup
  (d) batch_mix, CutMix with a centred box of half the image's area

timed with device events around ``--iters`` back-to-back launches after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round (the spread is printed), and the end-to-end step
of the native bf16 trainer with and without smoothing 0.1 + mixup 0.2 + CutMix 1.0, alternating.
Bytes are what the operation must move: mixup reads two batches and writes one, CutMix reads one
batch's worth (each pixel from one source) and writes one. Writes markdown to ``--out``.

    python tools/mix_bench.py --out profiles/mix.md
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


def _time_alternating(runs, iters, rounds, warmup=10):
    for fn in runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            out[k].append(_round(fn, iters))
    return out


class _Ctx:
    rank, engine = 0, "native"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/mix.md")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.mix import BatchMixer
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import native_ops as K
    dev = torch.device("cuda", 0)
    B, S, NC = args.batch, 224, 1000
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    m = tr.model
    tr.step(0)
    torch.cuda.synchronize()

    # ---- the kernels alone
    g = torch.Generator(device="cpu").manual_seed(0)
    logits = (torch.randn(B, NC, generator=g) * 3).to(dev)
    y = torch.randint(0, NC, (B,), generator=g).to(dev)
    yb = y.roll(1, 0).contiguous()
    rows = torch.empty(B, device=dev)
    loss = torch.empty((), device=dev)
    dlog = torch.empty(B, m.fc_rows, dtype=torch.bfloat16, device=dev)
    x, _ = tr.gen(torch.arange(B, dtype=torch.int64))
    out = torch.empty_like(x)
    h = int(round(S * 0.5 ** 0.5 / 2))
    box = (S // 2 - h, S // 2 + h, S // 2 - h, S // 2 + h)
    runs = {
        "a": lambda: K.xent(logits, y, rows, loss, dlog=dlog, gscale=1.0 / B),
        "b": lambda: K.xent_soft(logits, y, rows, loss, labels_b=yb, lam=0.3, eps=0.1, dlog=dlog,
                                 gscale=1.0 / B),
        "c": lambda: K.batch_mix(x, out, K.AUG_S2D, K.MIX_MIXUP, 0.3),
        "d": lambda: K.batch_mix(x, out, K.AUG_S2D, K.MIX_CUTMIX, 0.5, box),
    }
    nb = x.numel() * x.element_size()
    head = B * NC * 4 + dlog.numel() * 2
    nbytes = {"a": head, "b": head, "c": 3 * nb, "d": 2 * nb}
    names = {"a": "xent (hard labels)", "b": "xent_soft (eps 0.1, lam 0.3, two label sets)",
             "c": "batch_mix, mixup", "d": f"batch_mix, CutMix box {box}"}
    lines = ["# Label smoothing, mixup and CutMix: kernel and step cost (ResNet-50 shapes, bf16)", "",
             f"`tools/mix_bench.py`: logits {B} x {NC} f32 with a bf16 gradient of {m.fc_rows} columns; "
             f"batch {tuple(x.shape)} bf16 ({nb} bytes); device events around {args.iters} back-to-back "
             f"launches, {args.rounds} rounds, the variants taking turns inside every round.", "",
             "| variant | us / call (median) | min .. max | bytes moved | GB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in "abcd":
        t = times[k]
        med = statistics.median(t)
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k]} | "
                     f"{nbytes[k] / med / 1e3:.0f} |")
        print(lines[-1], flush=True)

    # ---- end to end: the same trainer, the plain step and the soft-target step alternating
    cfg = config_for("single", env={"MX_LABEL_SMOOTHING": "0.1", "MX_MIXUP": "0.2", "MX_CUTMIX": "1.0",
                                    "MX_IMAGE_SIZE": str(S)})
    mixer = BatchMixer(cfg, _Ctx())
    soft = m.make_criterion(label_smoothing=cfg.label_smoothing)

    def soft_step(i):
        ids = torch.arange(B, dtype=torch.int64) + i * B
        xs, ys = tr.gen(ids)
        xs, ys, ysb, lam = mixer(xs, ys, 0, i)
        l = soft(tr.net(xs), ys, ysb, lam)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        tr._loss = l.detach()

    step_ms = {"default": [], "smoothing 0.1 + mixup 0.2 + CutMix 1.0": []}
    i = 1
    for r in range(args.step_rounds + 1):
        for name, fn in zip(step_ms, (tr.step, soft_step)):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn(i)
                i += 1
            b.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms both up
                step_ms[name].append(a.elapsed_time(b) / args.steps)
    lines += ["", f"End to end: native bf16 training step, batch {B}, {args.steps} steps per round, the "
              f"two steps alternating on one trainer, {args.step_rounds} rounds after a warm-up round.", "",
              "| step | ms / step (median) | min .. max |", "|---|---|---|"]
    for name, t in step_ms.items():
        lines.append(f"| {name} | {statistics.median(t):.3f} | {min(t):.3f} .. {max(t):.3f} |")
        print(lines[-1], flush=True)
    assert tr.last_loss() == tr.last_loss(), "non-finite loss"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
