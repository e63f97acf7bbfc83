"""Cost of random erasing on the ResNet-50 shapes (batch: B x 224 px):

  (a) erase_draw + batch_erase, s2d bf16, p = 0.25
  (b) the same, p = 1
  (c) erase_draw + batch_erase, NCHW f32, p = 0.25
  (d) the same, p = 1
  (e) erase_draw alone (p = 1)

timed with device events around ``--iters`` back-to-back calls after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round (the spread is printed), and the end-to-end step
of the native bf16 trainer with and without ``MX_RANDOM_ERASE=0.25``, alternating. The erase is in
place and idempotent, so repeating it on one batch writes the same bytes every time. Bytes are what
the operation must move: the erased pixels, written once (nothing is read but the 16-byte table
rows); the boxes are those of the host mirror ``erase.draw_erase`` for the same key. Writes markdown
to ``--out``.

    python tools/erase_bench.py --out profiles/erase.md
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
    ap.add_argument("--out", default="profiles/erase.md")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.erase import BatchEraser, batch_key, draw_erase
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import native_ops as K
    dev = torch.device("cuda", 0)
    B, S = args.batch, 224
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    tr.step(0)
    torch.cuda.synchronize()

    # ---- the kernels alone
    x, _ = tr.gen(torch.arange(B, dtype=torch.int64))
    x = x.clone()
    n = torch.randn(B, 3, S, S, device=dev)
    table = torch.empty(B, 4, dtype=torch.int32, device=dev)
    key = batch_key(0, 0, 0, 0)

    def pair(t, layout, p):
        def fn():
            K.erase_draw(table, S, key, p)
            K.batch_erase(t, table, layout)
        return fn
    runs = {"a": pair(x, K.AUG_S2D, 0.25), "b": pair(x, K.AUG_S2D, 1.0),
            "c": pair(n, K.AUG_NCHW, 0.25), "d": pair(n, K.AUG_NCHW, 1.0),
            "e": lambda: K.erase_draw(table, S, key, 1.0)}
    pixels = {p: int(sum((y2 - y1) * (x2 - x1) for y1, y2, x1, x2 in draw_erase(0, 0, 0, 0, B, S, p).tolist()))
              for p in (0.25, 1.0)}
    nbytes = {"a": pixels[0.25] * 6, "b": pixels[1.0] * 6, "c": pixels[0.25] * 12, "d": pixels[1.0] * 12,
              "e": B * 16}
    names = {"a": "draw + erase, s2d bf16, p = 0.25", "b": "draw + erase, s2d bf16, p = 1",
             "c": "draw + erase, NCHW f32, p = 0.25", "d": "draw + erase, NCHW f32, p = 1",
             "e": "erase_draw alone, p = 1"}
    whole = {"s2d bf16": x.numel() * 2, "NCHW f32": n.numel() * 4}
    lines = ["# Random erasing: kernel and step cost (ResNet-50 shapes)", "",
             f"`tools/erase_bench.py`: batch {tuple(x.shape)} bf16 ({whole['s2d bf16']} bytes) and "
             f"{tuple(n.shape)} f32 ({whole['NCHW f32']} bytes); device events around {args.iters} "
             f"back-to-back calls, {args.rounds} rounds, the variants taking turns inside every round. "
             f"Erased pixels of the batch: {pixels[0.25]} at p = 0.25, {pixels[1.0]} at p = 1 "
             f"({100 * pixels[1.0] / (B * S * S):.1f} % of the batch).", "",
             "| variant | us / call (median) | min .. max | bytes written | GB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in "abcde":
        t = times[k]
        med = statistics.median(t)
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k]} | "
                     f"{nbytes[k] / med / 1e3:.0f} |")
        print(lines[-1], flush=True)

    # ---- end to end: the same trainer, the plain step and the erasing step alternating
    cfg = config_for("single", env={"MX_RANDOM_ERASE": "0.25", "MX_IMAGE_SIZE": str(S)})
    eraser = BatchEraser(cfg, _Ctx())
    crit = tr.model.make_criterion()

    def plain_step(i):
        ids = torch.arange(B, dtype=torch.int64) + i * B
        xs, ys = tr.gen(ids)
        l = crit(tr.net(xs), ys)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        tr._loss = l.detach()

    def erase_step(i):
        ids = torch.arange(B, dtype=torch.int64) + i * B
        xs, ys = tr.gen(ids)
        xs = eraser(xs, 0, i)
        l = crit(tr.net(xs), ys)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        tr._loss = l.detach()

    step_ms = {"NativeTrainer.step": [], "the same step made of the trainer's eager calls": [],
               "the eager calls with MX_RANDOM_ERASE=0.25": []}
    i = 1
    for r in range(args.step_rounds + 1):
        for name, fn in zip(step_ms, (tr.step, plain_step, erase_step)):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn(i)
                i += 1
            b.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms all of them up
                step_ms[name].append(a.elapsed_time(b) / args.steps)
    lines += ["", f"End to end: native bf16 training step, batch {B}, {args.steps} steps per round, the "
              f"steps alternating on one trainer, {args.step_rounds} rounds after a warm-up round.", "",
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
