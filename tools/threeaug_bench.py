"""Cost of the 3-Augment on the ResNet-50 shapes (batch: B x 224 px, s2d bf16), launch by launch:

  (a) three_aug_draw                 (b) three_aug on the drawn table (a third of the samples per op)
  (c) every sample grayscale         (d) every sample solarize      (e) every sample blur, R = 11
  (f) jitter_mean + batch_jitter (MX_COLOR_JITTER=0.4)     (g) randaug_stats + randaug_apply with
  every sample on Sharpness (the 3x3 neighbourhood fetched element-wise through L2)   -- yardsticks

timed with device events around ``--iters`` back-to-back calls after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round (the spread is printed), and the end-to-end step of
the native bf16 trainer with and without ``MX_THREE_AUGMENT=1``, alternating. The apply is out of
place, so repeated calls read the same source; the per-pixel work is branch-free within an op, so the
time does not depend on the values. Bytes are what the launch must move: the batch read and written
once. Writes markdown to ``--out``.

    python tools/threeaug_bench.py --out profiles/threeaug.md
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.erase_bench import _time_alternating  # noqa: E402


class _Ctx:
    rank, engine = 0, "native"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/threeaug.md")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd import jitter as J, randaug as RA, threeaug as T
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import native_ops as K
    dev = torch.device("cuda", 0)
    B, S = args.batch, 224
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    tr.step(0)
    torch.cuda.synchronize()

    # ---- the launches alone
    x, _ = tr.gen(torch.arange(B, dtype=torch.int64))
    x = x.clone()
    out = torch.empty_like(x)
    drawn = torch.empty(B, 16, dtype=torch.int32, device=dev)
    K.three_aug_draw(drawn, T.batch_key(0, 0, 0, 0))
    each = {op: torch.tensor(T.three_aug_table([op] * B, [1.0] * B, T.RADIUS), device=dev) for op in (0, 1, 2)}
    tj = torch.empty(B, 5, dtype=torch.int32, device=dev)
    K.jitter_draw(tj, J.batch_key(0, 0, 0, 0), (0.4, 0.4, 0.4, 0.0))
    jslab = torch.empty(B * K.jitter_bps(B, S, x.dtype, K.AUG_S2D), dtype=torch.float64, device=dev)
    rows = RA.draw_randaug(0, 0, 0, 0, 4096, S, 1, 9)        # a drawn Sharpness row, every sample on it
    sharp = torch.tensor(np.repeat(rows[rows[:, 0, 0] == RA.OPS.index("Sharpness")][:1], B, 0), device=dev)
    rstats = torch.zeros(B * K.randaug_stat_row(), dtype=torch.int32, device=dev)
    rslab = torch.empty(B * K.randaug_bps(B, S, x.dtype, K.AUG_S2D), dtype=torch.float64, device=dev)

    def sharpness():
        K.randaug_stats(x, sharp, 0, rstats, rslab, K.AUG_S2D)
        K.randaug_apply(x, out, sharp, 0, rstats, rslab, K.AUG_S2D)

    apply = lambda t: (lambda: K.three_aug(x, out, t, K.AUG_S2D, max_r=T.RADIUS))
    runs = {"a": lambda: K.three_aug_draw(drawn, T.batch_key(0, 0, 0, 0)), "b": apply(drawn), "c": apply(each[0]),
            "d": apply(each[1]), "e": apply(each[2]), "f": lambda: K.batch_jitter(x, tj, K.AUG_S2D, jslab),
            "g": sharpness}
    xb = x.numel() * 2
    nbytes = {"a": B * 64, "b": 2 * xb, "c": 2 * xb, "d": 2 * xb, "e": 2 * xb, "f": 3 * xb, "g": 2 * xb}
    names = {"a": "three_aug_draw", "b": "three_aug, the drawn table", "c": "three_aug, all grayscale",
             "d": "three_aug, all solarize", "e": "three_aug, all blur (R = 11, sigma 1)",
             "f": "jitter_mean + batch_jitter, b/c/s", "g": "randaug_stats + randaug_apply, all Sharpness"}
    ops = np.bincount(drawn.cpu().numpy()[:, 0], minlength=3)
    lines = ["# 3-Augment: launch and step cost (ResNet-50 shapes)", "",
             f"`tools/threeaug_bench.py`: batch {tuple(x.shape)} bf16 ({xb} bytes); the drawn table holds "
             f"{ops[0]} grayscale, {ops[1]} solarize and {ops[2]} blur samples; device events around {args.iters} "
             f"back-to-back calls, {args.rounds} rounds, the variants taking turns inside every round.", "",
             "| launch | us / call (median) | min .. max | bytes moved | TB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in runs:
        t = times[k]
        med = statistics.median(t)
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k]} | "
                     f"{nbytes[k] / med / 1e6:.2f} |")
        print(lines[-1], flush=True)

    # ---- end to end: the same trainer, the plain step and the augmenting step alternating
    three = T.BatchThreeAugment(config_for("single", env={"MX_THREE_AUGMENT": "1", "MX_IMAGE_SIZE": str(S)}), _Ctx())
    crit = tr.model.make_criterion()

    def eager_step(i, aug=None):
        xs, ys = tr.gen(torch.arange(B, dtype=torch.int64) + i * B)
        if aug is not None:
            xs = aug(xs, 0, i)
        l = crit(tr.net(xs), ys)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        tr._loss = l.detach()

    step_ms = {"NativeTrainer.step": [], "the same step made of the trainer's eager calls": [],
               "the eager calls with MX_THREE_AUGMENT=1": []}
    i = 1
    for r in range(args.step_rounds + 1):
        for name, fn in zip(step_ms, (tr.step, eager_step, lambda i: eager_step(i, three))):
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
