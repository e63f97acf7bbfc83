"""Cost of RandAugment on the ResNet-50 shapes (batch: B x 224 px, bf16 s2d), launch by launch:

  (a) randaug_draw, n = 2, m = 9
  (b) randaug_stats, one slot of the drawn table   (c) randaug_apply, the same slot
  (d) the whole n = 2 chain: the draw and two stats + apply slots (BatchRandAugment)
  (e) one stats + apply slot with EVERY sample on one op, for each of the 14 ops
  (g) batch_jitter (b/c/s, with its mean pass)     (h) batch_mix (mixup)             -- yardsticks

timed with device events around ``--iters`` back-to-back calls after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round (the spread is printed), and the end-to-end step of
the native bf16 trainer with and without ``MX_RAND_AUGMENT=2,9``, alternating. The chain is not
idempotent (repeated, the pictures drift), but no op's work depends on the values, except that the
Equalize histogram's LDS atomics collide more on flat pictures. Bytes are what a launch must move: the
stats pass reads the samples whose op takes a statistic, the apply reads and writes every sample.
Writes markdown to ``--out``.

    python tools/randaug_bench.py --out profiles/randaug.md
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
    ap.add_argument("--out", default="profiles/randaug.md")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd import randaug as A
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.jitter import batch_key as jitter_key
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import native_ops as K
    dev = torch.device("cuda", 0)
    B, S, n, m = args.batch, 224, 2, 9
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    tr.step(0)
    torch.cuda.synchronize()

    # ---- the launches alone
    x, _ = tr.gen(torch.arange(B, dtype=torch.int64))
    x = x.clone()
    out = torch.empty_like(x)
    cfg = config_for("single", env={"MX_RAND_AUGMENT": f"{n},{m}", "MX_IMAGE_SIZE": str(S)})
    aug = A.BatchRandAugment(cfg, _Ctx())
    aug(x.clone(), 0, 0)                                    # allocates table, stats, slab, buffer
    table, stats, slab = aug.table, aug.stats, aug.slab
    key = A.batch_key(0, 0, 0, 0)
    drawn = A.draw_randaug(0, 0, 0, 0, B, S, n, m)[:, 0, 0]
    one = {}                                                # a one-slot table per op, every sample on it
    for op in range(A.NUM_OPS):
        rows = A.draw_randaug(0, 0, 0, 0, 4096, S, 1, m)
        row = rows[rows[:, 0, 0] == op][0]
        one[op] = torch.tensor(np.repeat(row[None], B, 0), device=dev)
    stats1 = torch.zeros(B * K.randaug_stat_row(), dtype=torch.int32, device=dev)
    jt = torch.empty(B, 5, dtype=torch.int32, device=dev)
    K.jitter_draw(jt, jitter_key(0, 0, 0, 0), (0.4, 0.4, 0.4, 0.0))
    jslab = torch.empty(B * K.jitter_bps(B, S, x.dtype, K.AUG_S2D), dtype=torch.float64, device=dev)

    def slot_of(op):
        def fn():
            if op in (12, 13):
                stats1.zero_()
            K.randaug_stats(x, one[op], 0, stats1, slab, K.AUG_S2D)
            K.randaug_apply(x, out, one[op], 0, stats1, slab, K.AUG_S2D)
        return fn

    def draw():
        K.randaug_draw(table, stats, S, key, m)

    runs = {"a": draw, "b": lambda: K.randaug_stats(x, table, 0, stats, slab, K.AUG_S2D),
            "c": lambda: K.randaug_apply(x, out, table, 0, stats, slab, K.AUG_S2D),
            "d": lambda: aug(x, 0, 0)}
    runs.update({f"e{op}": slot_of(op) for op in range(A.NUM_OPS)})
    runs.update({"g": lambda: K.batch_jitter(x, jt, K.AUG_S2D, jslab),
                 "h": lambda: K.batch_mix(x, out, K.AUG_S2D, K.MIX_MIXUP, 0.3)})
    xb = x.numel() * 2
    share = float(np.isin(drawn, (8, 12, 13)).mean())
    nbytes = {"a": B * n * 32, "b": int(xb * share), "c": 2 * xb, "d": None, "g": 3 * xb, "h": 3 * xb}
    names = {"a": f"randaug_draw, n = {n}", "b": f"randaug_stats, slot 0 ({100 * share:.0f} % of the samples take a statistic)",
             "c": "randaug_apply, slot 0 of the drawn table", "d": f"the n = {n} chain: draw + {n} x (stats + apply)",
             "g": "jitter_mean + batch_jitter, b/c/s: reads x twice, writes it", "h": "batch_mix (mixup): reads x twice, writes out"}
    for op in range(A.NUM_OPS):
        names[f"e{op}"] = f"stats + apply, every sample {A.OPS[op]}" + (" (+ a memset of the rows)" if op in (12, 13) else "")
        nbytes[f"e{op}"] = (3 if op in (8, 12, 13) else 2) * xb
    lines = ["# RandAugment: launch and step cost (ResNet-50 shapes)", "",
             f"`tools/randaug_bench.py`: batch {tuple(x.shape)} bf16 ({xb} bytes), n = {n}, m = {m}; "
             f"{slab.numel() // B} partial sums per sample; device events around {args.iters} back-to-back calls, "
             f"{args.rounds} rounds, the variants taking turns inside every round. Ops of slot 0 of the drawn table: "
             + ", ".join(f"{A.OPS[o]} {int((drawn == o).sum())}" for o in range(A.NUM_OPS)) + ".", "",
             "| launch | us / call (median) | min .. max | bytes moved | TB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in runs:
        t = times[k]
        med = statistics.median(t)
        rate = "-" if nbytes[k] is None else f"{nbytes[k] / med / 1e6:.2f}"
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k] or '-'} | {rate} |")
        print(lines[-1], flush=True)

    # ---- end to end: the same trainer, the plain step and the augmenting step alternating
    crit = tr.model.make_criterion()

    def eager_step(i, pre=None):
        xs, ys = tr.gen(torch.arange(B, dtype=torch.int64) + i * B)
        if pre is not None:
            xs = pre(xs, 0, i)
        l = crit(tr.net(xs), ys)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        tr._loss = l.detach()

    step_ms = {"NativeTrainer.step": [], "the same step made of the trainer's eager calls": [],
               f"the eager calls with MX_RAND_AUGMENT={n},{m}": []}
    i = 1
    for r in range(args.step_rounds + 1):
        for name, fn in zip(step_ms, (tr.step, eager_step, lambda i: eager_step(i, aug))):
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
