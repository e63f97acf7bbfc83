"""Cost of the colour jitter on the ResNet-50 shapes (batch: B x 224 px), launch by launch:

  (a) jitter_draw
  (b) jitter_mean, s2d bf16      (c) batch_jitter (apply), s2d bf16, b/c/s on (MX_COLOR_JITTER=0.4)
  (d) the apply with hue on as well (0.4,0.4,0.4,0.1)
  (e) jitter_mean, NCHW f32      (f) the apply, NCHW f32, all four ops
  (g) batch_mix (mixup), s2d bf16     (h) erase_draw + batch_erase, s2d bf16, p = 0.25   -- yardsticks

timed with device events around ``--iters`` back-to-back calls after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round (the spread is printed), and the end-to-end step of
the native bf16 trainer with and without ``MX_COLOR_JITTER=0.4``, alternating. The jitter is in place
and not idempotent: repeated on one batch the colours drift, but the per-pixel work is branch-free
within an op, so the time does not depend on the values. Bytes are what the launch must move: the
mean pass reads every pixel once, the apply reads and writes it (s2d: the whole 16-slot group in
16-bit, 12 of 16 slots in f32). Writes markdown to ``--out``.

    python tools/jitter_bench.py --out profiles/jitter.md
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.erase_bench import _time_alternating  # noqa: E402


class _Ctx:
    rank, engine = 0, "native"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/jitter.md")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.data.synthetic import MEAN, STD
    from pytorch_distributed_amd.erase import batch_key as erase_key
    from pytorch_distributed_amd.jitter import BatchJitter, batch_key
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import ext, native_ops as K
    dev = torch.device("cuda", 0)
    B, S = args.batch, 224
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    tr.step(0)
    torch.cuda.synchronize()

    # ---- the launches alone
    x, _ = tr.gen(torch.arange(B, dtype=torch.int64))
    x = x.clone()
    out = torch.empty_like(x)
    n = torch.randn(B, 3, S, S, device=dev)
    L, st = ext.lib(), ext.stream(dev)
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    tables = {}
    for name, strengths in (("bcs", (0.4, 0.4, 0.4, 0.0)), ("bcsh", (0.4, 0.4, 0.4, 0.1))):
        tables[name] = torch.empty(B, 5, dtype=torch.int32, device=dev)
        K.jitter_draw(tables[name], batch_key(0, 0, 0, 0), strengths)
    boxes = torch.empty(B, 4, dtype=torch.int32, device=dev)
    slabs = {id(t): torch.empty(B * K.jitter_bps(B, S, t.dtype, l), dtype=torch.float64, device=dev)
             for t, l in ((x, K.AUG_S2D), (n, K.AUG_NCHW))}

    def mean_pass(t, layout, table):
        s = slabs[id(t)]
        return lambda: ext.check(L.pda_jitter_mean(t.data_ptr(), table.data_ptr(), s.data_ptr(), s.numel(), B, S,
                                                   ext.dt_of(t), layout, mean, std, 0, st), "jitter_mean")

    def apply(t, layout, table):
        s = slabs[id(t)]
        return lambda: ext.check(L.pda_batch_jitter(t.data_ptr(), table.data_ptr(), s.data_ptr(), s.numel(), 1, B,
                                                    S, ext.dt_of(t), layout, mean, std, 0, st), "batch_jitter")

    def erase():
        K.erase_draw(boxes, S, erase_key(0, 0, 0, 0), 0.25)
        K.batch_erase(x, boxes, K.AUG_S2D)

    runs = {"a": lambda: K.jitter_draw(tables["bcs"], batch_key(0, 0, 0, 0), (0.4, 0.4, 0.4, 0.0)),
            "b": mean_pass(x, K.AUG_S2D, tables["bcs"]), "c": apply(x, K.AUG_S2D, tables["bcs"]),
            "d": apply(x, K.AUG_S2D, tables["bcsh"]),
            "e": mean_pass(n, K.AUG_NCHW, tables["bcsh"]), "f": apply(n, K.AUG_NCHW, tables["bcsh"]),
            "g": lambda: K.batch_mix(x, out, K.AUG_S2D, K.MIX_MIXUP, 0.3), "h": erase}
    xb, nb = x.numel() * 2, n.numel() * 4
    nbytes = {"a": B * 20, "b": xb, "c": 2 * xb, "d": 2 * xb, "e": nb, "f": 2 * nb, "g": 3 * xb, "h": None}
    names = {"a": "jitter_draw", "b": "jitter_mean, s2d bf16", "c": "apply, s2d bf16, b/c/s",
             "d": "apply, s2d bf16, b/c/s/h", "e": "jitter_mean, NCHW f32", "f": "apply, NCHW f32, b/c/s/h",
             "g": "batch_mix (mixup), s2d bf16: reads x twice, writes out", "h": "erase_draw + batch_erase, s2d bf16, p = 0.25"}
    lines = ["# Colour jitter: launch and step cost (ResNet-50 shapes)", "",
             f"`tools/jitter_bench.py`: batch {tuple(x.shape)} bf16 ({xb} bytes) and {tuple(n.shape)} f32 "
             f"({nb} bytes); {slabs[id(x)].numel() // B} / {slabs[id(n)].numel() // B} partial sums per sample; "
             f"device events around {args.iters} back-to-back calls, {args.rounds} rounds, the variants taking "
             f"turns inside every round.", "",
             "| launch | us / call (median) | min .. max | bytes moved | TB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in runs:
        t = times[k]
        med = statistics.median(t)
        rate = "-" if nbytes[k] is None else f"{nbytes[k] / med / 1e6:.2f}"
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k] or '-'} | {rate} |")
        print(lines[-1], flush=True)

    # ---- end to end: the same trainer, the plain step and the jittering step alternating
    cfg = config_for("single", env={"MX_COLOR_JITTER": "0.4", "MX_IMAGE_SIZE": str(S)})
    jitter = BatchJitter(cfg, _Ctx())
    crit = tr.model.make_criterion()

    def eager_step(i, jit=None):
        xs, ys = tr.gen(torch.arange(B, dtype=torch.int64) + i * B)
        if jit is not None:
            xs = jit(xs, 0, i)
        l = crit(tr.net(xs), ys)
        l.backward()
        tr.opt.step()
        tr.opt.zero_grad()
        tr._loss = l.detach()

    step_ms = {"NativeTrainer.step": [], "the same step made of the trainer's eager calls": [],
               "the eager calls with MX_COLOR_JITTER=0.4": []}
    i = 1
    for r in range(args.step_rounds + 1):
        for name, fn in zip(step_ms, (tr.step, eager_step, lambda i: eager_step(i, jitter))):
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
