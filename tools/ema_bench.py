"""Cost of the weight EMA (csrc/ema.hip, ema.py) on the ResNet-50 flat buffers:

  (a) LERP : NativeEMA.update() -- one launch over (parameters, BN statistics) + the counter copy
  (b) SWAP : one exchange as swapped() enters or leaves (parameters with their bf16 shadow,
             statistics and counters; without the stem repack)
  (c) COPY : the launch that initialises the average

timed with device events around ``--iters`` back-to-back launches after a warm-up, ``--rounds`` rounds
with the variants taking turns inside every round, and the native bf16 training step at ``--batch``
with the EMA update off and on, alternating on one trainer. Bytes are what the operation must move:
LERP reads p and e and writes e; SWAP reads and writes both and writes the 16-bit shadow.

``--parent DIR`` (a built checkout of the parent commit) adds the default step of that checkout and
of this one measured the same way, as fresh processes taking turns (``--procs`` each): the spread of
the parent's runs is what "the step is unchanged with MX_EMA off" is judged against.
``--step-only`` is that child: it prints one JSON line and needs nothing of the EMA.

    python tools/ema_bench.py --out profiles/ema.md [--parent /path/to/parent/checkout]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _steps(fns, steps, rounds):
    """ms / step of each step function, the functions alternating, one warm-up round first."""
    out = {k: [] for k in fns}
    i = 1
    for r in range(rounds + 1):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn(i)
                i += 1
            b.record()
            torch.cuda.synchronize()
            if r:
                out[name].append(a.elapsed_time(b) / steps)
    return out


def _child(repo, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--step-only", "--repo", repo, "--batch",
           str(args.batch), "--steps", str(args.steps), "--step-rounds", str(args.step_rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ema.md")
    ap.add_argument("--repo", default=HERE)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    from pytorch_distributed_amd.models.native import NativeTrainer
    dev = torch.device("cuda", 0)
    B = args.batch
    tr = NativeTrainer("resnet50", B, torch.bfloat16, dev)
    m = tr.model
    tr.step(0)
    torch.cuda.synchronize()
    if args.step_only:
        t = _steps({"default": tr.step}, args.steps, args.step_rounds)["default"]
        assert tr.last_loss() == tr.last_loss(), "non-finite loss"
        print(json.dumps({"repo": os.path.abspath(args.repo), "ms": t}), flush=True)
        return

    from pytorch_distributed_amd.ema import NativeEMA
    from pytorch_distributed_amd.ops import native_ops as K
    ema = NativeEMA(m, 0.9999)
    runs = {"a": ema.update,
            "b": lambda: K.ema_update(ema._whole, K.EMA_SWAP),
            "c": lambda: K.ema_update(ema._whole, K.EMA_COPY)}
    n_p, n_b = m.flat_params.numel(), m.flat_bufstore.numel() // 4
    nbytes = {"a": 12 * (n_p + m.flat_buffers.numel()), "b": 16 * (n_p + n_b) + 2 * n_p, "c": 8 * (n_p + n_b)}
    names = {"a": "LERP: update() (parameters + statistics, counters copied)",
             "b": "SWAP: parameters + bf16 shadow, statistics, counters",
             "c": "COPY: parameters, statistics, counters"}
    lines = ["# Weight EMA: kernel and step cost (ResNet-50 flat buffers, bf16)", "",
             f"`tools/ema_bench.py`: {n_p} f32 parameters, {m.flat_buffers.numel()} f32 BN statistics, "
             f"{m.flat_nbt.numel()} int64 counters; device events around {args.iters} back-to-back calls, "
             f"{args.rounds} rounds, the variants taking turns inside every round. The buffers (about 0.3 GB "
             f"per LERP) fit the 256 MiB Infinity Cache only in part, so back-to-back calls see some of "
             f"their reads cached; inside a training step they come from HBM.", "",
             "| variant | us / call (median) | min .. max | bytes moved | GB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in "abc":
        t = times[k]
        med = statistics.median(t)
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k]} | "
                     f"{nbytes[k] / med / 1e3:.0f} |")
        print(lines[-1], flush=True)
    K.ema_update(ema._whole, K.EMA_COPY)       # (the timing loop left the exchange in any state)

    def ema_step(i):
        tr.step(i)
        ema.update()

    step_ms = _steps({"MX_EMA off": tr.step, "MX_EMA on (every step)": ema_step}, args.steps,
                     args.step_rounds)
    lines += ["", f"End to end: native bf16 training step, batch {B}, {args.steps} steps per round, the two "
              f"steps alternating on one trainer, {args.step_rounds} rounds after a warm-up round.", "",
              "| step | ms / step (median) | min .. max |", "|---|---|---|"]
    for name, t in step_ms.items():
        lines.append(f"| {name} | {statistics.median(t):.3f} | {min(t):.3f} .. {max(t):.3f} |")
        print(lines[-1], flush=True)
    assert tr.last_loss() == tr.last_loss(), "non-finite loss"

    if args.parent:
        del tr, m, ema
        torch.cuda.empty_cache()
        per = {"parent commit": [], "this tree, MX_EMA off": []}
        repos = {"parent commit": args.parent, "this tree, MX_EMA off": HERE}
        for i in range(args.procs):         # (the order flips every turn: a drift hits both alike)
            for name in (list(repos) if i % 2 == 0 else list(repos)[::-1]):
                per[name].append(_child(repos[name], args))
        lines += ["", f"The default step (no EMA object) of the parent commit and of this tree: {args.procs} "
                  f"fresh processes each, taking turns (the order flipping every turn), every process "
                  f"{args.step_rounds} rounds of {args.steps} steps after a warm-up round; the median of each "
                  f"process, and over all of its rounds the minimum and maximum.", "",
                  "| checkout | ms / step, per-process medians | min .. max over all rounds |", "|---|---|---|"]
        for name, runs_ in per.items():
            meds = ", ".join(f"{statistics.median(t):.3f}" for t in runs_)
            flat = [v for t in runs_ for v in t]
            lines.append(f"| {name} | {meds} | {min(flat):.3f} .. {max(flat):.3f} |")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
