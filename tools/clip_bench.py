"""Cost of global-norm gradient clipping (csrc/clip.hip, NativeSGD(clip_grad_norm=...)) on ResNet-50:

  (a) grad_clip : the clip launch alone over the optimizer's block table of the flat gradient
  (b) sgd_flat  : the fused SGD over the same buffers in the same run -- the streaming rate the clip
                  kernel, which only reads the gradient, is set against

timed with device events around ``--iters`` back-to-back launches after a warm-up, ``--rounds`` rounds
with the two taking turns inside every round, and the native bf16 training step at ``--batch`` with
clipping off, off again (two identical runs: their difference is the spread the on-cost is judged
against) and on, the three alternating on one trainer. Bytes are what the launch must move: the clip
reads g; the SGD reads p, g and the momentum and writes p, the momentum and the 16-bit shadow.

``--parent DIR`` (a built checkout of the parent commit) adds the default step of that checkout and
of this one measured the same way, as fresh processes taking turns (``--procs`` each, the order
flipping every turn): the spread of the parent's runs is what "the step is unchanged with
MX_CLIP_GRAD_NORM unset" is judged against. ``--step-only`` is that child: it prints one JSON line
and needs nothing of the clip.

    python tools/clip_bench.py --out profiles/clip.md [--parent /path/to/parent/checkout]
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
    ap.add_argument("--out", default="profiles/clip.md")
    ap.add_argument("--repo", default=HERE)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--max-norm", type=float, default=1.0)
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

    from pytorch_distributed_amd.ops import native_ops as K
    off = tr.opt
    on = m.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4, clip_grad_norm=args.max_norm)
    on.load_state_dict(off.state_dict())        # the same momentum: the two continue one run
    t = on._clip_tables
    n = m.flat_params.numel()
    owned = sum(b.count for b in t.blk_host)
    # the kernels alone work on copies, so the timing loops leave the trainer's state alone
    p, g, buf, sh = (x.clone() for x in (m.flat_params, m.flat_grad, off.flat_mom, m.flat_shadow))
    g.normal_(0.0, 1e-3)
    slab, cnt, out = (torch.zeros_like(x) for x in (on._clip_slab, on._clip_cnt, on._clip_out))
    runs = {"a": lambda: K.grad_clip(g, t, args.max_norm, slab, cnt, out),
            "b": lambda: K.sgd_flat(p, g, buf, sh, 0.0, 0.9, 1e-4, True)}
    nbytes = {"a": 4 * owned, "b": 4 * 5 * n + 2 * n}
    names = {"a": f"grad_clip: {t.nblocks} blocks, reads g", "b": "sgd_flat: reads p, g, momentum; "
             "writes p, momentum, bf16 shadow"}
    lines = ["# Gradient clipping: kernel and step cost (ResNet-50 flat gradient, bf16)", "",
             f"`tools/clip_bench.py`: {n} f32 elements in the flat buffers, {owned} of them owned by the "
             f"optimizer's {len(t.seg_host)} tensors; device events around {args.iters} back-to-back "
             f"calls, {args.rounds} rounds, the two taking turns inside every round. The gradient "
             f"({4 * owned / 1e6:.0f} MB) fits the 256 MiB Infinity Cache, so back-to-back clip launches "
             f"re-read it from there; inside a training step it was just written by the backward pass.", "",
             "| launch | us / call (median) | min .. max | bytes moved | GB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    for k in "ab":
        ts = times[k]
        med = statistics.median(ts)
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(ts):.1f} .. {max(ts):.1f} | {nbytes[k]} | "
                     f"{nbytes[k] / med / 1e3:.0f} |")
        print(lines[-1], flush=True)
    assert int(cnt.item()) == 0 and out[0].item() > 0
    del p, g, buf, sh

    def step_with(opt):
        def fn(i):
            tr.opt = opt
            tr.step(i)
        return fn

    step_ms = _steps({"clip off (A)": step_with(off), "clip on": step_with(on),
                      "clip off (B)": step_with(off)}, args.steps, args.step_rounds)
    lines += ["", f"End to end: native bf16 training step, batch {B}, {args.steps} steps per round, three "
              f"steps alternating on one trainer (two optimizers over the same model: clipping off, "
              f"on with max_norm {args.max_norm}, and off once more -- A and B are identical runs), "
              f"{args.step_rounds} rounds after a warm-up round. Last pre-clip norm: "
              f"{on.grad_norm.item():.4f}.", "",
              "| step | ms / step (median) | min .. max |", "|---|---|---|"]
    for name, ts in step_ms.items():
        lines.append(f"| {name} | {statistics.median(ts):.3f} | {min(ts):.3f} .. {max(ts):.3f} |")
        print(lines[-1], flush=True)
    assert tr.last_loss() == tr.last_loss(), "non-finite loss"

    if args.parent:
        del tr, m, on, off
        torch.cuda.empty_cache()
        per = {"parent commit": [], "this tree, clipping off": []}
        repos = {"parent commit": args.parent, "this tree, clipping off": HERE}
        for i in range(args.procs):         # (the order flips every turn: a drift hits both alike)
            for name in (list(repos) if i % 2 == 0 else list(repos)[::-1]):
                per[name].append(_child(repos[name], args))
        lines += ["", f"The default step (no clip_grad_norm) of the parent commit and of this tree: "
                  f"{args.procs} fresh processes each, taking turns (the order flipping every turn), every "
                  f"process {args.step_rounds} rounds of {args.steps} steps after a warm-up round; the "
                  f"median of each process, and over all of its rounds the minimum and maximum.", "",
                  "| checkout | ms / step, per-process medians | min .. max over all rounds |", "|---|---|---|"]
        for name, runs_ in per.items():
            meds = ", ".join(f"{statistics.median(ts):.3f}" for ts in runs_)
            flat = [v for ts in runs_ for v in ts]
            lines.append(f"| {name} | {meds} | {min(flat):.3f} .. {max(flat):.3f} |")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
