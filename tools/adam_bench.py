"""Cost of the AdamW / LAMB kernels (csrc/adam.hip, NativeAdamW) on the ResNet-50 flat buffers:

  (a) adamw_seg                 : the fused AdamW step
  (b) lamb_moments + lamb_apply : the two LAMB phases (trust ratio on the dim >= 2 tensors)
  (c) adam_tick                 : the one-block launch ahead of either
  (d) sgd_flat, (e) sgd_seg     : the SGD kernels over the same buffers in the same run

timed with device events around ``--iters`` back-to-back launches after a warm-up, ``--rounds`` rounds
with the launches taking turns inside every round, each with the bytes it must move; then the native
bf16 training step at ``--batch`` with SGD (twice: two identical runs, whose difference is the spread
the others are judged against), AdamW and LAMB, alternating on one trainer.

``--parent DIR`` (a built checkout of the parent commit) adds the default step of that checkout and
of this one, as fresh processes taking turns (``--procs`` each, the order flipping every turn): the
children are ``tools/clip_bench.py --step-only``, which need nothing of the optimizers here.

    python tools/adam_bench.py --out profiles/adam.md [--parent /path/to/parent/checkout]
"""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from clip_bench import _child, _steps, _time_alternating  # noqa: E402  (the same loops and child)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/adam.md")
    ap.add_argument("--repo", default=HERE)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--procs", type=int, default=3)
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

    from pytorch_distributed_amd.ops import native_ops as K
    from pytorch_distributed_amd.optim import build_param_groups
    sgd = tr.opt
    kw = dict(lr=1e-3, weight_decay=1e-2)
    adamw = m.make_optimizer(opt="adamw", param_groups=build_param_groups(m, 1e-2), **kw)
    lamb = m.make_optimizer(opt="lamb", param_groups=build_param_groups(m, 1e-2, lamb=True), **kw)
    seg = m.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    ta, tl, ts = adamw._tables, lamb._tables, seg._tables
    n = m.flat_params.numel()
    owned = sum(b.count for b in ta.seg.blk_host)
    # the kernels alone work on copies, so the timing loops leave the trainer's state alone
    p, g, sh = (x.clone() for x in (m.flat_params, m.flat_grad, m.flat_shadow))
    g.normal_(0.0, 1e-3)
    e1, e2, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)

    def lamb_step():
        K.lamb_moments(p, g, e1, e2, tl)
        K.lamb_apply(p, e1, e2, sh, tl)

    K.adam_tick(ta), K.adam_tick(tl)      # (the update kernels read a written bias table)
    runs = {"a": lambda: K.adamw_seg(p, g, e1, e2, sh, ta), "b": lamb_step,
            "c": lambda: K.adam_tick(ta),
            "d": lambda: K.sgd_flat(p, g, buf, sh, 0.0, 0.9, 1e-4, True),
            "e": lambda: K.sgd_seg(p, g, buf, sh, ts, True)}
    nbytes = {"a": 30 * owned, "b": 42 * owned, "c": 4 * (12 + 2) * ta.nseg, "d": 22 * n, "e": 22 * owned}
    names = {"a": "adamw_seg: reads p, g, m, v; writes p, m, v, bf16 shadow (30 B/element)",
             "b": "lamb_moments + lamb_apply: A reads p, g, m, v, writes m, v; B reads p, m, v, "
                  "writes p, shadow (42 B/element)",
             "c": f"adam_tick: one block, {ta.nseg} segments",
             "d": "sgd_flat: reads p, g, momentum; writes p, momentum, shadow (22 B/element)",
             "e": "sgd_seg (Nesterov): the same bytes over the segment table"}
    lines = ["# AdamW / LAMB: kernel and step cost (ResNet-50 flat buffers, bf16)", "",
             f"`tools/adam_bench.py`: {n} f32 elements in the flat buffers, {owned} of them owned by the "
             f"optimizer's {ta.nseg} tensors in {ta.nblocks} blocks; device events around {args.iters} "
             f"back-to-back calls, {args.rounds} rounds, the launches taking turns inside every round.", "",
             "| launch | us / call (median) | min .. max | bytes moved | GB/s |", "|---|---|---|---|---|"]
    times = _time_alternating(runs, args.iters, args.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in "abcde":
        lines.append(f"| ({k}) {names[k]} | {med[k]:.1f} | {min(times[k]):.1f} .. {max(times[k]):.1f} | "
                     f"{nbytes[k]} | {nbytes[k] / med[k] / 1e3:.0f} |")
        print(lines[-1], flush=True)
    lines += ["", f"adamw_seg / sgd_flat = {med['a'] / med['d']:.3f} in time against "
              f"{30 / 22 * owned / n:.3f} in bytes (30/22 x owned / all elements); (lamb_moments + "
              f"lamb_apply) / sgd_flat = {med['b'] / med['d']:.3f} against {42 / 22 * owned / n:.3f} "
              f"(42/22 scaled alike)."]
    print(lines[-1], flush=True)
    assert bool(p.isfinite().all()) and int(ta.step.item()) > 0
    del p, g, sh, e1, e2, buf

    def step_with(opt):
        def fn(i):
            tr.opt = opt
            tr.step(i)
        return fn

    step_ms = _steps({"sgd (A)": step_with(sgd), "adamw": step_with(adamw), "lamb": step_with(lamb),
                      "sgd (B)": step_with(sgd)}, args.steps, args.step_rounds)
    lines += ["", f"End to end: native bf16 training step, batch {B}, {args.steps} steps per round, four "
              f"optimizers over the same model alternating on one trainer (SGD A and B are identical "
              f"runs), {args.step_rounds} rounds after a warm-up round.", "",
              "| step | ms / step (median) | min .. max |", "|---|---|---|"]
    for name, t in step_ms.items():
        lines.append(f"| {name} | {statistics.median(t):.3f} | {min(t):.3f} .. {max(t):.3f} |")
        print(lines[-1], flush=True)
    assert tr.last_loss() == tr.last_loss(), "non-finite loss"

    if args.parent:
        del tr, m, sgd, adamw, lamb, seg
        torch.cuda.empty_cache()
        repos = {"parent commit": args.parent, "this tree, nothing set": HERE}
        per = {k: [] for k in repos}
        for i in range(args.procs):         # (the order flips every turn: a drift hits both alike)
            for name in (list(repos) if i % 2 == 0 else list(repos)[::-1]):
                per[name].append(_child(repos[name], args))
        lines += ["", f"The default step (MX_OPT unset: SGD) of the parent commit and of this tree: "
                  f"{args.procs} fresh processes each, taking turns (the order flipping every turn), every "
                  f"process {args.step_rounds} rounds of {args.steps} steps after a warm-up round; the "
                  f"median of each process, and over all of its rounds the minimum and maximum.", "",
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
