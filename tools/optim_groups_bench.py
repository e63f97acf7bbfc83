"""Cost of the segmented optimizer on a ResNet-50 flat buffer (bf16 shadow), each variant alone:

  (a) sgd_flat over the whole buffer (the default step's optimizer launch)
  (b) sgd_seg, one group of every parameter
  (c) sgd_seg, no_bn_decay groups
  (d) (c) + LARS: seg_norms + sgd_seg

timed with device events around ``--iters`` back-to-back launches after a warm-up, ``--rounds`` times
each (the spread is printed), and the end-to-end step time of the native bf16 trainer with the default
and with the grouped optimizer, taken alternately. Bytes are what the update must move: p, g and
the momentum read, p and the momentum written (4 B each) and the 2-B shadow written; seg_norms reads
p and g of the trust segments once more. Writes markdown to ``--out``.

    python tools/optim_groups_bench.py --out profiles/optim_groups.md
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters, rounds, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)      # us per call
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/optim_groups.md")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=3)
    args = ap.parse_args()
    from pytorch_distributed_amd.models.native import NativeTrainer
    from pytorch_distributed_amd.ops import native_ops as K
    from pytorch_distributed_amd.optim import build_param_groups
    dev = torch.device("cuda", 0)
    tr = NativeTrainer("resnet50", args.batch, torch.bfloat16, dev)
    m = tr.model
    tr.step(0)          # a real gradient in the flat buffer
    torch.cuda.synchronize()
    base = m.flat_params.data_ptr()
    params = list(m.parameters())
    segs = [((p.data_ptr() - base) // 4, p.numel()) for p in params]
    n_seg = sum(s for _, s in segs)
    h = dict(lr=0.0, momentum=0.9, weight_decay=1e-4)      # lr 0: the timed launches leave p alone
    mats = [p.dim() >= 2 for p in params]
    variants = {
        "b": [dict(h) for _ in params],
        "c": [dict(h) if d else dict(h, weight_decay=0.0) for d in mats],
        "d": [dict(h, lars=0.001) if d else dict(h, weight_decay=0.0) for d in mats],
    }
    tabs = {k: K.seg_tables(segs, v, dev)[0] for k, v in variants.items()}
    mom = torch.zeros_like(m.flat_params)
    p, g, sh = m.flat_params, m.flat_grad, m.flat_shadow

    def seg(k):
        def fn():
            if tabs[k].any_trust:
                K.seg_norms(p, g, tabs[k])
            K.sgd_seg(p, g, mom, sh, tabs[k], True)
        return fn

    runs = {"a": lambda: K.sgd_flat(p, g, mom, sh, 0.0, 0.9, 1e-4, True)}
    runs.update({k: seg(k) for k in tabs})
    n_trust = sum(s for (_, s), d in zip(segs, mats) if d)
    nbytes = {"a": m.numel * 22, "b": n_seg * 22, "c": n_seg * 22, "d": n_seg * 22 + n_trust * 8}
    names = {"a": "sgd_flat, whole buffer", "b": "sgd_seg, one group", "c": "sgd_seg, no_bn_decay groups",
             "d": "seg_norms + sgd_seg, no_bn_decay + LARS"}
    lines = ["# Segmented optimizer: kernel and step cost (ResNet-50, bf16 shadow)", "",
             f"`tools/optim_groups_bench.py`: {m.numel} flat elements, {n_seg} in {len(segs)} segments, "
             f"{tabs['b'].nblocks} blocks of at most {K.SEG_CHUNK} elements; device events around "
             f"{args.iters} back-to-back launches, {args.rounds} rounds, each variant alone.", "",
             "| variant | us / call (median) | min .. max | bytes moved | GB/s |", "|---|---|---|---|---|"]
    for k in "abcd":
        t = _time(runs[k], args.iters, args.rounds)
        med = statistics.median(t)
        lines.append(f"| ({k}) {names[k]} | {med:.1f} | {min(t):.1f} .. {max(t):.1f} | {nbytes[k]} | "
                     f"{nbytes[k] / med / 1e3:.0f} |")
        print(lines[-1], flush=True)
    # end to end: the same trainer, its optimizer swapped between rounds
    plain = tr.opt
    grouped = m.make_optimizer(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True,
                               param_groups=build_param_groups(m, 1e-4, no_bn_decay=True, lars=0.001))
    step_ms = {"default optimizer": [], "no_bn_decay + Nesterov + LARS": []}
    i = 1
    for r in range(args.step_rounds + 1):
        for name, opt in zip(step_ms, (plain, grouped)):
            tr.opt = opt
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                tr.step(i)
                i += 1
            b.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms both up
                step_ms[name].append(a.elapsed_time(b) / args.steps)
    lines += ["", f"End to end: native bf16 training step, batch {args.batch}, {args.steps} steps per "
              f"round, the two optimizers alternating, {args.step_rounds} rounds.", "",
              "| optimizer | ms / step (median) | min .. max |", "|---|---|---|"]
    for name, t in step_ms.items():
        lines.append(f"| {name} | {statistics.median(t):.3f} | {min(t):.3f} .. {max(t):.3f} |")
        print(lines[-1], flush=True)
    assert tr.last_loss() == tr.last_loss(), "non-finite loss"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
