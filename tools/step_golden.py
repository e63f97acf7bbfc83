"""Bit-exact record of three eager native training steps at the smallest shapes the engine takes
(tests/golden/native_step.json, checked by tests/test_native_step_golden_gpu.py): every kernel of
a step is deterministic, so a host-side change of the schedule must reproduce these integers.

    python tools/step_golden.py > tests/golden/native_step.json      (GPU)

Record the fixture from the commit BEFORE the change under test, twice in fresh processes, and
commit it only if both outputs are identical.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE = 64
STEPS = 3
# (arch, per-step batch, dtype name): bf16 default path, BasicBlock nets, the fp16 AMP path
CASES = (("resnet50", 16, "bfloat16"), ("resnet18", 8, "bfloat16"), ("resnet50", 16, "float16"))


def case_id(arch: str, batch: int, dtype: str) -> str:
    return f"{arch}-b{batch}-{dtype}"


def make_trainer(arch: str, batch: int, dtype: str):
    from pytorch_distributed_amd.models.native import NativeTrainer
    return NativeTrainer(arch, batch, getattr(torch, dtype), torch.device("cuda", 0),
                         image_size=IMAGE)


def step_record(arch: str, batch: int, dtype: str) -> dict:
    """Checksums of (master weights, momentum) and of the BN running statistics, and the losses,
    after STEPS eager steps of a fresh NativeTrainer."""
    from pytorch_distributed_amd.bench_step import tensor_checksum
    t = make_trainer(arch, batch, dtype)
    losses = []
    for i in range(STEPS):
        t.step(i)
        losses.append(t.last_loss())
    torch.cuda.synchronize()
    return {"state": tensor_checksum([t.model.flat_params, t.opt.flat_mom]).tolist(),
            "buffers": tensor_checksum([t.model.flat_buffers]).tolist(),
            "losses": losses}


def main() -> None:
    rec = {"torch": torch.__version__, "image_size": IMAGE, "steps": STEPS,
           "cases": {case_id(*c): step_record(*c) for c in CASES}}
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
