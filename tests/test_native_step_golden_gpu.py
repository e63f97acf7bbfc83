"""Three eager native training steps reproduce tests/golden/native_step.json bit for bit.

Every kernel of a step is deterministic (no float atomics, fixed-order slab reductions), so the
forward / backward schedule in models/native.py can be reorganised on the host with proof that
nothing changed: the fixture was recorded (tools/step_golden.py, twice, identical) from the commit
before the saved state of the schedule was given types, and the comparison has no tolerance."""
import json
import os

import pytest
import torch

from tools.step_golden import CASES, case_id, make_trainer, step_record

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_step.json")


def _golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=[case_id(*c) for c in CASES])
def test_three_steps_match_the_recorded_bits(case):
    gold = _golden()
    want = gold["cases"][case_id(*case)]
    got = step_record(*case)
    print(f"{case_id(*case)}: torch {torch.__version__} (recorded with {gold['torch']})\n"
          f"  got  {got}\n  want {want}")
    assert got["state"] == want["state"]
    assert got["buffers"] == want["buffers"]
    assert got["losses"] == want["losses"]


def test_golden_case_takes_the_default_schedules_fused_paths(monkeypatch):
    """The resnet50 bf16 case is not a fallback-only run: at 64 px / batch 16 the tail BN backward
    is folded into conv3, the forward leaves the decomposed weight gradient's Gram terms, and block
    tails are formed by the next block's conv1."""
    from pytorch_distributed_amd.ops import native_ops as K
    arch, batch, dtype = CASES[0]
    assert (arch, dtype) == ("resnet50", "bfloat16")
    t = make_trainer(arch, batch, dtype)
    m = t.model
    tails = []
    conv_fwd = K.conv_fwd

    def counting(*a, **kw):
        tails.append(kw.get("tail") is not None)
        return conv_fwd(*a, **kw)
    monkeypatch.setattr(K, "conv_fwd", counting)
    x, _ = t.gen(torch.arange(batch))
    m(x)
    torch.cuda.synchronize()
    assert any(m._tail_fold_ok(b, batch) for b in m.blocks)
    assert any(rec.gram is not None for rec in m._fwd_ctx.blocks)
    assert any(tails)
