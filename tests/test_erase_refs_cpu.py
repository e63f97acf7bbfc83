"""The random-erasing reference (tests/erase_refs.py) against the package's host mirror
(``erase.draw_erase``, ``erase.erase_torch``), and the structure of the draw itself."""
import numpy as np
import pytest
import torch

import erase_refs as R
from pytorch_distributed_amd import erase


def test_draw_erase_equals_the_reference_and_the_grid_is_not_fragile():
    """Seeds (0, 5) x ranks (0, 1) x epochs (0, 1, 2) x steps (0, 1, 7) x S in (4, 10, 32, 224),
    B = 64, p in (0, 0.25, 1): the same table, and no root within 1e-6 of k + 0.5 anywhere (so a
    device exp a few ulp off cannot change an integer: tests/test_erase_gpu.py compares bit for bit)."""
    fragile = []
    for seed, rank, epoch, step, S in R.grid():
        for p in R.PROBS:
            boxes, accepted, frag = R.grid_draw(seed, rank, epoch, step, S, p)
            got = erase.draw_erase(seed, rank, epoch, step, R.BATCH, S, p)
            assert got.dtype == np.int32 and got.shape == (R.BATCH, 4)
            assert np.array_equal(got, boxes), (seed, rank, epoch, step, S, p)
            fragile += [(seed, rank, epoch, step, S, p, b) for b, f in enumerate(frag) if f]
    assert not fragile, fragile


def test_key_chain():
    assert erase.batch_key(3, 1, 2, 7) == R.batch_key(3, 1, 2, 7)
    assert R.batch_key(0, 0, 0, 0) == R.hash32(R.hash32(R.hash32(R.hash32(0x455241))))
    keys = {R.batch_key(s, r, e, t) for s in range(3) for r in range(3) for e in range(3) for t in range(3)}
    assert len(keys) == 81


def test_structure_of_the_draw():
    """Every box lies inside [0, S]^2 with h < S and w < S; p = 0 erases nothing; p = 1 erases every
    sample that has an acceptable attempt, and only those; p = 0.25 erases a subset of p = 1's
    samples with the same boxes (the gate is one uniform, the attempts do not depend on p)."""
    taken = 0
    for seed, rank, epoch, step, S in R.grid():
        b0, a0, _ = R.grid_draw(seed, rank, epoch, step, S, 0.0)
        assert not b0.any() and set(a0) == {-1}
        b1, a1, _ = R.grid_draw(seed, rank, epoch, step, S, 1.0)
        bq, aq, _ = R.grid_draw(seed, rank, epoch, step, S, 0.25)
        for b in range(R.BATCH):
            y1, y2, x1, x2 = b1[b].tolist()
            if a1[b] < 0:
                assert (y1, y2, x1, x2) == (0, 0, 0, 0)
                assert S == 4, "only a 4-px image can refuse ten default attempts"
            else:
                assert 0 <= y1 <= y2 <= S and 0 <= x1 <= x2 <= S and y2 - y1 < S and x2 - x1 < S
                taken += 1
            if aq[b] >= 0:
                assert aq[b] == a1[b] and np.array_equal(bq[b], b1[b])
            else:
                assert not bq[b].any()
        n1, nq = sum(a >= 0 for a in a1), sum(a >= 0 for a in aq)
        assert nq <= n1
        if S >= 10:
            assert n1 == R.BATCH                      # (1 - P(accept))^10 is nothing at these sizes
            assert 3 <= nq <= 33                      # Binomial(64, 0.25): 16 +- 5 sigma
    assert taken > 0.9 * len(R.grid()) * R.BATCH


@pytest.mark.parametrize("S", [4, 10, 32, 224])
def test_strict_inequality_boundary(S):
    """scale (1, 1), ratio (1, 1): h = w = S in all ten attempts, refused (the comparison is strict),
    nothing is erased. Bounds that give h = w = S - 1: every sample takes attempt 0 at an offset in
    {0, 1}, and both offsets occur."""
    scale, ratio = R.REFUSED
    boxes, accepted, frag = R.grid_draw(0, 0, 0, 0, S, 1.0, R.BATCH, scale, ratio)
    assert not boxes.any() and set(accepted) == {-1} and not any(frag)
    assert not erase.draw_erase(0, 0, 0, 0, R.BATCH, S, 1.0, scale, ratio).any()
    scale, ratio = R.almost(S)
    boxes, accepted, frag = R.grid_draw(0, 0, 0, 0, S, 1.0, R.BATCH, scale, ratio)
    assert set(accepted) == {0} and not any(frag)
    assert np.array_equal(boxes[:, 1] - boxes[:, 0], np.full(R.BATCH, S - 1))
    assert np.array_equal(boxes[:, 3] - boxes[:, 2], np.full(R.BATCH, S - 1))
    assert set(boxes[:, 0].tolist()) == {0, 1} and set(boxes[:, 2].tolist()) == {0, 1}
    assert np.array_equal(erase.draw_erase(0, 0, 0, 0, R.BATCH, S, 1.0, scale, ratio), boxes)


def test_every_key_changes_the_table():
    base = erase.draw_erase(0, 0, 0, 0, R.BATCH, 32, 1.0)
    assert np.array_equal(base, erase.draw_erase(0, 0, 0, 0, R.BATCH, 32, 1.0))
    for args in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        assert not np.array_equal(base, erase.draw_erase(*args, R.BATCH, 32, 1.0)), args
    # a sample's draw depends on its position, not on the batch size
    assert np.array_equal(base[:5], erase.draw_erase(0, 0, 0, 0, 5, 32, 1.0))


def test_draw_erase_refusals():
    for kw in (dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(scale=(0.5, 0.2)),
               dict(ratio=(3.0, 0.3)), dict(scale=(-0.1, 0.3)), dict(scale=(0.1, float("inf"))),
               dict(ratio=(0.0, 1.0)), dict(ratio=(0.3, float("nan"))), dict(B=0), dict(S=0)):
        a = dict(B=4, S=8, p=0.5, scale=R.SCALE, ratio=R.RATIO)
        a.update(kw)
        with pytest.raises(ValueError):
            erase.draw_erase(0, 0, 0, 0, a["B"], a["S"], a["p"], a["scale"], a["ratio"])


CASES = ([(R.S2D, dt, S) for dt in (torch.float32, torch.bfloat16, torch.float16) for S in (4, 10, 32)]
         + [(R.NCHW, torch.float32, S) for S in (6, 10, 32)])
IDS = [f"{'s2d' if l == R.S2D else 'nchw'}-{str(dt).split('.')[1]}-S{S}" for l, dt, S in CASES]


@pytest.mark.parametrize("layout,dtype,S", CASES, ids=IDS)
def test_erase_torch_equals_the_reference_bit_for_bit(layout, dtype, S):
    """The eight hand-written boxes of erase_refs.box_kinds on the planted input (NaN payloads, -0,
    +-max inside and outside the boxes, non-zero s2d padding), then a drawn table: integer compare."""
    x = R.planted_input(layout, dtype, S)
    for boxes in (list(R.box_kinds(S).values()), erase.draw_erase(0, 0, 0, 3, 8, S, 1.0)):
        ref = R.erased(x, boxes, layout)
        got = x.clone()
        erase.erase_torch(got, np.asarray(boxes, dtype=np.int32), layout)
        assert torch.equal(R.bits(got), R.bits(ref))
        assert not torch.equal(R.bits(got), R.bits(x))
    # the reference itself: an erased pixel is +0.0 in three channels, the rest keeps its bits
    ref = R.erased(x, list(R.box_kinds(S).values()), layout)
    assert torch.equal(R.bits(ref)[0], R.bits(x)[0])                   # "empty"
    whole = R.bits(ref)[1]
    if layout == R.S2D:
        assert int(torch.count_nonzero(whole[..., :12])) == 0
        assert torch.equal(whole[..., 12:], R.bits(x)[1][..., 12:])
    else:
        assert int(torch.count_nonzero(whole)) == 0
    changed = (R.bits(ref) != R.bits(x))
    assert int(changed[2].sum()) <= 3                                  # "odd pixel": 3 elements
