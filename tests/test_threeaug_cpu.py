"""3-Augment off the GPU: the MX_THREE_AUGMENT variable and its flag, nothing built while it is unset,
three_aug_torch against the float64 reference of tests/threeaug_refs.py, and the shared inputs'
distance from the solarize threshold."""
import numpy as np
import pytest
import torch

import threeaug_refs as R
from pytorch_distributed_amd import threeaug as T
from pytorch_distributed_amd.config import config_for, parse_cli

CASES = ([(R.S2D, B, S, r) for B, S, r in R.SHAPES] + [(R.NCHW, B, S, r) for B, S, r in R.SHAPES + R.NCHW_ONLY])


def test_config_variable_and_flag():
    assert config_for("single", env={}).three_augment is False
    assert config_for("single", env={"MX_THREE_AUGMENT": "0"}).three_augment is False
    assert config_for("single", env={"MX_THREE_AUGMENT": "1"}).three_augment is True
    for bad in ("2", "true", "-1", "0.5"):
        with pytest.raises(ValueError, match="MX_THREE_AUGMENT"):
            config_for("single", env={"MX_THREE_AUGMENT": bad})
    assert parse_cli(["--three-augment", "1"]) == {"MX_THREE_AUGMENT": "1"}


def test_nothing_is_built_while_the_variable_is_unset():
    from types import SimpleNamespace
    from pytorch_distributed_amd import trainer
    ctx = SimpleNamespace(cfg=config_for("single", env={}), extra={}, rank=0, engine="torch")
    assert trainer._batch_three_aug(ctx) is None and ctx.extra == {}
    ctx.cfg = config_for("single", env={"MX_THREE_AUGMENT": "1", "MX_IMAGE_SIZE": "32"})
    assert trainer._batch_three_aug(ctx) is ctx.extra["three_aug"] is trainer._batch_three_aug(ctx)
    with pytest.raises(ValueError, match="image_size"):
        T.BatchThreeAugment(config_for("single", env={"MX_IMAGE_SIZE": "10"}), ctx)


@pytest.mark.parametrize("layout,B,S,r", CASES)
def test_three_aug_torch_against_the_reference(layout, B, S, r):
    """float32 torch against the float64 reference: the bound is that of the GPU test's f32 cases."""
    x0 = R.levels_input(layout, torch.float32, B, S)
    for k in range(R.KINDS):
        table = R.hand_table(k, B, r)
        got = T.three_aug_torch(x0.clone(), table, layout).double().numpy()
        want = R.three_aug_ref(x0.double().numpy(), table, layout)
        assert np.abs(got - want).max() <= 8 * 1.034e-6, k
        if layout == R.S2D:
            assert (got[..., 12:] == R.PAD).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_inputs_keep_off_the_solarize_threshold(dtype):
    """float32 and float64 un-normalisation put every element on the same side of 128/255, so no
    element is ever excluded from a comparison."""
    for layout, B, S, _ in CASES:
        if layout == R.NCHW and dtype != torch.float32:
            continue
        x = R.pixels(R.levels_input(layout, dtype, B, S).double().numpy(), layout)
        x64 = np.clip(x * R.STD + R.MEAN, 0, 1)
        x32 = np.clip(x.astype(np.float32) * R.STD.astype(np.float32) + R.MEAN.astype(np.float32), 0, 1)
        assert (np.abs(x64 - R.THR) >= 1e-4).all()
        assert ((x64 >= R.THR) == (x32 >= np.float32(R.THR))).all()
        assert (x64 >= R.THR).any() and (x64 < R.THR).any() and (x64 == 0).any() and (x64 == 1).any()


def test_draw_is_keyed_and_packs_normalised_weights():
    a = T.draw_three_aug(3, 1, 2, 5, 300)
    ops, radii, w = T.table_parts(a)
    assert set(ops) == {0, 1, 2} and (radii == 11).all()
    assert np.allclose(w[:, 0].astype(np.float64) + 2 * w[:, 1:].astype(np.float64).sum(1), 1, atol=1e-6)
    assert (T.table_parts(T.three_aug_table([2], [1.0], 3))[2][0, 4:] == 0).all()
    for other in ((4, 1, 2, 5), (3, 0, 2, 5), (3, 1, 3, 5), (3, 1, 2, 6)):
        assert not np.array_equal(a, T.draw_three_aug(*other, 300))
