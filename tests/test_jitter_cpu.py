"""Colour jitter without a GPU: jitter_torch against the float64 reference of tests/jitter_refs.py,
the host draw, the configuration, and the erase draw after the shared-helper move."""
import numpy as np
import pytest
import torch

import jitter_refs as R
from pytorch_distributed_amd import jitter as J
from pytorch_distributed_amd.config import config_for, parse_cli

# jitter_torch evaluates the reference's formulas in float32: the bound of tests/test_jitter_gpu.py
TOL32 = 8 * 4.367e-6


@pytest.mark.parametrize("layout,B,S", [(R.S2D, 3, 6), (R.NCHW, 2, 5)], ids=["s2d", "nchw"])
def test_jitter_torch_against_the_reference(layout, B, S):
    x0 = R.levels_input(layout, torch.float32, B, S)
    for k in range(len(R.ROWS)):
        factors, orders = R.hand_table(k, B)
        x = x0.clone()
        J.jitter_torch(x, J.jitter_table(factors, orders), layout)
        want = R.jitter_ref(x0.double().numpy(), factors, orders, layout)
        assert np.abs(x.double().numpy() - want).max() <= TOL32, k
        if layout == R.S2D:
            assert bool((x[..., 12:] == R.PAD).all())


def test_draw_jitter_ranges_permutations_and_purity():
    st = (0.4, 0.3, 0.2, 0.1)
    t = J.draw_jitter(3, 1, 2, 9, 257, st)
    f, o = J.table_parts(t)
    for k, s in enumerate(st[:3]):
        assert (f[:, k] >= np.float32(1 - s)).all() and (f[:, k] <= np.float32(1 + s)).all()
    assert (np.abs(f[:, 3]) <= np.float32(0.1)).all() and f.std(0).min() > 0.01
    assert (np.sort(o, 1) == np.arange(4)).all() and len({tuple(r) for r in o.tolist()}) == 24
    assert np.array_equal(t, J.draw_jitter(3, 1, 2, 9, 257, st))
    assert np.array_equal(t[:5], J.draw_jitter(3, 1, 2, 9, 5, st))               # position, not B
    for other in ((4, 1, 2, 9), (3, 0, 2, 9), (3, 1, 3, 9), (3, 1, 2, 8)):
        assert not np.array_equal(t, J.draw_jitter(*other, 257, st))
    f0, o0 = J.table_parts(J.draw_jitter(3, 1, 2, 9, 257, (0.4, 0, 0.2, 0)))
    assert np.array_equal(np.where(np.isin(o, (1, 3)), -1, o), o0)                # same places, marked
    assert (f0[:, 1] == 1).all() and (f0[:, 3] == 0).all() and np.array_equal(f0[:, 0], f[:, 0])
    assert np.array_equal(J.jitter_table(f, o), t)


def test_config_parses_the_three_forms_and_refuses_the_rest():
    assert config_for("single", env={}).color_jitter == (0.0, 0.0, 0.0, 0.0)
    assert config_for("single", env={"MX_COLOR_JITTER": "0.4"}).color_jitter == (0.4, 0.4, 0.4, 0.0)
    assert config_for("ddp", env={"MX_COLOR_JITTER": "0.4,0.3,0.2"}).color_jitter == (0.4, 0.3, 0.2, 0.0)
    assert config_for("single", env={}, argv=["--color-jitter", "0.4,0,0.2,0.1"]).color_jitter == (0.4, 0.0, 0.2, 0.1)
    assert set(parse_cli(["--color-jitter", "0.4"])) == {"MX_COLOR_JITTER"}
    for bad in ("a", "0.4,0.4", "1,2,3,4,5", "-0.1", "0.4,0.4,0.4,0.6", "0.4,0.4,0.4,-0.1", "nan", "inf", "0.1,,0.2"):
        with pytest.raises(ValueError, match="MX_COLOR_JITTER"):
            config_for("single", env={"MX_COLOR_JITTER": bad})


def test_off_by_default_and_the_erase_draw_is_unchanged():
    from pytorch_distributed_amd import trainer
    from pytorch_distributed_amd.erase import batch_key, draw_erase
    ctx = trainer.Context(cfg=config_for("single", env={"MX_COLOR_JITTER": "0"}), device=torch.device("cpu"),
                          dtype=torch.float32, engine="torch")
    assert trainer._batch_jitter(ctx) is None and ctx.extra == {}
    # the values of the commit before the helpers were shared
    assert batch_key(5, 1, 2, 3) == ERASE_KEY and J.batch_key(5, 1, 2, 3) != ERASE_KEY
    assert draw_erase(5, 1, 2, 3, 8, 32, 1.0)[6].tolist() == ERASE_ROW


ERASE_KEY, ERASE_ROW = 1593393458, [2, 14, 9, 22]
