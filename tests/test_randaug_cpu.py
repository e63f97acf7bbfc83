"""RandAugment without a GPU: randaug_torch against the float64 reference of tests/randaug_refs.py,
the host draw, the configuration, and a two-step trainer run with the variable set."""
import numpy as np
import pytest
import torch

import randaug_refs as R
from pytorch_distributed_amd import randaug as A
from pytorch_distributed_amd.config import config_for

# randaug_torch evaluates the reference's formulas in float32: the bound of tests/test_randaug_gpu.py
TOL32 = 8 * 1.102e-6


@pytest.mark.parametrize("layout,B,S", [(R.S2D, 3, 6), (R.NCHW, 2, 5)], ids=["s2d", "nchw"])
def test_randaug_torch_against_the_reference(layout, B, S):
    x0 = R.randaug_input(layout, torch.float32, B, S)
    for k in range(len(R.ROWS)):
        ops, par, co = R.hand_rows(k, B, S)
        x = A.randaug_torch(x0.clone(), A.pack_table(ops, par, co), layout)
        want, skip, eq_tie = R.chain_ref(R.images(x0, layout), ops, par, co, torch.float32)
        assert not eq_tie and skip.mean() <= 0.02
        err = np.abs(R.images(x, layout) - want)
        geo = np.isin(ops[:, 0], R.GEO)
        assert (err[geo][~skip[geo]] == 0).all() and (err[~skip] <= TOL32).all(), (k, float(err[~skip].max()))
        if layout == R.S2D:
            assert bool((x[..., 12:] == R.PAD).all())


def test_draw_randaug_ops_parameters_and_purity():
    t = A.draw_randaug(3, 1, 2, 9, 257, 224, 4, 30)
    ops, par, co = A.table_parts(t)
    assert t.shape == (257, 4, 8) and set(ops.ravel().tolist()) == set(range(14))
    assert set(par[(ops >= 6) & (ops <= 9)].tolist()) == {np.float32(1.9), np.float32(0.1)}
    assert set(par[ops == 10].tolist()) == {0xF0} and set(par[ops == 11].tolist()) == {0.0}
    assert set(co[ops == 1][:, 1].tolist()) == {np.float32(0.3), np.float32(-0.3)}
    assert set(co[ops == 3][:, 2].tolist()) == {101.0, -101.0}                    # trunc(150 / 331 * 224)
    rot = co[ops == 5]
    assert np.allclose(rot[:, 0], np.cos(np.pi / 6)) and set(np.sign(rot[:, 3]).tolist()) == {1.0, -1.0}
    assert not t[~np.isin(ops, R.GEO)][:, 2:].any() and np.array_equal(A.pack_table(ops, par, co), t)
    assert np.array_equal(t[:5, :2], A.draw_randaug(3, 1, 2, 9, 5, 224, 2, 30))   # position and slot, not B or n
    for other in ((4, 1, 2, 9), (3, 0, 2, 9), (3, 1, 3, 9), (3, 1, 2, 8)):
        assert not np.array_equal(t, A.draw_randaug(*other, 257, 224, 4, 30))


def test_config_parses_n_m_and_refuses_the_rest():
    from pytorch_distributed_amd import trainer
    assert config_for("single", env={}).rand_augment == (0, 0)
    assert config_for("ddp", env={"MX_RAND_AUGMENT": "2,9"}).rand_augment == (2, 9)
    assert config_for("single", env={}, argv=["--rand-augment", "4,30"]).rand_augment == (4, 30)
    for bad in ("a", "2", "2,9,1", "5,9", "-1,9", "2,31", "2,-1", "2.0,9", "2,,9", "2,9.5"):
        with pytest.raises(ValueError, match="MX_RAND_AUGMENT"):
            config_for("single", env={"MX_RAND_AUGMENT": bad})
    ctx = trainer.Context(cfg=config_for("single", env={"MX_RAND_AUGMENT": "0,9"}), device=torch.device("cpu"),
                          dtype=torch.float32, engine="torch")
    assert trainer._batch_randaug(ctx) is None and ctx.extra == {}


def test_cpu_trainer_runs_two_steps_with_the_variable_set(tmp_path, capsys, monkeypatch):
    from pytorch_distributed_amd import trainer
    calls, real = [], A.randaug_torch
    monkeypatch.setattr(A, "randaug_torch", lambda x, t, l: calls.append(t.shape) or real(x, t, l))
    trainer.run(config_for("single", env={
        "MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_STEPS_PER_EPOCH": "2", "MX_VAL_STEPS": "1", "MX_BATCH": "4",
        "MX_IMAGE_SIZE": "32", "MX_DEVICE": "cpu", "MX_LOG_EVERY": "0", "MX_WORKERS": "0", "MX_NUM_CLASSES": "10",
        "MX_RAND_AUGMENT": "2,9", "MX_SAVE_PATH": str(tmp_path)}), "single")
    capsys.readouterr()
    assert calls == [(4, 2, 8)] * 2                      # training steps only, never validation
