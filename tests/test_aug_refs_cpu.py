"""The yardstick of the GPU augmentation tests, checked on the CPU: the float64 reference
(tests/aug_refs.py) against PIL, the crop-parameter functions against the PIL transforms they were
split out of, the raw-batch collate, and the host-side refusals of ``aug_resize``."""
import random
import zlib

import numpy as np
import pytest
import torch

import aug_refs as R
from pytorch_distributed_amd.data.synthetic import STD

# |reference - PIL| in levels: 0.5 for PIL's rounding of the horizontal pass to uint8 + 0.5 for its
# final rounding + its 22-bit fixed-point coefficients (<= ksize * 2^-23 * 255 per pass)
PIL_TOL = 1.01


def _image(rng, W, H, binary=False):
    if binary:
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _pil_resize(img, box, S):
    from PIL import Image
    return np.asarray(Image.fromarray(img).resize((S, S), Image.BILINEAR, box=box), dtype=np.float64)


def _named_cases():
    """(name, W, H, integer box, S, binary)"""
    return [
        ("upscale_5x7_box", 48, 40, (11, 9, 16, 16), 32, False),
        ("upscale_whole_5x7", 5, 7, (0, 0, 5, 7), 32, True),
        ("down_8x", 263, 257, (3, 1, 259, 257), 32, False),
        ("down_9x_binary", 300, 290, (0, 0, 300, 290), 32, True),
        ("down_9x_224", 2000, 1500, (0, 0, 2000, 1500), 224, False),
        ("left_border", 48, 40, (0, 5, 20, 30), 32, False),
        ("top_border", 48, 40, (7, 0, 40, 22), 32, False),
        ("right_border", 48, 40, (30, 5, 48, 30), 32, True),
        ("bottom_border", 48, 40, (7, 20, 40, 40), 32, False),
        ("whole", 64, 64, (0, 0, 64, 64), 32, False),
        ("one_pixel_wide", 300, 10, (150, 0, 151, 10), 32, False),
        ("one_pixel_high", 10, 300, (0, 150, 10, 151), 32, True),
    ]


@pytest.mark.parametrize("case", _named_cases(), ids=lambda c: c[0])
def test_reference_matches_pil_named(case):
    _, W, H, box, S, binary = case
    img = _image(np.random.default_rng(zlib.crc32(case[0].encode())), W, H, binary)
    err = np.abs(R.resample(img, box, S) - _pil_resize(img, box, S)).max()
    assert err <= PIL_TOL, err


def test_reference_matches_pil_random():
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in range(120):
        W, H = (int(v) for v in rng.integers(1, 160, 2))
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        x1, y1 = int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))
        S = int(rng.choice([8, 32, 50]))
        img = _image(rng, W, H, binary=n % 3 == 0)
        err = np.abs(R.resample(img, (x0, y0, x1, y1), S) - _pil_resize(img, (x0, y0, x1, y1), S)).max()
        worst = max(worst, err)
        assert err <= PIL_TOL, (W, H, (x0, y0, x1, y1), S, err)
    assert worst > 0.4    # the comparison is not vacuous: PIL's roundings show


def test_rows_of_the_filter_sum_to_one_and_stay_inside():
    for lo, hi, n, S in [(0, 5, 5, 32), (2.25, 7.75, 9, 32), (0, 2000, 2000, 224), (150, 151, 300, 32)]:
        K, b = R.coeffs(lo, hi, n, S)
        assert np.allclose(K.sum(1), 1.0, atol=1e-14)
        assert (b[:, 0] >= 0).all() and (b[:, 1] <= n).all() and (b[:, 0] < b[:, 1]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 1]) >= 0).all()   # monotone taps


def test_s2d_layout_matches_the_definition():
    x = np.arange(2 * 3 * 4 * 4, dtype=np.float64).reshape(2, 3, 4, 4)
    s = R.s2d_from_nchw(x)
    assert s.shape == (2, 2, 2, 16) and (s[..., 12:] == 0).all()
    for y in range(4):
        for xx in range(4):
            for c in range(3):
                assert s[1, y // 2, xx // 2, 3 * (2 * (y & 1) + (xx & 1)) + c] == x[1, c, y, xx]


# ------------------------------------------------------------------ crop parameters vs the transforms
def _norm_tol():
    # 1.01 levels in normalised units + the f32 rounding of the CPU path's own arithmetic
    return (PIL_TOL / (255.0 * np.asarray(STD)) + 1e-6).reshape(3, 1, 1)


@pytest.mark.parametrize("size", [(48, 40), (300, 10), (10, 300), (263, 257)], ids=str)
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_train_params_reproduce_train_transform(size, seed):
    from PIL import Image
    from pytorch_distributed_amd.data.folder import train_crop_params, train_transform
    W, H = size
    img = _image(np.random.default_rng(seed), W, H)
    S = 32
    rng_a, rng_b = random.Random(seed), random.Random(seed)
    got = train_transform(S, rng=rng_a)(Image.fromarray(img)).numpy().astype(np.float64)
    box, flip = train_crop_params(W, H, (0.08, 1.0), (3 / 4, 4 / 3), rng_b)
    assert rng_a.random() == rng_b.random()     # the same number of draws, in the same order
    ref = R.transform(img, box, S, flip)
    assert (np.abs(got - ref) <= _norm_tol()).all(), np.abs(got - ref).max()


def test_train_params_fallback_is_hit():
    """300x10 never fits a ratio in [3/4, 4/3] at scale >= 0.08 ... most seeds: the 10-attempt
    fallback (center crop at the clamped ratio) must be among the seeds the parity test uses."""
    from pytorch_distributed_amd.data.folder import train_crop_params
    fallback = 0
    for seed in range(5):
        box, _ = train_crop_params(300, 10, (0.08, 1.0), (3 / 4, 4 / 3), random.Random(seed))
        fallback += box == (143, 0, 156, 10)     # h = H = 10, w = round(10 * 4/3) = 13, centred
    assert fallback >= 1


@pytest.mark.parametrize("size", [(48, 40), (40, 48), (500, 375), (263, 257), (64, 64)], ids=str)
@pytest.mark.parametrize("S,resize", [(32, 36), (32, 37), (224, 256)])
def test_val_params_reproduce_val_transform(size, S, resize):
    from PIL import Image
    from pytorch_distributed_amd.data.folder import val_crop_params, val_transform
    W, H = size
    img = _image(np.random.default_rng(W * 1000 + H), W, H)
    got = val_transform(S, resize)(Image.fromarray(img)).numpy().astype(np.float64)
    ref = R.transform(img, val_crop_params(W, H, S, resize), S, False)
    assert (np.abs(got - ref) <= _norm_tol()).all(), np.abs(got - ref).max()


# ------------------------------------------------------------------ collate
def test_collate_round_trip_mixed_sizes():
    from pytorch_distributed_amd.data.folder import collate_raw, unpack_raw
    rng = np.random.default_rng(3)
    sizes = [(5, 7), (48, 41), (1, 1), (33, 3)]       # odd byte counts -> odd offsets
    imgs = [torch.from_numpy(_image(rng, W, H)) for W, H in sizes]
    params = [((0.5, 0.25, W - 0.5, H), bool(i & 1)) for i, (W, H) in enumerate(sizes)]
    packed, ti, tf, labels = collate_raw([(im, 10 + i, p) for i, (im, p) in enumerate(zip(imgs, params))])
    assert packed.dtype == torch.uint8 and packed.numel() == sum(W * H * 3 for W, H in sizes)
    assert ti.dtype == torch.int64 and tf.dtype == torch.float64 and labels.dtype == torch.int64
    assert labels.tolist() == [10, 11, 12, 13]
    assert ti[:, 0].tolist() == [0, 105, 105 + 5904, 105 + 5904 + 3] and ti[1, 0] % 2 == 1
    assert ti[:, 1:3].tolist() == [[H, W] for W, H in sizes] and ti[:, 3].tolist() == [0, 1, 0, 1]
    assert tf.tolist() == [list(p[0]) for p in params]
    for a, b in zip(unpack_raw(packed, ti), imgs):
        assert torch.equal(a, b)


def test_raw_dataset_items(tmp_path):
    from test_folder_data_cpu import _make_tree
    from PIL import Image
    from pytorch_distributed_amd.data.folder import ImageFolder, train_crop_params, train_params
    _make_tree(str(tmp_path))
    ds = ImageFolder(str(tmp_path), "train", raw_params=train_params(rng=random.Random(5)))
    img, label, (box, flip) = ds[5]
    path = ds.samples[5][0]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (40, 48, 3) and label == 1
    assert torch.equal(img, torch.from_numpy(np.array(Image.open(path).convert("RGB"))))
    assert (box, flip) == train_crop_params(48, 40, rng=random.Random(5))


# ------------------------------------------------------------------ wrapper validation (no kernel library)
def _valid(S=32, layout=0, dtype=torch.bfloat16):
    img = np.zeros((40, 48, 3), dtype=np.uint8)
    packed, ti, tf = R.pack([img, img], [(0, 0, 48, 40), (1.5, 2.5, 40.25, 33)], [False, True], gaps=[3, 5])
    out = torch.empty((2, S // 2, S // 2, 16), dtype=dtype) if layout == 0 else torch.empty(2, 3, S, S)
    return packed, ti, tf, out, layout


def test_aug_check_accepts_a_valid_call():
    from pytorch_distributed_amd.ops import native_ops as K
    assert K.aug_check(*_valid()) == (2, 32)
    assert K.aug_check(*_valid(layout=1)) == (2, 32)


def _break(name):
    packed, ti, tf, out, layout = _valid()
    if name == "negative_offset":
        ti[0, 0] = -1
    elif name == "past_the_end":
        ti[1, 0] = packed.numel() - 48 * 40 * 3 + 1
    elif name == "zero_height":
        ti[0, 1] = 0
    elif name == "width_too_large":
        ti[0, 2] = 32769
    elif name == "x0_negative":
        tf[0, 0] = -0.5
    elif name == "x1_past_width":
        tf[0, 2] = 48.5
    elif name == "empty_x":
        tf[0, 0] = tf[0, 2]
    elif name == "y1_past_height":
        tf[1, 3] = 40.01
    elif name == "y_reversed":
        tf[1, 1], tf[1, 3] = 30.0, 20.0
    elif name == "nan_box":
        tf[0, 1] = float("nan")
    elif name == "inf_box":
        tf[0, 2] = float("inf")
    elif name == "odd_size":
        out, layout = torch.empty(2, 3, 31, 31), 1
    elif name == "wrong_batch":
        out = torch.empty(3, 16, 16, 16, dtype=torch.bfloat16)
    elif name == "wrong_shape":
        out = torch.empty(2, 16, 15, 16, dtype=torch.bfloat16)
    elif name == "wrong_channels":
        out = torch.empty(2, 16, 16, 12, dtype=torch.bfloat16)
    elif name == "nchw_not_f32":
        out, layout = torch.empty(2, 3, 32, 32, dtype=torch.bfloat16), 1
    elif name == "s2d_dtype":
        out = torch.empty(2, 16, 16, 16, dtype=torch.float64)
    elif name == "bad_layout":
        layout = 2
    elif name == "out_device":
        out = torch.empty(2, 16, 16, 16, dtype=torch.bfloat16, device="meta")
    elif name == "table_on_device":
        ti = ti.to("meta")
    elif name == "table_dtype":
        tf = tf.float()
    elif name == "table_rows":
        tf = tf[:1].contiguous()
    elif name == "packed_dtype":
        packed = packed.to(torch.int8)
    return packed, ti, tf, out, layout


@pytest.mark.parametrize("name", [
    "negative_offset", "past_the_end", "zero_height", "width_too_large", "x0_negative",
    "x1_past_width", "empty_x", "y1_past_height", "y_reversed", "nan_box", "inf_box", "odd_size",
    "wrong_batch", "wrong_shape", "wrong_channels", "nchw_not_f32", "s2d_dtype", "bad_layout",
    "out_device", "table_on_device", "table_dtype", "table_rows", "packed_dtype"])
def test_aug_check_refuses(name):
    from pytorch_distributed_amd.ops import native_ops as K
    with pytest.raises(ValueError):
        K.aug_check(*_break(name))


def test_aug_resize_refuses_before_loading_the_library(monkeypatch):
    """A bad table raises from the host check; the kernel library is never asked for."""
    from pytorch_distributed_amd.ops import ext, native_ops as K

    def boom(*a, **k):
        raise AssertionError("the kernel library was loaded")
    monkeypatch.setattr(ext, "lib", boom)
    with pytest.raises(ValueError):
        K.aug_resize(*_break("past_the_end"))
    with pytest.raises(ValueError):       # a valid call on CPU tensors: refused, not emulated
        K.aug_resize(*_valid())


# ------------------------------------------------------------------ MX_AUG
def test_mx_aug_config():
    from pytorch_distributed_amd.config import config_for
    assert config_for("single", env={}).aug == "cpu"
    assert config_for("single", env={"MX_AUG": "gpu"}).aug == "gpu"
    assert config_for("single", env={}, argv=["--aug", "gpu"]).aug == "gpu"
    with pytest.raises(ValueError):
        config_for("single", env={"MX_AUG": "dali"})


def test_gpu_aug_on_a_cpu_device_raises(tmp_path):
    from test_folder_data_cpu import _make_tree
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.data.folder import ImageFolder, train_params
    from pytorch_distributed_amd.trainer import Context, _make_folder_loaders
    _make_tree(str(tmp_path), classes=1, per=1)
    ds = ImageFolder(str(tmp_path), "train", raw_params=train_params())
    for device in (None, "cpu", torch.device("cpu")):
        with pytest.raises(ValueError, match="MX_AUG=gpu"):
            ds.loader(2, num_workers=0, device=device, image_size=32)
    cfg = config_for("single", env={"MX_AUG": "gpu", "MX_DATA": f"folder:{tmp_path}", "MX_IMAGE_SIZE": "32"})
    ctx = Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")
    with pytest.raises(ValueError, match="MX_AUG=gpu"):
        _make_folder_loaders(cfg, ctx, 2)
    # the default keeps the CPU path on a CPU device
    tl, _, _ = _make_folder_loaders(cfg.replace(aug="cpu"), ctx, 2)
    assert next(iter(tl))[0].shape == (1, 3, 32, 32)
