"""The packed data path on the CPU: the float64 reference of the crop draw (tests/packed_refs.py)
against ``data.folder``'s own transforms, the file format and its refusals, and the wiring."""
import math
import os
import random
import struct

import numpy as np
import pytest
import torch

import packed_refs as P
from pytorch_distributed_amd.data.folder import train_crop_params, val_crop_params, val_transform


# ------------------------------------------------------------------ the draw
def test_hash_matches_the_package_hash():
    from pytorch_distributed_amd.data.synthetic import hash32
    xs = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789, 2654435761]
    assert hash32(torch.tensor(xs, dtype=torch.int64)).tolist() == [P.hash32(x) for x in xs]


def test_uniforms_are_exact_and_in_range():
    ek = P.epoch_key(3, 0, "train", 1)
    us = [P.uniform(ek, k) for k in range(41)]
    assert all(0.0 <= u < 1.0 and (u * 2.0 ** 32).is_integer() for u in us)
    assert len(set(us)) == 41
    # a pure function of (seed, split, epoch, id)
    assert ek == P.epoch_key(3, 0, "train", 1)
    assert len({P.epoch_key(3, 0, "train", 1), P.epoch_key(4, 0, "train", 1), P.epoch_key(3, 1, "train", 1),
                P.epoch_key(3, 0, "val", 1), P.epoch_key(3, 0, "train", 2)}) == 5


def test_fixture_draws_reach_every_branch_and_none_is_fragile():
    sizes = P.fixture_sizes()
    seen = set()
    for seed in P.SEEDS:
        for epoch in P.EPOCHS:
            for k, (W, H) in enumerate(sizes):
                box, flip, attempts, fragile = P.draw_train(W, H, k, seed, epoch)
                assert not fragile, (seed, epoch, k)
                x0, y0, x1, y1 = box
                assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
                if (W, H) == (5, 200):
                    assert attempts == 11 and box == (0, 96, 5, 103)      # w = 5, h = round(5 / 0.75) = 7
                    seen.add("tall")
                elif (W, H) == (200, 5):
                    assert attempts == 11 and box == (96, 0, 103, 5)      # h = 5, w = round(5 * 4/3) = 7
                    seen.add("wide")
                else:
                    seen.add("accepted" if attempts <= 10 else "whole")
                    seen.add("retry" if 1 < attempts <= 10 else "first")
                seen.add(flip)
    assert {"tall", "wide", "accepted", "retry", "first", True, False} <= seen


def test_fragile_flag():
    assert P._near_half(12.5) and P._near_half(12.5 + 5e-7) and P._near_half(0.5 - 5e-7)
    assert not P._near_half(12.5 + 2e-6) and not P._near_half(12.0) and not P._near_half(12.49)


class _Counting(random.Random):
    calls = 0

    def uniform(self, a, b):
        self.calls += 1
        return super().uniform(a, b)


def test_statistics_agree_with_train_crop_params():
    """20000 draws on a 500x375 image against ``train_crop_params`` under ``random.Random(0)``:
    first-attempt acceptance rate, mean area fraction and flip rate, each within three standard
    errors of the difference, computed from the two samples."""
    n, W, H = 20000, 500, 375
    rng = _Counting(0)
    a = np.zeros((n, 3))
    b = np.zeros((n, 3))
    fragile = 0
    for k in range(n):
        before = rng.calls
        (x0, y0, x1, y1), flip = train_crop_params(W, H, rng=rng)
        a[k] = ((rng.calls - before) == 2, (x1 - x0) * (y1 - y0) / (W * H), flip)
        (x0, y0, x1, y1), flip, attempts, fr = P.draw_train(W, H, k, 0, 0)
        b[k] = (attempts == 1, (x1 - x0) * (y1 - y0) / (W * H), flip)
        fragile += fr
    assert fragile <= n // 100
    for c, name in enumerate(("first-attempt acceptance", "area fraction", "flip rate")):
        se = math.sqrt(a[:, c].var(ddof=1) / n + b[:, c].var(ddof=1) / n)
        diff = abs(a[:, c].mean() - b[:, c].mean())
        print(f"{name}: folder {a[:, c].mean():.4f}, packed {b[:, c].mean():.4f}, diff/se {diff / se:.2f}")
        assert diff <= 3 * se, (name, a[:, c].mean(), b[:, c].mean(), se)


def test_train_reference_is_train_crop_params_on_its_own_uniforms():
    """Feed ``train_crop_params`` the reference's uniforms through a stub rng: same box and flip."""
    class Stub:
        def __init__(self, ekey):
            self.ekey, self.attempt = ekey, -1

        def uniform(self, lo, hi):
            if lo == P.SCALE[0]:
                self.attempt += 1
                return lo + (hi - lo) * P.uniform(self.ekey, 4 * self.attempt)
            return lo + (hi - lo) * P.uniform(self.ekey, 4 * self.attempt + 1)

        def randint(self, lo, hi):
            self.k = getattr(self, "k", 1) + 1          # 2: row, 3: column
            return int(P.uniform(self.ekey, 4 * self.attempt + self.k) * (hi + 1))

        def random(self):
            return P.uniform(self.ekey, 40)

    for seed in P.SEEDS:
        for epoch in P.EPOCHS:
            for k, (W, H) in enumerate(P.fixture_sizes() + [(500, 375), (640, 480)]):
                want = train_crop_params(W, H, rng=Stub(P.epoch_key(k, seed, "train", epoch)))
                box, flip, _, _ = P.draw_train(W, H, k, seed, epoch)
                assert (box, flip) == want


def test_val_reference_is_val_crop_params():
    for W, H in P.fixture_sizes() + [(300, 260), (500, 375), (375, 500)]:
        for size, resize in ((16, 18), (64, 73), (224, 256)):
            assert P.draw_val(W, H, size, resize) == val_crop_params(W, H, size, resize)


# ------------------------------------------------------------------ the file format
def test_round_trip(tmp_path):
    from pytorch_distributed_amd.data.packed import PackedImages
    images, labels = P.make_packed(str(tmp_path))
    for split in ("train", "val"):
        pk = PackedImages(str(tmp_path / f"{split}.pack"))
        assert len(pk) == P.N_IMAGES and pk.short_side == 256
        assert pk.classes == [f"c{k}" for k in range(P.N_CLASSES)]
        for k, (img, label) in enumerate(zip(images, labels)):
            assert pk.image(k).shape == img.shape and np.array_equal(pk.image(k), img)
            assert pk.label(k) == label
        assert pk.pixel_bytes == sum(i.size for i in images)
        assert os.path.getsize(pk.path) < 2 ** 20


def test_writer_with_worker_processes_writes_the_same_file(tmp_path):
    from pytorch_distributed_amd.data.packed import write_packed
    P.make_tree(str(tmp_path))
    write_packed(str(tmp_path), "train", str(tmp_path / "a.pack"))
    write_packed(str(tmp_path), "train", str(tmp_path / "b.pack"), workers=2)
    assert (tmp_path / "a.pack").read_bytes() == (tmp_path / "b.pack").read_bytes()


def test_shrink_gives_val_transform_size(tmp_path):
    from PIL import Image
    from pytorch_distributed_amd.data.packed import PackedImages, shrunk_size, write_packed
    rng = np.random.default_rng(1)
    sizes = [(90, 61), (61, 90), (40, 33), (64, 64), (33, 200), (32, 32), (20, 100)]
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for W, H in sizes]
    P.make_tree(str(tmp_path), "train", images=images, labels=[0] * len(images))
    write_packed(str(tmp_path), "train", str(tmp_path / "train.pack"), short_side=32)
    pk = PackedImages(str(tmp_path / "train.pack"))
    for k, ((W, H), img) in enumerate(zip(sizes, images)):
        if min(W, H) > 32:
            seen = {}
            orig = Image.Image.resize

            def spy(self, size, *a, **kw):
                seen["size"] = tuple(size)
                return orig(self, size, *a, **kw)

            Image.Image.resize = spy
            try:
                val_transform(32, 32)(Image.fromarray(img))
            finally:
                Image.Image.resize = orig
            nw, nh = seen["size"]
            assert shrunk_size(W, H, 32) == (nw, nh) and min(nw, nh) == 32
            want = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
        else:
            assert shrunk_size(W, H, 32) == (W, H)          # never enlarged
            want = img
        assert np.array_equal(pk.image(k), want)


def _patched(tmp_path, name, edit):
    """A copy of the fixture file with ``edit(bytearray, header fields)`` applied."""
    from pytorch_distributed_amd.data.packed import _HEADER
    src = tmp_path / "train.pack"
    if not src.exists():
        P.make_tree(str(tmp_path))
        from pytorch_distributed_amd.data.packed import write_packed
        write_packed(str(tmp_path), "train", str(src))
    data = bytearray(src.read_bytes())
    out = edit(data, list(_HEADER.unpack_from(data, 0)))
    dst = tmp_path / name
    dst.write_bytes(bytes(out if out is not None else data))
    return str(dst)


def _set_record(data, hdr, k, col, value):
    struct.pack_into("<q", data, hdr[6] + (k * 4 + col) * 8, value)


def _get_record(data, hdr, k, col):
    return struct.unpack_from("<q", data, hdr[6] + (k * 4 + col) * 8)[0]


def test_bad_files_are_refused(tmp_path):
    from pytorch_distributed_amd.data.packed import PackedImages
    from pytorch_distributed_amd.ops.native_ops import AUG_MAX_SIDE
    PackedImages(_patched(tmp_path, "ok.pack", lambda d, h: None))
    with pytest.raises(ValueError, match="magic"):
        PackedImages(_patched(tmp_path, "magic.pack", lambda d, h: d.__setitem__(slice(0, 4), b"JUNK")))
    with pytest.raises(ValueError, match="version"):
        PackedImages(_patched(tmp_path, "version.pack", lambda d, h: struct.pack_into("<Q", d, 8, 99)))
    with pytest.raises(ValueError, match="truncated"):
        PackedImages(_patched(tmp_path, "short.pack", lambda d, h: d[:-100]))
    with pytest.raises(ValueError, match="header"):
        PackedImages(_patched(tmp_path, "tiny.pack", lambda d, h: d[:40]))
    with pytest.raises(ValueError, match=r"record 4: bytes .* outside the pixel section"):
        PackedImages(_patched(tmp_path, "off.pack", lambda d, h: _set_record(d, h, 4, 0, h[8] - 10)))
    with pytest.raises(ValueError, match=r"record 2: bytes"):
        PackedImages(_patched(tmp_path, "neg.pack", lambda d, h: _set_record(d, h, 2, 0, -1)))
    with pytest.raises(ValueError, match=r"record 6: its bytes overlap"):
        PackedImages(_patched(tmp_path, "overlap.pack", lambda d, h: _set_record(
            d, h, 6, 0, _get_record(d, h, 5, 0) + 1)))
    with pytest.raises(ValueError, match=rf"record 3: size {AUG_MAX_SIDE + 1}x"):
        PackedImages(_patched(tmp_path, "big.pack", lambda d, h: _set_record(d, h, 3, 2, AUG_MAX_SIDE + 1)))
    with pytest.raises(ValueError, match=r"record 0: size"):
        PackedImages(_patched(tmp_path, "zero.pack", lambda d, h: _set_record(d, h, 0, 1, 0)))
    with pytest.raises(ValueError, match=r"record 10: label 3 outside"):
        PackedImages(_patched(tmp_path, "label.pack", lambda d, h: _set_record(d, h, 10, 3, 3)))


# ------------------------------------------------------------------ wiring
def test_config_and_cpu_device_refusal(tmp_path):
    from pytorch_distributed_amd import trainer
    from pytorch_distributed_amd.config import config_for
    from pytorch_distributed_amd.data.packed import PackedImages, PackedStore
    cfg = config_for("single", env={"MX_DATA": f"packed:{tmp_path}", "MX_PACK_RESIDENT": "host"})
    assert cfg.data == f"packed:{tmp_path}" and cfg.pack_resident == "host"
    assert config_for("single", env={}).pack_resident == "auto"
    with pytest.raises(ValueError, match="MX_PACK_RESIDENT"):
        config_for("single", env={"MX_PACK_RESIDENT": "disk"})
    with pytest.raises(ValueError, match="packed:<dir>"):
        config_for("single", env={"MX_DATA": "packed:"})
    P.make_packed(str(tmp_path))
    ctx = trainer.Context(cfg=cfg, device=torch.device("cpu"), dtype=torch.float32, engine="torch")
    with pytest.raises(ValueError, match="MX_DATA=packed"):
        trainer._make_loaders(cfg, ctx, torch.nn.Identity(), 4)
    with pytest.raises(ValueError, match="GPU"):
        PackedStore(PackedImages(str(tmp_path / "train.pack")), "cpu")
    with pytest.raises(ValueError, match="'packed:<dir>'"):
        trainer._make_loaders(cfg.replace(data="ffrecord:/x"), ctx, torch.nn.Identity(), 4)


def test_aug_draw_checks_its_arguments_on_the_host():
    """Refusals that need no GPU: they are raised before anything touches the device."""
    from pytorch_distributed_amd.ops import native_ops as K
    index = torch.zeros(4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        K.aug_draw(torch.arange(3), index, 4, 0, "train", 0, K.AUG_TRAIN, 16)
    with pytest.raises(ValueError, match="host int64"):
        K.aug_draw(torch.arange(3, dtype=torch.int32), index, 4, 0, "train", 0, K.AUG_TRAIN, 16)
    with pytest.raises(ValueError, match="GPU"):
        K.aug_resize_dev(torch.zeros(8, dtype=torch.uint8), index, index.double(),
                         torch.zeros(4, 3, 16, 16), K.AUG_NCHW)
