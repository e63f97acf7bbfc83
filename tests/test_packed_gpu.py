"""The packed data path on the GPU: the crop-draw kernel (csrc/augment.hip ``aug_draw_kernel``,
``K.aug_draw``) against the float64 reference of tests/packed_refs.py, and the resident store,
loader and entrypoint built on it.

Draw: train boxes and flips are integers and must be EQUAL on every sample the reference does not
mark fragile (tests/packed_refs.py; test_packed_refs_cpu.py asserts these seeds and epochs have
none, so nothing is left out here); val boxes are float64 quotients of exact integers, evaluated with
the same IEEE operations (the file is built without fma contraction), so they must be bit-equal.

Pixels: the loader's batches against tests/aug_refs.py applied to the reference's boxes, under the
bound of tests/test_aug_gpu.py (half an ulp of the stored dtype + the f32 accumulation term).

Val against the CPU pipeline: an image stored at ``short_side`` = the Resize size has an integral val
box at scale 1, so the filter is the identity and only the normalisation differs:
``(a/255 - mean)/std`` in f32 (three roundings of values <= 2.7/std-scaled, each <= 2^-24 relative
of a magnitude <= ~4.4 before the division: ~1e-6) against one f32 fma with 1/(255 std) and -mean/std
rounded to f32 (<= (|R a| + |b| + |out|) 2^-24 ~ 5e-7); 2e-6 absolute covers their sum for
|out| <= 2.7.
"""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import aug_refs as R
import packed_refs as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# two batches of B = 7 that cover all 11 records, out of order, with repeats across batches
BATCHES = ([3, 0, 10, 7, 5, 9, 1], [2, 4, 6, 8, 3, 0, 10])


def _K():
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _resize(S):
    return int(round(S * 256 / 224))


@pytest.fixture(scope="module")
def packed_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("packed")
    images, labels = P.make_packed(str(root))
    return str(root), images, labels


@pytest.fixture(scope="module")
def store(packed_dir):
    from pytorch_distributed_amd.data.packed import PackedImages
    return PackedImages(os.path.join(packed_dir[0], "train.pack")).to_device(_dev(), "device")


def _loader(store, split="train", S=16, layout="nchw", dtype=torch.float32, seed=0, batch=P.BATCH, **kw):
    from pytorch_distributed_amd.data.packed import PackedLoader
    return PackedLoader(store, split, batch, dtype=dtype, layout=layout, image_size=S, seed=seed, **kw)


def _ref_rows(ids, images, labels, seed, epoch, offsets):
    ti, tf = [], []
    for i in ids:
        H, W, _ = images[i].shape
        box, flip, _, fragile = P.draw_train(W, H, i, seed, epoch)
        assert not fragile
        ti.append([offsets[i], H, W, int(flip)])
        tf.append([float(v) for v in box])
    return ti, tf, [labels[i] for i in ids]


# ------------------------------------------------------------------ draw
@pytest.mark.parametrize("S", [16, 64])
def test_draw_matches_reference(store, packed_dir, S):
    K = _K()
    _, images, labels = packed_dir
    offsets = store.images.index[:, 0].tolist()
    n = len(images)
    for seed in P.SEEDS:
        for epoch in P.EPOCHS:
            for ids in BATCHES:
                ti, tf, lab = K.aug_draw(torch.tensor(ids), store.index_dev, n, seed, "train", epoch,
                                         K.AUG_TRAIN, S)
                wi, wf, wl = _ref_rows(ids, images, labels, seed, epoch, offsets)
                assert ti.tolist() == wi and lab.tolist() == wl, (seed, epoch, ids)
                assert tf.tolist() == wf, (seed, epoch, ids)          # integer-valued float64
    for ids in BATCHES:
        ti, tf, lab = K.aug_draw(torch.tensor(ids), store.index_dev, n, 0, "val", 0, K.AUG_VAL, S, _resize(S))
        want = [list(P.draw_val(images[i].shape[1], images[i].shape[0], S, _resize(S))) for i in ids]
        got = tf.cpu().numpy()
        assert got.tobytes() == np.asarray(want, dtype=np.float64).tobytes(), (got, want)   # bit-equal
        assert ti.tolist() == [[offsets[i], images[i].shape[0], images[i].shape[1], 0] for i in ids]
        assert lab.tolist() == [labels[i] for i in ids]


def test_draw_is_independent_of_batch_position_and_size(store):
    K = _K()
    n = len(store.images)
    ids = BATCHES[0]
    ti, tf, lab = (t.cpu() for t in K.aug_draw(torch.tensor(ids), store.index_dev, n, 5, "train", 2,
                                                K.AUG_TRAIN, 16))
    rows = {i: (ti[k].tolist(), tf[k].tolist(), int(lab[k])) for k, i in enumerate(ids)}
    for sub in (ids[::-1][:3], ids[::-1][3:6], ids[6:]):
        ti2, tf2, lab2 = (t.cpu() for t in K.aug_draw(torch.tensor(sub), store.index_dev, n, 5, "train", 2,
                                                       K.AUG_TRAIN, 16))
        for k, i in enumerate(sub):
            assert (ti2[k].tolist(), tf2[k].tolist(), int(lab2[k])) == rows[i]
    # another epoch, seed or split draws other boxes
    for args in ((5, "train", 1), (0, "train", 2), (5, "val", 2)):
        other = K.aug_draw(torch.tensor(ids), store.index_dev, n, *args, K.AUG_TRAIN, 16)
        assert not (torch.equal(other[1].cpu(), tf) and torch.equal(other[0].cpu(), ti))


def test_draw_refuses_bad_arguments(store):
    K = _K()
    n = len(store.images)
    for ids in ([0, n], [-1, 2]):
        with pytest.raises(ValueError, match="outside"):
            K.aug_draw(torch.tensor(ids), store.index_dev, n, 0, "train", 0, K.AUG_TRAIN, 16)
    with pytest.raises(ValueError, match="host"):
        K.aug_draw(torch.tensor([0, 1]).cuda(), store.index_dev, n, 0, "train", 0, K.AUG_TRAIN, 16)
    with pytest.raises(ValueError, match="index"):
        K.aug_draw(torch.tensor([0, 1]), store.index_dev, n + 1, 0, "train", 0, K.AUG_TRAIN, 16)
    with pytest.raises(ValueError, match="val mode"):
        K.aug_draw(torch.tensor([0, 1]), store.index_dev, n, 0, "val", 0, K.AUG_VAL, 16, 8)
    with pytest.raises(ValueError, match="scale"):
        K.aug_draw(torch.tensor([0, 1]), store.index_dev, n, 0, "train", 0, K.AUG_TRAIN, 16, scale=(0.5, 0.1))
    with pytest.raises(ValueError, match="batch_off"):
        K.aug_draw(torch.tensor([0, 1]), store.index_dev, n, 0, "train", 0, K.AUG_TRAIN, 16,
                   batch_off=torch.zeros(3, dtype=torch.int64, device=store.device))


# ------------------------------------------------------------------ pixels
@functools.lru_cache(maxsize=None)
def _pixel_ref(S, seed, epoch):
    """(float64 NCHW reference of all 11 fixture images, [11, 3] accumulation bound); read-only."""
    images, _ = P.fixture_images(0)
    boxes, flips = [], []
    for k, img in enumerate(images):
        box, flip, _, _ = P.draw_train(img.shape[1], img.shape[0], k, seed, epoch)
        boxes.append(box)
        flips.append(flip)
    ref = R.batch_nchw(images, boxes, flips, S)
    acc = np.stack([R.accum_bound(R.taps(b[0], b[2], i.shape[1], S), R.taps(b[1], b[3], i.shape[0], S))
                    for i, b in zip(images, boxes)])
    ref.setflags(write=False)
    return ref, acc


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("layout,dt", [("s2d", torch.bfloat16), ("nchw", torch.float32)])
def test_loader_pixels_match_reference(store, packed_dir, S, layout, dt):
    _, _, labels = packed_dir
    seed, epoch = 5, 1
    ref, acc = _pixel_ref(S, seed, epoch)
    ld = _loader(store, "train", S, layout, dt, seed)
    ld.set_epoch(epoch)
    batches = list(ld)
    assert len(ld) == len(batches) == 2 and [b[0].shape[0] for b in batches] == [7, 4]
    for step, (x, y) in enumerate(batches):
        ids = list(range(step * P.BATCH, min((step + 1) * P.BATCH, P.N_IMAGES)))
        assert x.is_cuda and y.is_cuda and x.dtype == dt and y.tolist() == [labels[i] for i in ids]
        want = ref[ids]
        bound = R.half_ulp(want, dt) + acc[ids][:, :, None, None]
        got = x.double().cpu().numpy()
        if layout == "s2d":
            assert got.shape == (len(ids), S // 2, S // 2, 16) and (got[..., 12:] == 0).all()
            got, want, bound = got[..., :12], R.s2d_from_nchw(want)[..., :12], R.s2d_from_nchw(bound)[..., :12]
        assert got.shape == want.shape and np.isfinite(got).all()
        ratio = np.abs(got - want) / bound
        print(f"packed S={S} {layout} step {step}: max error/bound {ratio.max():.4f}")
        assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


def test_val_matches_the_cpu_pipeline(tmp_path):
    """short_side = 256, S = 224, a 300x260 image: stored 295x256, val box integral at scale 1."""
    from PIL import Image
    from pytorch_distributed_amd.data.folder import val_transform
    from pytorch_distributed_amd.data.packed import PackedImages, write_packed
    rng = np.random.default_rng(7)
    images = [rng.integers(0, 256, (260, 300, 3), dtype=np.uint8),
              rng.integers(0, 256, (300, 260, 3), dtype=np.uint8)]
    P.make_tree(str(tmp_path), "val", images=images, labels=[0, 1])
    write_packed(str(tmp_path), "val", str(tmp_path / "val.pack"), short_side=256)
    pk = PackedImages(str(tmp_path / "val.pack"))
    assert pk.image(0).shape == (256, 295, 3) and pk.image(1).shape == (295, 256, 3)
    box = P.draw_val(295, 256, 224, 256)
    assert all(float(v).is_integer() for v in box) and box[2] - box[0] == box[3] - box[1] == 224
    ld = _loader(pk.to_device(_dev(), "device"), "val", 224, "nchw", torch.float32, batch=2, resize=256)
    (x, y), = list(ld)
    assert y.tolist() == [0, 1]
    f = val_transform(224, 256)
    want = torch.stack([f(Image.fromarray(i)) for i in images])
    err = (x.cpu() - want).abs().max().item()
    print(f"val vs val_transform: max |error| {err:.3e}")
    assert err <= 2e-6


# ------------------------------------------------------------------ residency, resume
def test_device_and_host_residency_agree(store):
    from pytorch_distributed_amd.data.packed import PackedStore
    host = PackedStore(store.images, _dev(), "host")
    chunked = PackedStore(store.images, _dev(), "device", stage_bytes=4096)     # many staging chunks
    assert host.mode == "host" and host.pixels_dev is None
    assert torch.equal(chunked.pixels_dev, store.pixels_dev)
    assert np.array_equal(store.pixels_dev.cpu().numpy(), store.images.pixels)
    auto = PackedStore(store.images, _dev(), "auto")
    assert auto.mode == "device"            # a few KB against the free memory of the device
    for split, S, layout, dt in (("train", 16, "s2d", torch.bfloat16), ("train", 64, "nchw", torch.float32),
                                 ("val", 16, "nchw", torch.float32)):
        a = list(_loader(store, split, S, layout, dt, seed=3))
        # three epochs' worth of batches through the two host staging slots
        for _ in range(3):
            b = list(_loader(host, split, S, layout, dt, seed=3))
            assert len(a) == len(b) == 2
            for (xa, ya), (xb, yb) in zip(a, b):
                assert torch.equal(xa, xb) and torch.equal(ya, yb)


def test_resume_and_epochs(store):
    ld = _loader(store, "train", 16, "s2d", torch.bfloat16, seed=1, batch=3)
    assert len(ld) == 4
    fresh = list(ld.iter_from(0))
    assert [s for s, _ in fresh] == [0, 1, 2, 3]
    for k in (1, 3):
        step, (x, y) = next(iter(ld.iter_from(k)))
        assert step == k and torch.equal(x, fresh[k][1][0]) and torch.equal(y, fresh[k][1][1])
    assert list(ld.iter_from(4)) == []
    ld.set_epoch(1)
    other = list(ld.iter_from(0))
    assert all(torch.equal(a[1][1], b[1][1]) for a, b in zip(fresh, other))         # same labels
    assert not all(torch.equal(a[1][0], b[1][0]) for a, b in zip(fresh, other))     # other crops
    ld.set_epoch(0)
    again = list(ld.iter_from(0))
    assert all(torch.equal(a[1][0], b[1][0]) for a, b in zip(fresh, again))
    capped = _loader(store, "train", 16, "s2d", torch.bfloat16, seed=1, batch=3, max_steps=2)
    assert len(capped) == 2 and len(list(capped)) == 2


def test_sampler_ids_are_used(store):
    """With a DistributedSampler the loader draws the sampler's ids: rank 1 of 2 gets the same rows
    for a sample as a plain loader does (same seed and epoch)."""
    from pytorch_distributed_amd.data import DistributedSampler
    plain = torch.cat([x for x, _ in _loader(store, "train", 16, seed=2)])
    sampler = DistributedSampler(store.images, 2, 1, shuffle=True, seed=2)
    ids = sampler.index_tensor().tolist()
    got = torch.cat([x for x, _ in _loader(store, "train", 16, seed=2, sampler=sampler, batch=4)])
    assert got.shape[0] == len(ids) == 6
    assert torch.equal(got, plain[ids])


# ------------------------------------------------------------------ entrypoint
def test_cli_trains_from_packed_files(packed_dir, tmp_path):
    env = dict(os.environ)
    env.update({"MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_BATCH": "4", "MX_IMAGE_SIZE": "32",
                "MX_DATA": f"packed:{packed_dir[0]}", "MX_ENGINE": "native", "MX_DTYPE": "bf16",
                "MX_METRICS": "1", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "resnet_single_gpu.py")], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "epoch: 0, step: 0" in r.stdout and "cost time per epoch" in r.stdout
    m = re.search(r"Epoch: 0, Loss: (\S+), Acc1: ", r.stdout)
    assert m and math.isfinite(float(m.group(1))), r.stdout[-2000:]
    assert "residency" in r.stdout
    assert '"engine": "native"' in (tmp_path / "output" / "resnet_single" / "metrics.jsonl").read_text()
