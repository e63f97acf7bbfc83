"""YCbCr 4:2:0 packed files on the GPU: the format-1 path of ``aug_resize_kernel`` (csrc/augment.hip,
``K.aug_resize(..., fmt=K.AUG_YUV420)``) against the float64 reference of tests/yuv_refs.py, element
by element, and the store, loader and entrypoint on version-2 files.

Bound per element (normalised units), derived in tests/yuv_refs.py, not fitted: half an ulp of the
stored dtype at the reference value plus ``(2 (kh + kv + 8) + 2) * 2^-23 * 255`` levels, with kh / kv
the image's own largest tap counts. The kernel's operation order is the one the bound assumes: the
three planes (Y, Cb - 128, Cr - 128) go through the tap loops of the RGB path, then per output value
``R = fma(1.402, cr, Y)``, ``G = fma(-0.714136, cr, fma(-0.344136, cb, Y))``, ``B = fma(1.772, cb, Y)``,
a clamp to [0, 255] and the normalising fma.

Grey images: every chroma byte is 128, so the chroma sums are exactly +0 and the conversion returns
Y itself; the clamp is the only operation the RGB path does not have. A filtered value can exceed
255 only when all its taps are 255 and the rounded f32 weights sum to more than 1, so the grey
fixture draws its levels from 0..254 (sum <= 254 (1 + k 2^-24) < 255) and the two packs must then give
bit-equal batches.
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
import yuv_refs as Y

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
S2D, NCHW = 0, 1
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 200), (200, 5), (53, 37), (48, 64)]      # (W, H)


def _K():
    from pytorch_distributed_amd.ops import native_ops as K
    return K


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------ kernel on hand-made tables
def _boxes(W, H, S):
    """The boxes of one image at output size S: the whole image; a fractional box that enlarges
    (smaller than S on both axes); a fractional box ending at the last column and row (odd for the
    odd sizes: its last chroma sample covers one luma column / row); where the image is large
    enough, a fractional box that shrinks by more than 2x on its long axis."""
    ew, eh = min(0.61 * W, 0.7 * S), min(0.61 * H, 0.7 * S)
    out = [(0, 0, W, H),
           (0.23 * (W - ew), 0.31 * (H - eh), 0.23 * (W - ew) + ew, 0.31 * (H - eh) + eh),
           (0.37 * W, 0.41 * H, W, H)]
    if max(W, H) * 0.93 > 2 * S:
        out.append((0.031 * W, 0.043 * H, 0.961 * W, 0.973 * H))
    return out


@functools.lru_cache(maxsize=None)
def _case(S):
    """(planes, boxes, S) of the batch at output size S; S = 258 is the two-column-tile case."""
    rng = np.random.default_rng(100 + S)
    planes, boxes = [], []
    if S == 258:
        for (W, H), box in (((53, 37), (0.5, 1.25, 52.75, 37)), ((48, 64), (0, 0, 48, 64))):
            planes.append(Y.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)))
            boxes.append(box)
        return planes, boxes, S
    for W, H in SIZES:
        p = Y.encode(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        for box in _boxes(W, H, S):
            planes.append(p)
            boxes.append(box)
    assert any((b[2] - b[0]) > 2 * S or (b[3] - b[1]) > 2 * S for b in boxes)
    assert any((b[2] - b[0]) < S and (b[3] - b[1]) < S and b[0] != int(b[0]) for b in boxes)
    return planes, boxes, S


@functools.lru_cache(maxsize=None)
def _ref(S):
    """(float64 NCHW reference WITHOUT flips, [B, 3] accumulation term); computed once, read-only.
    A flipped image's reference is the mirror of its row (yuv_refs.transform flips before a
    per-pixel conversion)."""
    planes, boxes, _ = _case(S)
    ref = Y.batch_nchw(planes, boxes, [False] * len(planes), S)
    acc = np.stack([Y.accum_bound(R.taps(b[0], b[2], p[0].shape[1], S), R.taps(b[1], b[3], p[0].shape[0], S))
                    for p, b in zip(planes, boxes)])
    ref.setflags(write=False)
    return ref, acc


def _check(got, want, bound, layout, tag):
    if layout == S2D:
        assert (got[..., 12:] == 0).all() and not np.signbit(got[..., 12:]).any()
        got, want, bound = got[..., :12], R.s2d_from_nchw(want)[..., :12], R.s2d_from_nchw(bound)[..., :12]
    assert got.shape == want.shape and np.isfinite(got).all()
    ratio = np.abs(got - want) / bound
    print(f"yuv {tag}: max error/bound {ratio.max():.4f}, max |error| {np.abs(got - want).max():.3e}")
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


CASES = [(d, S2D) for d in DTYPES] + [("f32", NCHW)]


@pytest.mark.parametrize("first_flipped", [False, True], ids=["flip_odd", "flip_even"])
@pytest.mark.parametrize("dt,layout", CASES, ids=lambda v: {0: "s2d", 1: "nchw"}.get(v, v))
@pytest.mark.parametrize("S", [2, 16, 64, 258])
def test_kernel_matches_reference(S, dt, layout, first_flipped):
    K = _K()
    dtype = DTYPES[dt]
    planes, boxes, _ = _case(S)
    B = len(planes)
    flips = [(b % 2 == 0) == first_flipped for b in range(B)]          # both runs: every image both ways
    assert (S != 258) or (B == 2 and sorted(flips) == [False, True])
    ref, acc = _ref(S)
    want = np.stack([ref[b][..., ::-1] if flips[b] else ref[b] for b in range(B)])
    packed, ti, tf = Y.pack(planes, boxes, flips)
    assert all(o % 2 == 1 for o in ti[:, 0].tolist())
    shape = (B, S // 2, S // 2, 16) if layout == S2D else (B, 3, S, S)
    out, check = R.guarded(shape, dtype, device="cuda")
    K.aug_resize(packed.cuda(), ti, tf, out, layout, fmt=K.AUG_YUV420)
    torch.cuda.synchronize()
    assert check(), "the kernel wrote outside its output"
    bound = R.half_ulp(want, dtype) + acc[:, :, None, None]
    _check(out.double().cpu().numpy(), want, bound, layout,
           f"S={S} {dt} {'s2d' if layout == S2D else 'nchw'} B={B}")


# ------------------------------------------------------------------ packs of the fixture tree
def _write_both(root, images, labels):
    """``<root>/rgb`` and ``<root>/yuv``: train.pack / val.pack of one tree in the two formats."""
    from pytorch_distributed_amd.data.packed import write_packed
    for split in ("train", "val"):
        P.make_tree(root, split, images=images, labels=labels)
    for fmt, sub in (("rgb", "rgb"), ("yuv420", "yuv")):
        os.makedirs(os.path.join(root, sub))
        for split in ("train", "val"):
            r = write_packed(root, split, os.path.join(root, sub, split + ".pack"), fmt=fmt)
            assert r["format"] == fmt


@pytest.fixture(scope="module")
def packs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("yuvpacks"))
    images, labels = P.fixture_images(0)
    _write_both(root, images, labels)
    return root, images, labels


def _store(root, sub, mode="device", **kw):
    from pytorch_distributed_amd.data.packed import PackedImages, PackedStore
    return PackedStore(PackedImages(os.path.join(root, sub, "train.pack")), _dev(), mode, **kw)


@pytest.fixture(scope="module")
def stores(packs):
    return _store(packs[0], "rgb"), _store(packs[0], "yuv")


def _loader(store, split="train", S=16, layout="nchw", dtype=torch.float32, seed=0, batch=P.BATCH, **kw):
    from pytorch_distributed_amd.data.packed import PackedLoader
    return PackedLoader(store, split, batch, dtype=dtype, layout=layout, image_size=S, seed=seed, **kw)


def test_grey_packs_give_bit_equal_batches(tmp_path):
    rng = np.random.default_rng(21)
    images = [np.repeat(rng.integers(0, 255, (H, W, 1), dtype=np.uint8), 3, axis=2)      # levels 0..254
              for W, H in P.fixture_sizes()]
    labels = P.fixture_images(0)[1]
    _write_both(str(tmp_path), images, labels)
    rgb, yuv = _store(str(tmp_path), "rgb"), _store(str(tmp_path), "yuv")
    assert rgb.format == "rgb" and yuv.format == "yuv420"
    assert 2 * yuv.images.pixel_bytes < 1.1 * rgb.images.pixel_bytes
    for k in range(len(images)):
        assert (yuv.images.planes(k)[1] == 128).all()
    for split, S, layout, dt in (("train", 16, "s2d", torch.bfloat16), ("train", 64, "nchw", torch.float32),
                                 ("train", 64, "s2d", torch.float32), ("val", 16, "nchw", torch.float32)):
        a = list(_loader(rgb, split, S, layout, dt, seed=4))
        b = list(_loader(yuv, split, S, layout, dt, seed=4))
        assert len(a) == len(b) == 2
        for (xa, ya), (xb, yb) in zip(a, b):
            assert torch.equal(xa, xb) and torch.equal(ya, yb), (split, S, layout)


@functools.lru_cache(maxsize=None)
def _pixel_ref(S, seed, epoch):
    """(float64 NCHW reference of the 11 fixture images from their yuv420 records, [11, 3] bound)."""
    images, _ = P.fixture_images(0)
    planes = [Y.encode(i) for i in images]
    boxes, flips = [], []
    for k, img in enumerate(images):
        box, flip, _, fragile = P.draw_train(img.shape[1], img.shape[0], k, seed, epoch)
        assert not fragile
        boxes.append(box)
        flips.append(flip)
    ref = Y.batch_nchw(planes, boxes, flips, S)
    acc = np.stack([Y.accum_bound(R.taps(b[0], b[2], i.shape[1], S), R.taps(b[1], b[3], i.shape[0], S))
                    for i, b in zip(images, boxes)])
    ref.setflags(write=False)
    return ref, acc


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("layout,dt", [("s2d", torch.bfloat16), ("nchw", torch.float32)])
def test_loader_pixels_match_reference(stores, packs, S, layout, dt):
    _, _, labels = packs
    seed, epoch = 5, 1
    ref, acc = _pixel_ref(S, seed, epoch)
    ld = _loader(stores[1], "train", S, layout, dt, seed)
    ld.set_epoch(epoch)
    batches = list(ld)
    assert len(ld) == len(batches) == 2 and [b[0].shape[0] for b in batches] == [7, 4]
    for step, (x, y) in enumerate(batches):
        ids = list(range(step * P.BATCH, min((step + 1) * P.BATCH, P.N_IMAGES)))
        assert x.is_cuda and y.is_cuda and x.dtype == dt and y.tolist() == [labels[i] for i in ids]
        want = ref[ids]
        bound = R.half_ulp(want, dt) + acc[ids][:, :, None, None]
        got = x.double().cpu().numpy()
        assert got.shape == ((len(ids), S // 2, S // 2, 16) if layout == "s2d" else (len(ids), 3, S, S))
        _check(got, want, bound, S2D if layout == "s2d" else NCHW, f"loader S={S} {layout} step {step}")


def test_draw_is_independent_of_the_format(stores):
    K = _K()
    rgb, yuv = stores
    n = len(rgb.images)
    assert rgb.images.index[:, 1:].tolist() == yuv.images.index[:, 1:].tolist()
    assert rgb.images.index[1:, 0].tolist() != yuv.images.index[1:, 0].tolist()
    for ids in ([3, 0, 10, 7, 5, 9, 1], [2, 4, 6, 8, 3, 0, 10]):
        for args, mode, resize in (((5, "train", 1), K.AUG_TRAIN, 0), ((0, "val", 0), K.AUG_VAL, 18)):
            a = K.aug_draw(torch.tensor(ids), rgb.index_dev, n, *args, mode, 16, resize)
            b = K.aug_draw(torch.tensor(ids), yuv.index_dev, n, *args, mode, 16, resize)
            assert torch.equal(a[0][:, 1:], b[0][:, 1:]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
            assert a[0][:, 0].tolist() == [int(rgb.images.index[i, 0]) for i in ids]
            assert b[0][:, 0].tolist() == [int(yuv.images.index[i, 0]) for i in ids]


def test_device_and_host_residency_agree(stores, packs):
    yuv = stores[1]
    host = _store(packs[0], "yuv", "host")
    chunked = _store(packs[0], "yuv", "device", stage_bytes=4096)       # many staging chunks
    assert host.mode == "host" and host.pixels_dev is None and host.format == "yuv420"
    assert yuv.images.pixel_bytes > 4 * 4096
    assert torch.equal(chunked.pixels_dev, yuv.pixels_dev)
    assert np.array_equal(chunked.pixels_dev.cpu().numpy(), yuv.images.pixels)
    for split, S, layout, dt in (("train", 16, "s2d", torch.bfloat16), ("train", 64, "nchw", torch.float32),
                                 ("val", 16, "nchw", torch.float32)):
        a = list(_loader(yuv, split, S, layout, dt, seed=3))
        for _ in range(3):      # three epochs' worth of batches through the two host staging slots
            b = list(_loader(host, split, S, layout, dt, seed=3))
            assert len(a) == len(b) == 2
            for (xa, ya), (xb, yb) in zip(a, b):
                assert torch.equal(xa, xb) and torch.equal(ya, yb)


# ------------------------------------------------------------------ entrypoint
def test_cli_trains_from_yuv420_files(packs, tmp_path):
    env = dict(os.environ)
    env.update({"MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_BATCH": "4", "MX_IMAGE_SIZE": "32",
                "MX_DATA": f"packed:{os.path.join(packs[0], 'yuv')}", "MX_ENGINE": "native",
                "MX_DTYPE": "bf16", "MX_METRICS": "1", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "resnet_single_gpu.py")], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "epoch: 0, step: 0" in r.stdout and "cost time per epoch" in r.stdout
    m = re.search(r"Epoch: 0, Loss: (\S+), Acc1: ", r.stdout)
    assert m and math.isfinite(float(m.group(1))), r.stdout[-2000:]
    lines = [l for l in r.stdout.splitlines() if "residency" in l]
    assert lines and all("yuv420" in l for l in lines), lines
    assert '"engine": "native"' in (tmp_path / "output" / "resnet_single" / "metrics.jsonl").read_text()
