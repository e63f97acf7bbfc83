"""The folder-image augmentation kernel (csrc/augment.hip, ``K.aug_resize``) against the float64
reference of tests/aug_refs.py, element by element, and the loader / entrypoint built on it.

Bound per element (normalised units), derived, not fitted:

* half an ulp of the output dtype at the reference value: the kernel's one rounding of its f32
  result to the stored dtype (f32 itself: the final fma's rounding);
* plus ``(kh + kv + 8) * 2^-23 * 255 / (255*STD[c])``, the f32 arithmetic before it, with kh / kv
  the image's own largest tap counts. In levels: each pass is a chain of k fmas whose partial sums
  stay <= 255, so each step rounds by <= 2^-24 * 256, and the f32 tap weights (rounded once from
  the double product w * 1/sum(w)) add a relative 2^-24 to a sum <= 255: (k + 1) * 2^-24 * 256 per
  pass, i.e. about half of the (kh + kv) * 2^-23 * 255 the bound grants. The remaining 8 * 2^-23 *
  255 levels cover the normalisation ``fma(R, a, b)`` with a = 1/(255 std) and b = -mean/std
  rounded to f32: <= (|R a| + |b| + |out|) * 2^-24 <= 9.4 * 2^-24 against 16 * 2^-24 / STD[c] >=
  69 * 2^-24.

Largest observed error / bound over all cases of ``test_kernel_matches_reference``, per dtype
(MI355X): f32 0.114 (s258), f16 0.993, bf16 0.999. The 16-bit ratios sit just under 1 because the
half ulp of the store dominates their bound and a correctly rounded value attains it; f32 shows that
the arithmetic before the store uses about a ninth of its allowance.
"""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import aug_refs as R
from pytorch_distributed_amd.data.synthetic import STD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
S2D, NCHW = 0, 1


def _K():
    from pytorch_distributed_amd.ops import native_ops as K
    return K


# ------------------------------------------------------------------ cases
def _img(seed, W, H, binary=False):
    rng = np.random.default_rng(seed)
    if binary:
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(images, boxes, flips, gaps, S) of a named batch."""
    from pytorch_distributed_amd.data.folder import val_crop_params
    small = [_img(1, 48, 40), _img(2, 5, 7, True), _img(3, 300, 10), _img(4, 10, 300),
             _img(5, 263, 257), _img(6, 64, 64, True)]
    gaps = [1, 3, 0, 7, 5, 9]                      # image byte offsets 1, 5764, ...: odd ones
    if name == "mixed_a":
        boxes = [(0, 0, 48, 40),                   # whole image
                 (0, 0, 5, 7),                     # upscaling, whole image
                 (150, 0, 151, 10),                # one pixel wide
                 (0, 150, 10, 151),                # one pixel high
                 (3, 1, 259, 257),                 # ~8x downscale, touches the bottom
                 val_crop_params(64, 64, 32, 36)]  # fractional (Resize -> CenterCrop)
        return small, boxes, [False, True, False, True, True, False], gaps, 32
    if name == "mixed_b":
        boxes = [(0, 0, 20, 22),                   # touches left and top
                 (1, 2, 3, 5),                     # strong upscaling inside the image
                 (143, 0, 156, 10),                # RandomResizedCrop's fallback box
                 (4, 200, 10, 300),                # touches right and bottom
                 (0.37, 10.62, 262.5, 250.1),      # fractional ~8x downscale
                 (0, 0, 64, 64)]
        return small, boxes, [True, False, True, False, False, True], gaps, 32
    if name == "s224":                             # the many-chunk band: ~19 taps per axis
        imgs = [_img(7, 500, 375), _img(8, 2000, 1500)]
        return imgs, [(37, 21, 391, 330), (0, 0, 2000, 1500)], [True, False], [3, 1], 224
    if name == "s258":                             # two column tiles (256 + 2)
        imgs = [_img(9, 48, 40), _img(10, 263, 257)]
        return imgs, [(0, 0, 48, 40), (0.5, 1.25, 262.75, 256)], [True, False], [1, 2], 258
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(float64 NCHW reference, [B, 3] accumulation term of the bound); computed once, read-only."""
    imgs, boxes, flips, _, S = _case(name)
    ref = R.batch_nchw(imgs, boxes, flips, S)
    acc = np.stack([R.accum_bound(R.taps(b[0], b[2], i.shape[1], S), R.taps(b[1], b[3], i.shape[0], S))
                    for i, b in zip(imgs, boxes)])
    ref.setflags(write=False)
    return ref, acc


def _launch(name, dtype, layout, flips=None):
    """Run the kernel on a named batch into a guarded output; returns (out, guard check)."""
    imgs, boxes, case_flips, gaps, S = _case(name)
    packed, ti, tf = R.pack(imgs, boxes, flips if flips is not None else case_flips, gaps)
    B = len(imgs)
    shape = (B, S // 2, S // 2, 16) if layout == S2D else (B, 3, S, S)
    out, check = R.guarded(shape, dtype, device="cuda")
    _K().aug_resize(packed.cuda(), ti, tf, out, layout)
    torch.cuda.synchronize()
    return out, check


CASES = [(n, d, S2D) for n in ("mixed_a", "mixed_b", "s224", "s258") for d in DTYPES] + \
        [(n, "f32", NCHW) for n in ("mixed_a", "mixed_b", "s224", "s258")]


@pytest.mark.parametrize("name,dt,layout", CASES, ids=lambda v: {0: "s2d", 1: "nchw"}.get(v, v))
def test_kernel_matches_reference(name, dt, layout):
    dtype = DTYPES[dt]
    ref, acc = _ref(name)
    out, check = _launch(name, dtype, layout)
    assert check(), "the kernel wrote outside its output"
    got = out.double().cpu().numpy()
    bound_nchw = R.half_ulp(ref, dtype) + acc[:, :, None, None]
    if layout == S2D:
        assert (got[..., 12:] == 0).all() and not np.signbit(got[..., 12:]).any()
        want, bound = R.s2d_from_nchw(ref), R.s2d_from_nchw(bound_nchw)
        got, want, bound = got[..., :12], want[..., :12], bound[..., :12]
    else:
        want, bound = ref, bound_nchw
    assert np.isfinite(got).all()
    ratio = np.abs(got - want) / bound
    print(f"aug {name} {dt} {'s2d' if layout == S2D else 'nchw'}: max error/bound {ratio.max():.4f}, "
          f"max |error| {np.abs(got - want).max():.3e}")
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))


@pytest.mark.parametrize("name", ["mixed_a", "s258"])
def test_flip_is_the_mirror_and_launches_repeat(name):
    _, _, flips, _, _ = _case(name)
    a, _ = _launch(name, torch.float32, NCHW)
    b, _ = _launch(name, torch.float32, NCHW)
    assert torch.equal(a, b)                                    # bit-equal run to run
    f, _ = _launch(name, torch.float32, NCHW, flips=[not v for v in flips])
    assert torch.equal(f, a.flip(3))
    s1, _ = _launch(name, torch.bfloat16, S2D)
    s2, _ = _launch(name, torch.bfloat16, S2D)
    assert torch.equal(s1, s2)


@pytest.mark.parametrize("name", ["mixed_b", "s224", "s258"])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_s2d_equals_nchw_to_s2d_of_the_nchw_output(name, dt):
    nchw, _ = _launch(name, torch.float32, NCHW)
    s2d, _ = _launch(name, DTYPES[dt], S2D)
    via = torch.empty_like(s2d)
    _K().nchw_to_s2d(nchw.contiguous(), via)
    torch.cuda.synchronize()
    assert torch.equal(s2d, via)


def test_bad_table_never_launches():
    K = _K()
    imgs, boxes, flips, gaps, S = _case("mixed_a")
    packed, ti, tf = R.pack(imgs, boxes, flips, gaps)
    out, check = R.guarded((len(imgs), 3, S, S), torch.float32, device="cuda")
    before = out.clone()
    ti[4, 0] = packed.numel() - 10
    with pytest.raises(ValueError):
        K.aug_resize(packed.cuda(), ti, tf, out, NCHW)
    torch.cuda.synchronize()
    assert check() and torch.equal(torch.nan_to_num(out), torch.nan_to_num(before))


# ------------------------------------------------------------------ loader
def _loaders(root, split, seed, layout, dtype, S=32):
    from pytorch_distributed_amd.data.folder import (ImageFolder, train_params, train_transform,
                                                     val_params, val_transform)
    if split == "train":
        cpu_ds = ImageFolder(root, split, train_transform(S, rng=random.Random(seed)))
        gpu_ds = ImageFolder(root, split, raw_params=train_params(rng=random.Random(seed)))
    else:
        cpu_ds = ImageFolder(root, split, val_transform(S, 36))
        gpu_ds = ImageFolder(root, split, raw_params=val_params(S, 36))
    return (cpu_ds.loader(5, num_workers=0),
            gpu_ds.loader(5, num_workers=0, device=torch.device("cuda", torch.cuda.current_device()),
                          dtype=dtype, layout=layout, image_size=S))


@pytest.mark.parametrize("split", ["train", "val"])
@pytest.mark.parametrize("layout,dt", [("nchw", "f32"), ("s2d", "bf16"), ("s2d", "f32")])
def test_loader_matches_the_cpu_path(tmp_path, split, layout, dt):
    from test_folder_data_cpu import _make_tree
    _make_tree(str(tmp_path))
    dtype = DTYPES[dt]
    pil_tol = (1.01 / (255.0 * np.asarray(STD)) + 1e-6).reshape(1, 3, 1, 1)
    for start in (0, 1):     # both draw per item from a fresh Random(seed): a resumed epoch agrees too
        cpu_ld, gpu_ld = _loaders(str(tmp_path), split, 11, layout, dtype)
        assert len(cpu_ld) == len(gpu_ld) == 3
        cpu_b, gpu_b = list(cpu_ld.iter_from(start)), list(gpu_ld.iter_from(start))
        assert [s for s, _ in cpu_b] == [s for s, _ in gpu_b] == list(range(start, 3))
        for (_, (xc, yc)), (_, (xg, yg)) in zip(cpu_b, gpu_b):
            assert xg.is_cuda and yg.is_cuda and xg.dtype == dtype and torch.equal(yg.cpu(), yc)
            want = xc.double().numpy()
            tol = pil_tol + R.half_ulp(want, dtype)
            got = xg.double().cpu().numpy()
            if layout == "s2d":
                assert got.shape == (xc.shape[0], 16, 16, 16) and (got[..., 12:] == 0).all()
                want, tol = R.s2d_from_nchw(want)[..., :12], R.s2d_from_nchw(tol)[..., :12]
                got = got[..., :12]
            assert got.shape == want.shape
            assert (np.abs(got - want) <= tol).all(), np.abs(got - want).max()


# ------------------------------------------------------------------ entrypoint
def test_cli_with_gpu_augmentation(tmp_path):
    from test_folder_data_cpu import _make_tree
    _make_tree(str(tmp_path / "data"))
    env = dict(os.environ)
    env.update({"MX_ARCH": "resnet18", "MX_EPOCHS": "1", "MX_BATCH": "4", "MX_IMAGE_SIZE": "32",
                "MX_DATA": f"folder:{tmp_path / 'data'}", "MX_AUG": "gpu", "MX_ENGINE": "native",
                "MX_WORKERS": "0", "MX_METRICS": "1", "PYTHONPATH": ROOT})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "resnet_single_gpu.py")], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Epoch: 0, Loss: " in r.stdout and "cost time per epoch" in r.stdout
    assert '"engine": "native"' in (tmp_path / "output" / "resnet_single" / "metrics.jsonl").read_text()
