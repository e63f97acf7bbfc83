"""The YCbCr 4:2:0 packed format (data/packed.py version 2) on the CPU: ``write_packed(fmt="yuv420")``
against the integer encoder of tests/yuv_refs.py byte for byte, the properties of the stored image,
the reader's whole-index validation by yuv record sizes, and the refusals of the wrappers."""
import os
import struct

import numpy as np
import pytest
import torch

import packed_refs as P
import yuv_refs as Y

TINY = [(1, 1), (1, 2), (2, 1), (3, 3), (3, 2)]          # (W, H): images of 1x1, 2x1, 1x2, 3x3, 2x3


def _images():
    images, labels = P.fixture_images(0)
    rng = np.random.default_rng(11)
    images = images + [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for W, H in TINY]
    return images, labels + [0] * len(TINY)


def _write(tmp_path, images, labels, name="train.pack", **kw):
    from pytorch_distributed_amd.data.packed import write_packed
    if not (tmp_path / "train").exists():
        P.make_tree(str(tmp_path), "train", images=images, labels=labels)
    return write_packed(str(tmp_path), "train", str(tmp_path / name), **kw)


def _sorted(images, labels):
    """Dataset order: ImageFolder lists class folders, then file names; make_tree names files by
    fixture index, so the order is by (label, index)."""
    order = sorted(range(len(images)), key=lambda k: (labels[k], k))
    return [images[k] for k in order], [labels[k] for k in order]


# ------------------------------------------------------------------ encoding
def test_records_equal_the_reference_encoder(tmp_path):
    from pytorch_distributed_amd.data.packed import PackedImages
    images, labels = _sorted(*_images())
    r = _write(tmp_path, images, labels, fmt="yuv420", workers=0)
    pk = PackedImages(str(tmp_path / "train.pack"))
    assert r["format"] == "yuv420" and pk.format == "yuv420" and len(pk) == len(images)
    assert struct.unpack_from("<Q", (tmp_path / "train.pack").read_bytes(), 8)[0] == 2
    off = 0
    for k, (img, label) in enumerate(zip(images, labels)):
        H, W, _ = img.shape
        want = Y.encode(img)
        n = H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)
        assert pk.index[k].tolist() == [off, H, W, label] and int(pk.nbytes[k]) == n
        assert np.array_equal(pk.pixels[off:off + n], Y.record(want)), k
        y, c = pk.planes(k)
        assert y.shape == (H, W) and c.shape == ((H + 1) // 2, (W + 1) // 2, 2)
        assert y.dtype == c.dtype == np.uint8
        assert np.array_equal(y, want[0]) and np.array_equal(c, want[1])
        off += n
    assert pk.pixel_bytes == off == r["pixel_bytes"]
    with pytest.raises(ValueError, match="planes"):
        pk.image(0)
    # worker processes write the same file
    _write(tmp_path, images, labels, "b.pack", fmt="yuv420", workers=2)
    assert (tmp_path / "train.pack").read_bytes() == (tmp_path / "b.pack").read_bytes()


def test_grey_is_exact_and_constant_colours_are_close(tmp_path):
    from pytorch_distributed_amd.data.packed import PackedImages
    rng = np.random.default_rng(3)
    grey = [np.repeat(rng.integers(0, 256, (H, W, 1), dtype=np.uint8), 3, axis=2)
            for W, H in [(7, 5), (1, 1), (16, 16)]]
    grey.append(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2))    # every level
    colours = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0),
               (0, 255, 255), (255, 0, 255), (1, 2, 3), (200, 100, 50)]
    colours += [tuple(int(v) for v in c) for c in rng.integers(0, 256, (40, 3))]
    const = [np.broadcast_to(np.array(c, dtype=np.uint8), (3, 5, 3)).copy() for c in colours]
    images = grey + const
    _write(tmp_path, images, [0] * len(images), fmt="yuv420")
    pk = PackedImages(str(tmp_path / "train.pack"))
    for k, img in enumerate(images):
        planes = pk.planes(k)
        got = Y.stored_image(planes)
        if k < len(grey):
            assert (planes[1] == 128).all() and np.array_equal(planes[0], img[..., 0])
            assert np.array_equal(got, img.astype(np.float64))          # exact: chroma terms are 0
        else:
            err = np.abs(got - img).max()
            assert err <= 1.5, (colours[k - len(grey)], err)


def test_rgb_format_writes_the_version_1_file(tmp_path):
    from pytorch_distributed_amd.data.packed import PackedImages
    images, labels = _images()
    plain = _write(tmp_path, images, labels, "plain.pack")
    named = _write(tmp_path, images, labels, "named.pack", fmt="rgb")
    assert (tmp_path / "plain.pack").read_bytes() == (tmp_path / "named.pack").read_bytes()
    assert plain["format"] == named["format"] == "rgb"
    assert struct.unpack_from("<Q", (tmp_path / "plain.pack").read_bytes(), 8)[0] == 1
    pk = PackedImages(str(tmp_path / "plain.pack"))
    assert pk.format == "rgb" and pk.image(0).shape[2] == 3
    yuv = _write(tmp_path, images, labels, "yuv.pack", fmt="yuv420")
    assert yuv["pixel_bytes"] < 0.55 * plain["pixel_bytes"]
    for bad in ("yuv422", "RGB", "", None, 2):
        with pytest.raises(ValueError, match="fmt"):
            _write(tmp_path, images, labels, "bad.pack", fmt=bad)


# ------------------------------------------------------------------ reader validation
def _patched(tmp_path, name, edit):
    """A copy of the yuv420 fixture file with ``edit(bytearray, header fields)`` applied."""
    from pytorch_distributed_amd.data.packed import _HEADER
    src = tmp_path / "train.pack"
    if not src.exists():
        images, labels = P.fixture_images(0)
        _write(tmp_path, images, labels, fmt="yuv420")
    data = bytearray(src.read_bytes())
    out = edit(data, list(_HEADER.unpack_from(data, 0)))
    (tmp_path / name).write_bytes(bytes(out if out is not None else data))
    return str(tmp_path / name)


def _set(data, hdr, k, col, value):
    struct.pack_into("<q", data, hdr[6] + (k * 4 + col) * 8, value)


def _get(data, hdr, k, col):
    return struct.unpack_from("<q", data, hdr[6] + (k * 4 + col) * 8)[0]


def test_bad_yuv_files_are_refused(tmp_path):
    from pytorch_distributed_amd.data.packed import PackedImages
    pk = PackedImages(_patched(tmp_path, "ok.pack", lambda d, h: None))
    last = len(pk) - 1
    H, W = int(pk.index[last, 1]), int(pk.index[last, 2])
    assert int(pk.index[last, 0]) + Y.record_bytes(H, W) == pk.pixel_bytes      # the last record ends the file

    def cut(d, h):          # drop 3 bytes of the last CbCr plane and say so in the header
        struct.pack_into("<Q", d, 64, h[8] - 3)
        return d[:-3]
    with pytest.raises(ValueError, match=rf"record {last}: bytes .* outside the pixel section"):
        PackedImages(_patched(tmp_path, "cut.pack", cut))
    with pytest.raises(ValueError, match="truncated"):
        PackedImages(_patched(tmp_path, "short.pack", lambda d, h: d[:-3]))
    # one byte less than the yuv record is left behind this offset (the rgb size would have been
    # refused for any offset in the last record's second half; this one is decided by the yuv size)
    n4 = Y.record_bytes(*[int(v) for v in pk.index[4, 1:3]])
    with pytest.raises(ValueError, match=r"record 4: bytes .* outside the pixel section"):
        PackedImages(_patched(tmp_path, "off.pack", lambda d, h: _set(d, h, 4, 0, h[8] - n4 + 1)))
    # records 5 and 6 are adjacent; moving 6 one byte back overlaps it with the end of 5's CbCr plane
    with pytest.raises(ValueError, match=r"record 6: its bytes overlap"):
        PackedImages(_patched(tmp_path, "overlap.pack", lambda d, h: _set(d, h, 6, 0, _get(d, h, 6, 0) - 1)))
    with pytest.raises(ValueError, match="version 3"):
        PackedImages(_patched(tmp_path, "v3.pack", lambda d, h: struct.pack_into("<Q", d, 8, 3)))
    # the same bytes read as version 1 are too short for rgb records: the version selects the size
    with pytest.raises(ValueError, match=r"outside the pixel section"):
        PackedImages(_patched(tmp_path, "v1.pack", lambda d, h: struct.pack_into("<Q", d, 8, 1)))


# ------------------------------------------------------------------ wrappers
def test_wrappers_check_the_format_on_the_host():
    from pytorch_distributed_amd.ops import native_ops as K
    assert (K.AUG_RGB, K.AUG_YUV420) == (0, 1)
    img = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)      # W = 7, H = 5
    planes = Y.encode(img)
    packed, ti, tf = Y.pack([planes], [(0, 0, 7, 5)], [False], gaps=[1])
    assert packed.numel() == 1 + 35 + 2 * 3 * 4
    out = torch.empty(1, 3, 4, 4)
    assert K.aug_check(packed, ti, tf, out, K.AUG_NCHW, K.AUG_YUV420) == (1, 4)
    assert K.aug_check(packed, ti, tf, out, K.AUG_NCHW, fmt=K.AUG_YUV420) == (1, 4)
    with pytest.raises(ValueError, match="outside the packed buffer"):     # 3*35 rgb bytes are not there
        K.aug_check(packed, ti, tf, out, K.AUG_NCHW)
    with pytest.raises(ValueError, match=r"image 0: bytes \[1, 60\) outside the packed buffer of 59"):
        K.aug_check(packed[:-1].clone(), ti, tf, out, K.AUG_NCHW, K.AUG_YUV420)
    for bad in (2, -1, "yuv420", None):
        with pytest.raises(ValueError, match="fmt"):
            K.aug_check(packed, ti, tf, out, K.AUG_NCHW, bad)
        with pytest.raises(ValueError, match="fmt"):       # before the device check and any launch
            K.aug_resize(packed, ti, tf, out, K.AUG_NCHW, bad)
        with pytest.raises(ValueError, match="fmt"):
            K.aug_resize_dev(packed, ti, tf, out, K.AUG_NCHW, bad)


def test_reference_pack_makes_odd_offsets():
    imgs = [np.zeros((H, W, 3), dtype=np.uint8) for W, H in TINY + [(4, 4)]]
    packed, ti, _ = Y.pack([Y.encode(i) for i in imgs], [(0, 0, i.shape[1], i.shape[0]) for i in imgs],
                           [False] * len(imgs))
    assert all(o % 2 == 1 for o in ti[:, 0].tolist())
    assert packed.numel() == int(ti[-1, 0]) + Y.record_bytes(4, 4)
