"""thumbnail() on the GPU (lars_h_thumbnail_u8): bit-identical to Pillow's Image.thumbnail(size, LANCZOS, reducing_gap)
on the same machine -- reduce, fractional float32 boxes, JPEG draft, RGBA, the tall-image branch."""
import io

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars

pytestmark = pytest.mark.gpu

LANCZOS = Image.Resampling.LANCZOS


def _image(w, h, mode, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if mode == "L" else (h, w, len(mode))
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    # a smooth ramp above the noise: the resampler's clipping and rounding both show up
    ramp = (np.arange(w, dtype=np.int64) * 255 // max(w - 1, 1)).astype(np.uint8)
    a[: h // 3] = ramp[None, :] if mode == "L" else ramp[None, :, None]
    if mode == "RGBA":
        a[h // 4: h // 2, :, 3] = 0
        a[h // 2: 3 * h // 4, :, 3] = 255
    return a


def _pillow(im, size, gap):
    im.thumbnail(size, LANCZOS, gap)
    return np.asarray(im)


def _check_array(a, size=(400, 400), gap=2.0):
    want = _pillow(Image.fromarray(a), size, gap)
    got = lars.thumbnail(a, size, gap)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    # and the PIL flavour of the same call
    pil = Image.fromarray(a)
    got_pil = lars.thumbnail(pil, size, gap)
    assert isinstance(got_pil, Image.Image) and got_pil.mode == pil.mode
    np.testing.assert_array_equal(np.asarray(got_pil), want)
    return got


@pytest.mark.parametrize("mode", ["L", "RGB"])
@pytest.mark.parametrize("wh", [(2048, 1536), (1536, 2048), (4000, 3000), (2047, 1001), (401, 1999), (2999, 2999), (2803, 1201),
                                (2048, 2048)])
def test_thumbnail_matches_pillow_sizes(wh, mode):
    _check_array(_image(*wh, mode, seed=wh[0] * 7 + wh[1]))


@pytest.mark.parametrize("wh", [(2048, 1536), (1203, 905), (401, 1999)])
def test_thumbnail_rgba_matches_pillow(wh):
    a = _image(*wh, "RGBA", seed=5)
    got = _check_array(a)
    assert (got[..., 3] == 0).any() and (got[..., 3] == 255).any()


@pytest.mark.parametrize("gap", [None, 1.0, 3.0, 2.0])
@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA"])
def test_thumbnail_reducing_gap(gap, mode):
    _check_array(_image(1203, 905, mode, seed=11), gap=gap)


@pytest.mark.parametrize("size", [(128, 128), (400, 300), (64, 400), (400.7, 250.2)])
@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA"])
def test_thumbnail_requested_sizes(size, mode):
    _check_array(_image(2048, 1536, mode, seed=13), size=size)


@pytest.mark.parametrize("wh", [(7, 900), (900, 7), (3, 2001), (5, 1000)])
@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA"])
def test_thumbnail_tall_and_wide(wh, mode):
    """h > 100 w takes Image.resize's vertical-first branch; the wide mirror does not."""
    plan = lars.thumbnail_plan(wh, (400, 400), 2.0, rgba=mode == "RGBA")
    assert plan.vertical_first == (wh[1] > 100 * wh[0])
    _check_array(_image(*wh, mode, seed=17), size=(400, 400))


def _encoded(a, fmt, **kw):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, fmt, **kw)
    return buf.getvalue()


FILE_CASES = [(fmt, wh, mode) for fmt in ("PNG", "TIFF", "JPEG")
              for wh, mode in [((2048, 1536), "RGB"), ((3333, 2001), "RGB"), ((1001, 777), "L"), ((3333, 2001), "L"),
                               ((1700, 1300), "RGBA")]
              if not (fmt == "JPEG" and mode == "RGBA")]           # JPEG holds no alpha


@pytest.mark.parametrize("fmt,wh,mode", FILE_CASES)
@pytest.mark.parametrize("gap", [2.0, 1.0, None])
def test_thumbnail_file_backed(fmt, wh, mode, gap):
    data = _encoded(_image(*wh, mode, seed=23), fmt, **({"quality": 92} if fmt == "JPEG" else {}))
    ref = Image.open(io.BytesIO(data))
    ref.thumbnail((400, 400), LANCZOS, gap)
    want = np.asarray(ref)
    im = Image.open(io.BytesIO(data))
    got = lars.thumbnail(im, (400, 400), gap)
    assert isinstance(got, Image.Image) and got.mode == mode
    np.testing.assert_array_equal(np.asarray(got), want)
    if fmt == "JPEG" and gap is not None:
        probe = Image.open(io.BytesIO(data))
        probe.draft(None, (int(400 * gap), int(400 * gap)))
        assert im.size == probe.size                                # drafted in place, as Pillow's call drafts
    else:
        assert im.size == wh


@pytest.mark.parametrize("wh", [(3333, 2001), (2047, 1999), (3001, 1701)])
def test_thumbnail_jpeg_fractional_draft_box(wh):
    """JPEG sizes whose draft scale leaves a fractional box (e.g. 1666.5 x 1000.5)."""
    data = _encoded(_image(*wh, "RGB", seed=29), "JPEG", quality=90)
    probe = Image.open(io.BytesIO(data))
    _, box = probe.draft(None, (800, 800))
    assert any(v != int(v) for v in box), box
    ref = Image.open(io.BytesIO(data))
    ref.thumbnail((400, 400), LANCZOS)
    got = lars.thumbnail(Image.open(io.BytesIO(data)))
    np.testing.assert_array_equal(np.asarray(got), np.asarray(ref))


def test_thumbnail_does_not_touch_input():
    a = _image(2048, 1536, "RGBA", seed=31)
    keep = a.copy()
    lars.thumbnail(a)
    np.testing.assert_array_equal(a, keep)
    # non-contiguous input
    b = _image(3000, 2000, "RGB", seed=37)[::2, ::3]
    np.testing.assert_array_equal(lars.thumbnail(b), _pillow(Image.fromarray(np.ascontiguousarray(b)), (400, 400), 2.0))


def test_thumbnail_fuzz():
    """~150 random shapes up to 2048 px, random requests, modes and reducing gaps."""
    rng = np.random.default_rng(2024)
    n = 0
    for case in range(150):
        w, h = (int(v) for v in rng.integers(1, 2049, 2))
        if rng.random() < 0.15:
            w = int(rng.integers(1, 12))
        mode = ["L", "RGB", "RGBA"][case % 3]
        size = (float(rng.uniform(1, 600)), float(rng.uniform(1, 600))) if rng.random() < 0.3 else \
            (int(rng.integers(1, 600)), int(rng.integers(1, 600)))
        gap = [None, 1.0, 1.5, 2.0, 3.0][int(rng.integers(0, 5))]
        a = _image(w, h, mode, seed=1000 + case)
        want = _pillow(Image.fromarray(a), size, gap)
        got = lars.thumbnail(a, size, gap)
        assert got.shape == want.shape, (case, w, h, mode, size, gap)
        np.testing.assert_array_equal(got, want, err_msg=str((case, w, h, mode, size, gap)))
        n += got is not a
    assert n > 100
