"""thumbnail() on the host: Pillow's thumbnail policy (api.thumbnail_plan), the modes it refuses, the calls that never reach
the GPU, and the arguments the C entry point receives.  No GPU needed."""
import io
import itertools

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api


def _grid():
    sides = [1, 2, 3, 7, 64, 99, 100, 101, 299, 300, 399, 400, 401, 799, 800, 801, 1001, 1536, 2047, 2048, 2803, 4000]
    sizes = [(400, 400), (400, 300), (64, 400), (128, 128), (1, 1), (400.7, 300.2), (150.5, 149.9), (1000, 50)]
    gaps = [2.0, None, 1.0, 3.0, 1.5]
    cases = [(w, h, s, g) for (w, h), s, g in itertools.product(itertools.product(sides, sides), sizes, gaps)
             if (w * 131 + h * 17 + int(s[0] * 7) + (g or 0) * 3) % 4 == 0]
    cases += [(w, h, (400, 400), 2.0) for w, h in [(7, 900), (900, 7), (1, 4000), (4000, 1), (5, 2001), (2001, 5), (3, 301)]]
    return cases


CASES = _grid()


def test_grid_is_large():
    assert len(CASES) > 2000


def test_plan_size_matches_pillow_thumbnail():
    """The final size over a few thousand (w, h, requested size, reducing_gap) cases, against Pillow on a mode-1 image."""
    bad = []
    for w, h, size, gap in CASES:
        im = Image.new("1", (w, h))
        im.thumbnail(size, Image.Resampling.LANCZOS, gap)
        plan = lars.thumbnail_plan((w, h), size, gap)
        got = (w, h) if plan is None else plan.size
        if got != im.size:
            bad.append(((w, h, size, gap), got, im.size))
        if plan is None:
            assert api.thumbnail_size((w, h), size) is None or api.thumbnail_size((w, h), size) == (w, h)
    assert not bad, bad[:10]


def test_plan_reduce_matches_pillow():
    """Reduce factors and the safe box the plan picks are the ones Image.resize hands Image.reduce."""
    seen = []
    orig = Image.Image.reduce

    def spy(self, factor, box=None):
        seen.append((tuple(factor), tuple(box)))
        return orig(self, factor, box)

    Image.Image.reduce = spy
    reduced = 0
    try:
        for w, h, size, gap in CASES[::15]:
            seen.clear()
            im = Image.new("L", (w, h))
            im.thumbnail(size, Image.Resampling.LANCZOS, gap)
            plan = lars.thumbnail_plan((w, h), size, gap)
            if plan is None or plan.factor == (1, 1):
                assert seen == [], (w, h, size, gap)
            else:
                assert seen == [(plan.factor, plan.reduce_box)], (w, h, size, gap, plan)
                reduced += 1
    finally:
        Image.Image.reduce = orig
    assert reduced > 20


def test_plan_known_cases():
    p = lars.thumbnail_plan((2048, 1536))
    assert p == api.ThumbnailPlan((400, 300), (2, 2), (0, 0, 2048, 1536), (0.0, 0.0, 1024.0, 768.0), False, False)
    # a box Pillow's C code holds as float32: 2999 / 3 rounded to float, not the float64 quotient
    p = lars.thumbnail_plan((2999, 2999))
    assert p.factor == (3, 3) and p.box[2] == float(np.float32(2999 / 3)) != 2999 / 3
    # Image.resize's tall-image branch: more than 100 times as tall as wide
    assert lars.thumbnail_plan((7, 900)).vertical_first and not lars.thumbnail_plan((900, 7)).vertical_first
    # RGBA: premultiplied, no reduce
    p = lars.thumbnail_plan((2048, 1536), rgba=True)
    assert p.premultiply and p.factor == (1, 1) and p.box == (0.0, 0.0, 2048.0, 1536.0)
    assert lars.thumbnail_plan((2048, 1536), reducing_gap=None).factor == (1, 1)
    # a JPEG draft: decoded at half size, fractional box
    p = lars.thumbnail_plan((3333, 2001), draft_box=(0, 0, 1666.5, 1000.5), image_size=(1667, 1001))
    assert p.size == (400, 240) and p.factor == (2, 2) and p.reduce_box == (0, 0, 1667, 1001)
    assert p.box == (0.0, 0.0, 833.25, 500.25)
    # drafted straight to the final size: nothing left to do
    assert lars.thumbnail_plan((800, 800), (100, 100), 1.0, (0, 0, 100.0, 100.0), (100, 100)) is None


def test_reducing_gap_below_one_raises():
    with pytest.raises(ValueError, match="reducing_gap"):
        lars.thumbnail_plan((2048, 1536), reducing_gap=0.5)
    with pytest.raises(ValueError, match="reducing_gap"):
        lars.thumbnail(np.zeros((600, 500, 3), np.uint8), reducing_gap=0.99)
    with pytest.raises(ValueError):
        Image.new("RGB", (500, 600)).thumbnail((400, 400), Image.Resampling.LANCZOS, 0.99)


@pytest.mark.parametrize("mode", ["P", "1", "LA", "I;16", "I", "F", "CMYK", "RGBa", "YCbCr"])
def test_unsupported_pil_modes_raise_type_error(mode):
    im = Image.new(mode, (900, 700))
    with pytest.raises(TypeError, match=mode.replace(";", ".")):
        lars.thumbnail(im)
    small = Image.new(mode, (10, 10))
    with pytest.raises(TypeError):
        lars.thumbnail(small)


@pytest.mark.parametrize("arr", [np.zeros((900, 700), np.uint16), np.zeros((900, 700, 3), np.float32),
                                 np.zeros((900, 700, 2), np.uint8), np.zeros((900, 700, 1), np.uint8),
                                 np.zeros((900, 700, 5), np.uint8), np.zeros((4, 900, 700), np.int8)])
def test_unsupported_arrays_raise_type_error(arr):
    with pytest.raises(TypeError):
        lars.thumbnail(arr)


def _no_gpu(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("reached the C library")
    monkeypatch.setattr(_ffi, "call", refuse)


@pytest.mark.parametrize("shape", [(400, 400, 3), (300, 200), (1, 1, 4), (399, 12, 3)])
def test_image_that_fits_is_returned_as_is(monkeypatch, shape):
    _no_gpu(monkeypatch)
    arr = np.ones(shape, np.uint8)
    assert lars.thumbnail(arr) is arr
    pil = Image.fromarray(arr)
    assert lars.thumbnail(pil) is pil
    assert lars.thumbnail(arr, (shape[1], shape[0])) is arr


def test_jpeg_drafted_to_final_size_is_returned_as_is(monkeypatch):
    _no_gpu(monkeypatch)
    buf = io.BytesIO()
    Image.fromarray(np.full((800, 800, 3), 90, np.uint8)).save(buf, "JPEG")
    im = Image.open(io.BytesIO(buf.getvalue()))
    ref = Image.open(io.BytesIO(buf.getvalue()))
    ref.thumbnail((100, 100), Image.Resampling.LANCZOS, 1.0)
    assert lars.thumbnail(im, (100, 100), 1.0) is im
    assert im.size == ref.size == (100, 100)


def test_entry_point_receives_the_plan(monkeypatch):
    """A JPEG source is drafted as Pillow drafts it, and lars_h_thumbnail_u8 gets the plan's numbers and shapes."""
    got = {}

    def capture(name, *args):
        got["name"], got["args"] = name, args
        return 0

    monkeypatch.setattr(_ffi, "call", capture)
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(3).integers(0, 256, (2001, 3333, 3), dtype=np.uint8)).save(buf, "JPEG")
    im = Image.open(io.BytesIO(buf.getvalue()))
    out = lars.thumbnail(im)
    assert isinstance(out, Image.Image) and out.mode == "RGB" and out.size == (400, 240)
    assert im.size == (1667, 1001)                                  # drafted in place, as Pillow does
    name, a = got["name"], got["args"]
    assert name == "lars_h_thumbnail_u8"
    assert (a[1], a[2], a[3], a[4], a[5]) == (1001, 1667, 3, 2, 2)
    assert list(a[6]) == [0, 0, 1667, 1001] and list(a[7]) == [0.0, 0.0, 833.25, 500.25]
    assert (a[8], a[9], a[10]) == (240, 400, 0)

    out = lars.thumbnail(np.zeros((900, 7), np.uint8))
    assert out.shape == (400, 3) and out.dtype == np.uint8
    a = got["args"]
    assert (a[1], a[2], a[3], a[4], a[5], a[10]) == (900, 7, 1, 1, 1, 1)
    out = lars.thumbnail(np.zeros((1536, 2048, 4), np.uint8), (128, 128))
    assert out.shape == (96, 128, 4)
    assert (got["args"][3], got["args"][4], got["args"][5]) == (4, 1, 1)


def test_exported():
    assert "thumbnail" in api.__all__ and lars.thumbnail is api.thumbnail


@pytest.mark.skipif(_ffi.device_count() > 0, reason="only meaningful without a GPU")
def test_thumbnail_has_no_cpu_fallback():
    for img in (np.zeros((900, 700, 3), np.uint8), Image.new("L", (900, 700)), Image.new("RGBA", (900, 700))):
        with pytest.raises(_ffi.LarsError) as e:
            lars.thumbnail(img)
        assert e.value.code == -2 and "no CPU fallback" in str(e.value)
