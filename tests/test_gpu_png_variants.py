"""decode_png / thumbnail_png with extended=True and png_decoder="device+extended" on the GPU: 1-, 2-, 4- and 16-bit and
Adam7-interlaced files.  Every array is compared with Pillow's of the same file in the same test: dtype, shape, values."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import tiffio

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_variant_writer as W  # noqa: E402

pytestmark = pytest.mark.gpu

# one (colour type, depth) per filter distance bpp = 1, 2, 3, 4, 6, 8
BPP_PAIRS = [(0, 2), (0, 16), (2, 8), (6, 8), (2, 16), (6, 16)]
# width at which that pair's rows take more than 2048 bytes (the unfilter tile), no multiple of 16
WIDE = [((3, 4), 4113), ((0, 16), 1029), ((4, 8), 1029), ((2, 8), 686), ((6, 8), 515), ((2, 16), 343), ((6, 16), 257), ((0, 1), 16450)]


def same(b, got=None):
    want = np.asarray(Image.open(io.BytesIO(b)))
    got = lars.decode_png(b, extended=True) if got is None else got
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want)
    return got


def smooth(rng, h, w, ctype, depth):
    """Samples with structure, so that the file compresses into many blocks as a photograph does."""
    c = W.CHANNELS[ctype]
    y, x = np.mgrid[0:h, 0:w]
    base = (np.sin(x / 37.0)[:, :, None] + np.cos(y / 23.0)[:, :, None] + np.arange(c) * 0.3 + 2.3) / 4.6
    v = base * ((1 << depth) - 1) + rng.integers(0, 3 if depth < 16 else 300, (h, w, c))
    return np.clip(v, 0, (1 << depth) - 1).astype(np.uint16 if depth == 16 else np.uint8)


@pytest.mark.parametrize("interlace", [False, True])
@pytest.mark.parametrize("ctype,depth", W.PAIRS)
def test_every_mode(ctype, depth, interlace):
    rng = np.random.default_rng(1000 * ctype + 10 * depth + interlace)
    for h, w in ((1, 1), (10, 33), (70, 3)):                               # 70 rows: past the 64-row group
        s = W.random_samples(rng, h, w, ctype, depth)
        same(W.write_png(s, ctype, depth, interlace, seed=h, idat_split=29 if h == 10 else None))


@pytest.mark.parametrize("interlace", [False, True])
@pytest.mark.parametrize("ctype,depth", BPP_PAIRS)
def test_every_small_size(ctype, depth, interlace):
    """1..9 x 1..9: every combination of empty Adam7 passes."""
    rng = np.random.default_rng(77 * ctype + depth)
    for h in range(1, 10):
        for w in range(1, 10):
            same(W.write_png(W.random_samples(rng, h, w, ctype, depth), ctype, depth, interlace, seed=9 * h + w))


@pytest.mark.parametrize("interlace", [False, True])
@pytest.mark.parametrize("pair,w", WIDE)
def test_rows_wider_than_a_tile(pair, w, interlace):
    ctype, depth = pair
    rng = np.random.default_rng(w)
    same(W.write_png(W.random_samples(rng, 5, w, ctype, depth), ctype, depth, interlace, seed=w))


@pytest.mark.parametrize("ctype,depth", [(0, 1), (2, 16)])
def test_tall_interlaced_file_wraps_the_waves(ctype, depth):
    """3 x 2100: pass 7 has 1050 rows, more than the 16 waves of 64 rows take in one turn."""
    rng = np.random.default_rng(2100 + depth)
    same(W.write_png(W.random_samples(rng, 2100, 3, ctype, depth), ctype, depth, True, seed=3))


@pytest.mark.parametrize("ftype", range(5))
@pytest.mark.parametrize("ctype,depth", [(3, 2), (2, 16), (6, 16)])         # bpp 1, 6, 8
def test_forced_filters(ctype, depth, ftype):
    rng = np.random.default_rng(10 * ftype + depth)
    s = W.random_samples(rng, 21, 37, ctype, depth)
    for interlace in (False, True):
        same(W.write_png(s, ctype, depth, interlace, filters=ftype))


def test_files_pillow_writes():
    rng = np.random.default_rng(12)

    def save(im, **kw):
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        return b.getvalue()
    g = rng.integers(0, 65536, (45, 67), dtype=np.uint16)
    b = save(Image.fromarray(g))
    assert Image.open(io.BytesIO(b)).mode == "I;16"
    assert np.array_equal(same(b), g)
    b = save(Image.fromarray(rng.integers(0, 2, (45, 67)).astype(bool)))
    assert Image.open(io.BytesIO(b)).mode == "1"
    same(b)
    for colours, bits in ((2, 1), (4, 2), (16, 4)):
        im = Image.fromarray(rng.integers(0, colours, (45, 67), dtype=np.uint8), "P")
        im.putpalette(bytes(rng.integers(0, 256, 3 * colours, dtype=np.uint8)))
        b = save(im, bits=bits)
        assert lars.png_info(b)["bit_depth"] == bits
        same(b)


@pytest.mark.parametrize("ctype,depth,interlace", [(0, 16, False), (2, 8, True)])
def test_realistic_size(ctype, depth, interlace):
    """2048 x 1536 I;16, and 2048 x 1536 RGB interlaced."""
    rng = np.random.default_rng(depth)
    s = smooth(rng, 1536, 2048, ctype, depth)
    same(W.write_png(s, ctype, depth, interlace, seed=1, level=1, idat_split=65536))


@pytest.mark.parametrize("ctype,depth,interlace", [(2, 8, True), (6, 16, False), (0, 4, False), (4, 16, True)])
def test_thumbnail_extended_matches_pillow(ctype, depth, interlace):
    rng = np.random.default_rng(ctype + depth)
    b = W.write_png(smooth(rng, 700, 900, ctype, depth), ctype, depth, interlace, seed=2, level=1)
    im = Image.open(io.BytesIO(b))
    im.thumbnail((400, 400), Image.Resampling.LANCZOS, 2.0)
    want = np.asarray(im)
    got = lars.thumbnail_png(b, (400, 400), 2.0, extended=True)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    # a file that already fits comes back as decode_png gives it
    small = W.write_png(W.random_samples(rng, 30, 40, ctype, depth), ctype, depth, interlace)
    same(small, lars.thumbnail_png(small, (400, 400), 2.0, extended=True))


def test_thumbnail_extended_refuses_other_modes():
    rng = np.random.default_rng(3)
    for ctype, depth in ((0, 1), (0, 16), (3, 4)):
        b = W.write_png(W.random_samples(rng, 500, 500, ctype, depth), ctype, depth, True, level=1)
        with pytest.raises(TypeError, match="mode"):
            lars.thumbnail_png(b, (400, 400), extended=True)


def test_bad_filter_byte_in_a_late_pass():
    rng = np.random.default_rng(4)
    s = W.random_samples(rng, 40, 40, 2, 16)
    b = W.write_png(s, 2, 16, True, filters=lambda p, r: 5 if (p, r) == (6, 3) else 1)
    with pytest.raises(ValueError, match="bad filter byte in row 3 of pass 6"):
        lars.decode_png(b, extended=True)
    b = W.write_png(s[:, :, :1], 0, 16, False, filters=lambda p, r: 200 if r == 17 else 4)
    with pytest.raises(ValueError, match="bad filter byte in row 17"):
        lars.decode_png(b, extended=True)
    same(W.write_png(s, 2, 16, True, filters=1))                           # and the decoder works after both


def test_interlaced_stream_one_byte_short():
    rng = np.random.default_rng(5)
    s = W.random_samples(rng, 20, 23, 0, 4)
    raw = W.filtered_stream(s, 0, 4, True)
    b = W.write_png(s, 0, 4, True, stream=raw[:-1])
    with pytest.raises(ValueError, match=f"too few decoded bytes \\({len(raw) - 1}\\)"):
        lars.decode_png(b, extended=True)
    same(W.write_png(s, 0, 4, True, stream=raw))


@pytest.mark.parametrize("ctype", [0, 2, 3, 4, 6])
def test_eight_bit_files_are_the_same_either_way(ctype):
    rng = np.random.default_rng(ctype)
    for h, w in ((1, 1), (70, 45), (300, 700)):
        b = W.write_png(W.random_samples(rng, h, w, ctype, 8), ctype, 8, False, seed=h, level=1)
        got = same(b)
        plain = lars.decode_png(b)
        assert plain.dtype == got.dtype and plain.shape == got.shape and np.array_equal(plain, got)


def test_read_image_device_extended(tmp_path):
    rng = np.random.default_rng(6)
    f = tmp_path / "band.png"
    f.write_bytes(W.write_png(W.random_samples(rng, 130, 170, 0, 16), 0, 16, False))
    want = np.array(Image.open(f))
    assert want.dtype == np.uint16
    for full_depth in (True, False):
        got = tiffio.read_image(f, full_depth=full_depth, png_decoder="device+extended")
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    g = tmp_path / "adam.png"
    g.write_bytes(W.write_png(W.random_samples(rng, 130, 170, 2, 8), 2, 8, True))
    assert np.array_equal(tiffio.read_image(g, png_decoder="device+extended"), np.array(Image.open(g)))
