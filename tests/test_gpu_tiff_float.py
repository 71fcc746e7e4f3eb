"""Float32 TIFF on the device: decode_tiff against tiffio.read_tiff on every layout of write_float_tiff and on Pillow's files,
encode_tiff_f32 against the greedy encoder on the model's bytes (libtiff's strips), against write_float_tiff's directory and
against every reader, process_image(want_tiff=...) and the directory driver against calculate_index.  No tolerance anywhere:
equality is on the 32-bit patterns, NaN payloads, infinities, denormals and -0.0 included."""
import ctypes as C
import io
import struct

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
import lzw_writer as lz
import tiff_float_model as fm
from lars_image_processing_amd import _ffi, driver, tiffio
from test_tiff_encode_cpu import directory
from test_tiff_float_cpu import pillow_file, same_bits, written

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 15, 16, 17, 63, 64, 65, 129)
HEIGHTS = (1, 2, 9)
SAMPLES = (1, 2, 3, 5)
KINDS = ("bits", "smooth", "constant")


def picture(kind, h, w, c, seed):
    return fm.values(kind, (h, w) if c == 1 else (h, w, c), seed)


def check_decode(blob, a, deflate=False):
    want = tiffio.read_tiff(blob)
    same_bits(want, a)
    same_bits(lars.decode_tiff(blob, deflate=True) if deflate else lars.decode_tiff(blob), want)


@pytest.mark.parametrize("predictor", [1, 2, 3])
@pytest.mark.parametrize("lzw", [False, True])
def test_decode_strips_every_width_and_sample_count(lzw, predictor):
    """Every width with every sample count; height, rows per strip (1, 4, all), chunky / planar, byte order and the kind of
    values rotate on counters of different periods, so that each value of each meets each width and each sample count."""
    n = 0
    for w in WIDTHS:
        for c in SAMPLES:
            for rps in (1, 4, None):
                h = HEIGHTS[(n // 2) % 3]
                a = picture(KINDS[n % 3], h, w, c, seed=n)
                blob = written(a, rows_per_strip=rps, planar=1 + n % 2, byteorder="<>"[(n // 3) % 2], lzw=lzw, predictor=predictor)
                check_decode(blob, a)
                n += 1


@pytest.mark.parametrize("predictor", [1, 2, 3])
@pytest.mark.parametrize("shape, tile", [((21, 19), (16, 16)), ((50, 70), (32, 48))])
def test_decode_tiles_cropped_right_and_bottom(shape, tile, predictor):
    """The right and bottom tiles are cropped; with predictor 3 their padding columns lie between the byte planes and take
    part in the running sum."""
    n = 0
    for c in SAMPLES:
        for planar in (1, 2):
            for lzw in (False, True):
                a = picture(KINDS[n % 2], shape[0], shape[1], c, seed=n)
                check_decode(written(a, tile=tile, planar=planar, byteorder="<>"[(n // 2 + c) % 2], lzw=lzw, predictor=predictor), a)
                n += 1


def test_decode_padding_that_is_not_zero():
    """A tile whose padding columns hold noise: with predictor 3 the sums run through them and nothing of them comes out."""
    a = picture("bits", 21, 19, 3, seed=5)
    wide = picture("bits", 32, 32, 3, seed=6)
    wide[:21, :19] = a
    for lzw in (False, True):
        for predictor in (1, 2, 3):
            blob = bytearray(written(wide, tile=(16, 16), lzw=lzw, predictor=predictor))
            # the same tiles under a directory that says 21 x 19: ImageWidth and ImageLength are the first two entries
            (ifd,) = struct.unpack_from("<I", blob, 4)
            assert struct.unpack_from("<H", blob, ifd + 2)[0] == tiffio.IMAGE_WIDTH
            struct.pack_into("<I", blob, ifd + 2 + 8, 19)
            struct.pack_into("<I", blob, ifd + 14 + 8, 21)
            # 2 x 2 tiles stay 2 x 2 tiles
            check_decode(bytes(blob), a)


def test_decode_deflate_files():
    n = 0
    for layout in ({"rows_per_strip": 4}, {"tile": (16, 16)}):
        for predictor in (1, 2, 3):
            for c, planar in ((1, 1), (3, 2), (5, 1)):
                a = picture(KINDS[n % 2], 21, 19, c, seed=n)
                blob = written(a, deflate=True, predictor=predictor, planar=planar, byteorder="<>"[n % 2], **layout)
                with pytest.raises(NotImplementedError, match="Deflate"):
                    lars.decode_tiff(blob)
                check_decode(blob, a, deflate=True)
                n += 1


def test_decode_pillow_files():
    for kind, shape in (("bits", (33, 47)), ("smooth", (70, 90)), ("constant", (9, 300)), ("bits", (1, 1)), ("smooth", (200, 129))):
        a = fm.values(kind, shape, seed=1)
        for predictor in (1, 2, 3):
            blob = pillow_file(a, "tiff_lzw", predictor)
            check_decode(blob, a)
            same_bits(lars.decode_tiff(blob), np.asarray(Image.open(io.BytesIO(blob))))
            check_decode(pillow_file(a, "tiff_adobe_deflate", predictor), a, deflate=True)
        check_decode(pillow_file(a), a)


def test_damaged_strips_raise_as_for_integer_files():
    a = picture("smooth", 12, 40, 1, seed=2)
    good = written(a, rows_per_strip=4, lzw=True, predictor=3)
    tags = tiffio._read_ifd(memoryview(good), "<")
    off, cnt = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]      # the second of three strips
    want_bytes = 4 * 40 * 4
    for stream, message in ((lz.pack([lz.CLEAR, 65, 400]), "corrupt"), (lz.pack([lz.CLEAR, 65, 66, lz.EOI]), f"holds 2 bytes, {want_bytes} expected")):
        assert len(stream) <= cnt
        bad = bytearray(good)
        bad[off:off + cnt] = stream + bytes(cnt - len(stream))
        with pytest.raises(tiffio.TiffError, match=message) as host:
            tiffio.read_tiff(bytes(bad))
        with pytest.raises(tiffio.TiffError, match=message) as dev:
            lars.decode_tiff(bytes(bad))
        if "expected" in message:
            assert str(host.value) in str(dev.value)
        check_decode(good, a)                                           # the status was reset
    # an uncompressed strip shorter than its rows: the directory is refused before anything is launched
    raw = written(a, rows_per_strip=4, predictor=3)
    with pytest.raises(tiffio.TiffError):
        lars.decode_tiff(raw[:len(raw) // 2])
    with pytest.raises(TypeError, match="thumbnail_tiff: 8-bit TIFF files"):
        lars.thumbnail_tiff(good, size=(4, 4))


SKIPPED_TAGS = (tiffio.COMPRESSION, tiffio.STRIP_OFFSETS, tiffio.STRIP_BYTE_COUNTS)


def check_encode(a, rps=None, predictor=False, strip_bytes=65536):
    """Everything the issue asks of one file; returns (the file, the streams' codes per strip)."""
    blob = lars.encode_tiff_f32(a, rows_per_strip=rps, predictor=predictor)
    assert isinstance(blob, bytes)
    a3 = a.reshape(a.shape[0], a.shape[1], -1)
    h, w, c = a3.shape
    rows = min(rps, h) if rps else min(h, max(1, strip_bytes // (w * c * 4)))
    tags, ifd = directory(blob)
    want, _ = directory(written(a, rows_per_strip=rows, predictor=3 if predictor else 1))
    assert list(tags) == list(want) == sorted(want)
    for tag in want:
        if tag not in SKIPPED_TAGS:
            assert tags[tag] == want[tag], tag
    assert tags[tiffio.COMPRESSION] == (3, (5,)) and tags[tiffio.ROWS_PER_STRIP] == (4, (rows,))
    assert tags[tiffio.BITS_PER_SAMPLE] == (3, (32,) * c) and tags[tiffio.SAMPLE_FORMAT] == (3, (3,) * c)
    assert (tags[tiffio.PREDICTOR] == (3, (3,))) if predictor else (tiffio.PREDICTOR not in tags)
    offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
    assert len(offsets) == len(counts) == -(-h // rows)
    at, all_codes = 8, []
    for k, (o, n) in enumerate(zip(offsets, counts)):
        assert o == at and o % 2 == 0, k
        at += n + (n & 1)
        codes = lz.encode(fm.strip_bytes(a3, k * rows, rows, predictor), clear_at=4094)
        assert blob[o:o + n] == lz.pack(codes), (k, a.shape, rps, predictor)
        assert n % 2 == 0 or blob[o + n] == 0
        all_codes.append(codes)
    assert at == ifd and len(blob) <= lars.tiff_f32_bound(h, w, c, rps)
    shape = a.shape[:2] if c == 1 else a.shape
    for back in (tiffio.read_tiff(blob), lars.decode_tiff(blob)):
        same_bits(back, a.reshape(shape))
    if c == 1:
        same_bits(np.asarray(Image.open(io.BytesIO(blob))), a.reshape(shape))
        pil = pillow_file(a.reshape(shape), "tiff_lzw", 3 if predictor else 1)
        ptags = tiffio._read_ifd(memoryview(pil), "<")
        if min(ptags[tiffio.ROWS_PER_STRIP][0], h) == rows:              # at equal rows per strip: Pillow's (libtiff's) bytes
            for o, n, po, pn in zip(offsets, counts, ptags[tiffio.STRIP_OFFSETS], ptags[tiffio.STRIP_BYTE_COUNTS]):
                assert blob[o:o + n] == pil[po:po + pn]
    return blob, all_codes


@pytest.mark.parametrize("predictor", [False, True])
@pytest.mark.parametrize("c", SAMPLES)
def test_encode_every_width(c, predictor):
    n = 0
    for w in WIDTHS:
        for rps in (1, 4, None):
            check_encode(picture(KINDS[n % 3], HEIGHTS[(n // 2) % 3], w, c, seed=n + c), rps, predictor)
            n += 1
    if c == 1:
        check_encode(picture("smooth", 9, 17, 1, 0)[..., None], 4, predictor)     # [H, W, 1] is the same file


@pytest.mark.parametrize("predictor", [False, True])
def test_encode_equals_pillow_strips(predictor):
    """Pillow's default strips are the library's (the most rows within 64 KiB), so whole files compare strip by strip."""
    for kind, shape in (("smooth", (70, 90)), ("bits", (33, 47)), ("constant", (100, 300)), ("smooth", (300, 129))):
        a = fm.values(kind, shape, seed=4)
        blob, _ = check_encode(a, None, predictor)
        pil = pillow_file(a, "tiff_lzw", 3 if predictor else 1)
        ptags = tiffio._read_ifd(memoryview(pil), "<")
        tags, _ = directory(blob)
        assert min(ptags[tiffio.ROWS_PER_STRIP][0], shape[0]) == tags[tiffio.ROWS_PER_STRIP][1][0]
        assert tuple(ptags[tiffio.STRIP_BYTE_COUNTS]) == tags[tiffio.STRIP_BYTE_COUNTS][1]


@pytest.mark.parametrize("predictor", [False, True])
def test_encode_one_strip_of_noise_with_a_table_clear(predictor):
    a = fm.values("bits", (40, 40), seed=7)
    _, (codes,) = check_encode(a, 40, predictor)
    assert codes.count(lz.CLEAR) >= 2                                     # the leading one and at least one of a full table
    i, widths = 0, set()
    for code in codes:
        widths.add(lz.width_of(i))
        i = 0 if code == lz.CLEAR else i + 1
    assert widths == {9, 10, 11, 12}


def test_encode_follows_the_strip_knob():
    a = picture("smooth", 64, 100, 1, seed=8)
    with _ffi.tuning(tiff_strip_bytes=8192):
        check_encode(a, None, True, strip_bytes=8192)                     # 20 rows
    with _ffi.tuning(tiff_strip_bytes=100):
        check_encode(a, None, False, strip_bytes=100)                     # less than a row: one row per strip
    check_encode(a, None, True)


def test_encode_too_small_out_cap_gives_nospace_and_the_needed_length():
    a = np.ascontiguousarray(picture("smooth", 40, 60, 1, seed=9))
    blob = lars.encode_tiff_f32(a, rows_per_strip=16, predictor=True)
    d_img, d_out = _ffi.DeviceBuffer(a.nbytes), _ffi.DeviceBuffer(len(blob))
    d_scr = _ffi.DeviceBuffer(_ffi.load().lars_tiff_f32_encode_scratch_bytes(40, 60, 1, 16))
    d_ans = _ffi.DeviceBuffer(16)                                         # int64 length, int32 status[2]
    try:
        d_img.upload(a)
        for cap, want_status in ((len(blob) - 1, 1), (len(blob), 0), (0, 1)):
            _ffi.call("lars_d_encode_tiff_f32", C.c_void_p(d_img.ptr), 40, 60, 1, 16, 1, C.c_void_p(d_out.ptr), cap, C.c_void_p(d_ans.ptr),
                      C.c_void_p(d_ans.ptr + 8), C.c_void_p(d_scr.ptr), None)
            _ffi.call("lars_synchronize", None)
            assert int(d_ans.download(np.int64, (1,))[0]) == len(blob)
            assert d_ans.download(np.int32, (2,), offset=8).tolist() == [want_status, 0]   # LARS_TIFE_NOSPACE = 1
            if want_status == 0:
                assert d_out.download(np.uint8, (len(blob),)).tobytes() == blob
    finally:
        for b in (d_img, d_out, d_scr, d_ans):
            b.free()
    out = np.zeros(len(blob), np.uint8)
    n = C.c_int64(-7)
    with pytest.raises(_ffi.LarsError) as e:
        _ffi.call("lars_h_encode_tiff_f32", _ffi.ptr(a), 40, 60, 1, 16, 1, _ffi.ptr(out), len(blob) - 1, C.byref(n))
    assert e.value.code == -1 and f"the file needs {len(blob)} bytes, out_cap is {len(blob) - 1} (device status 1)" in str(e.value)
    assert lars.encode_tiff_f32(a, rows_per_strip=16, predictor=True) == blob


def rgnir(h, w, seed):
    rng = np.random.default_rng(seed)
    base = (np.add.outer(np.arange(h), 2 * np.arange(w))[..., None] * np.array([3, 5, 7])) % 256
    return np.where(rng.random((h, w, 1)) < 0.3, rng.integers(0, 256, (h, w, 3)), base).astype(np.uint8)


@pytest.fixture(scope="module")
def images():
    return {shape: rgnir(shape[0], shape[1], seed) for seed, shape in enumerate(((33, 47), (64, 64)))}


@pytest.mark.parametrize("white_balance", [False, True])
@pytest.mark.parametrize("shape", [(33, 47), (64, 64)])
def test_process_image_want_tiff(images, shape, white_balance):
    img = images[shape]
    ref = lars.process_image(img, white_balance=white_balance, want_hist=True)
    plain = lars.process_image(img, white_balance=white_balance, want_arrays=False, want_hist=True)      # the same call without want_tiff
    src = ref["corrected"] if white_balance else img
    for mode, tag in ((True, None), ("predictor", (3,))):
        got = lars.process_image(img, white_balance=white_balance, want_arrays=False, want_hist=True, want_tiff=mode)
        assert (got["corrected"] is None) if not white_balance else np.array_equal(got["corrected"], ref["corrected"])
        for t in lars.api.INDEX_NAMES:
            entry = got["indices"][t]
            assert entry["index"] is None and entry["png"] is None and isinstance(entry["tiff"], bytes)
            plane = lars.calculate_index(src, t)
            for back in (tiffio.read_tiff(entry["tiff"]), lars.decode_tiff(entry["tiff"]), np.asarray(Image.open(io.BytesIO(entry["tiff"])))):
                same_bits(back, plane)
            assert tiffio._read_ifd(memoryview(entry["tiff"]), "<").get(tiffio.PREDICTOR) == tag
            assert entry["tiff"] == lars.encode_tiff_f32(plane, predictor=mode == "predictor")
            for other in (plain, ref):
                assert entry["stats"] == other["indices"][t]["stats"] and np.array_equal(entry["hist"], other["indices"][t]["hist"])
            assert ref["indices"][t]["tiff"] is None
    # one index, with the plane and the colormap picture in the same call
    one = lars.process_image(img, indices=["GNDVI"], white_balance=white_balance, want_rgba=True, want_tiff="predictor")
    same_bits(one["indices"]["GNDVI"]["index"], lars.calculate_index(src, "GNDVI"))
    same_bits(tiffio.read_tiff(one["indices"]["GNDVI"]["tiff"]), one["indices"]["GNDVI"]["index"])
    assert np.array_equal(one["indices"]["GNDVI"]["rgba"], lars.colorize_index(one["indices"]["GNDVI"]["index"], "GNDVI"))


@pytest.mark.parametrize("png_encoder, lut_format", [("pillow", "png"), ("device", "png8"), ("pillow", "tiff")])
def test_driver_index_tiff(tmp_path, images, png_encoder, lut_format):
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(images[(33, 47)]).save(src / "field.png")
    kw = dict(process_wb=True, indices=["NDVI", "GNDVI", "NDWI"], lut_format=lut_format, png_encoder=png_encoder)
    stats_off = driver.process_image(src / "field.png", tmp_path / "off", **kw)
    stats_on = driver.process_image(src / "field.png", tmp_path / "on", index_tiff=True, **kw)
    assert stats_on == stats_off
    files_off = sorted(p.relative_to(tmp_path / "off") for p in (tmp_path / "off").rglob("*") if p.is_file())
    files_on = sorted(p.relative_to(tmp_path / "on") for p in (tmp_path / "on").rglob("*") if p.is_file())
    extra = sorted(set(files_on) - set(files_off))
    assert [str(p) for p in extra] == ["GNDVI/field_gndvi_f32.tif", "NDVI/field_ndvi_f32.tif", "NDWI/field_ndwi_f32.tif"]
    assert not any("_f32" in str(p) for p in files_off) and sorted(set(files_on) - set(extra)) == files_off
    for rel in files_off:
        assert (tmp_path / "on" / rel).read_bytes() == (tmp_path / "off" / rel).read_bytes(), rel
    corrected = lars.fix_white_balance(images[(33, 47)])
    for t in ("NDVI", "GNDVI", "NDWI"):
        blob = (tmp_path / "on" / t / f"field_{t.lower()}_f32.tif").read_bytes()
        same_bits(tiffio.read_tiff(blob), lars.calculate_index(corrected, t))
        assert tiffio._read_ifd(memoryview(blob), "<")[tiffio.PREDICTOR] == (3,)
    if lut_format == "png":                                               # the command line and batch_process hand the flag on
        assert driver.main([str(src), str(tmp_path / "cli"), "--wb", "--ndvi", "--gndvi", "--index-tiff", "--quiet", "--workers", "1"]) == 0
        for rel in files_on:
            assert (tmp_path / "cli" / rel).read_bytes() == (tmp_path / "on" / rel).read_bytes(), rel
