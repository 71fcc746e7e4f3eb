"""encode_tiff / encode_tiff_f32 with compression="deflate" on the device.  Every strip of every file must be, byte for byte, the
stream tests/tiff_deflate_encode_model.py builds for the strip's stored bytes; the directory must be tiffio.write_tiff's (or
write_float_tiff's) with deflate=True, but for StripOffsets and StripByteCounts; tiffio.read_tiff, lars.decode_tiff(...,
deflate=True) and, where it reads the layout as stored, Pillow must give the array back bit for bit.  No tolerance anywhere."""
import io
import threading
import zlib

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
import tiff_deflate_encode_model as dm
from lars_image_processing_amd import _ffi, driver, tiffio
from test_gpu_tiff_decode import one_over_f, sample

pytestmark = pytest.mark.gpu

SKIPPED_TAGS = (tiffio.STRIP_OFFSETS, tiffio.STRIP_BYTE_COUNTS)
SEG = dm.SEG


def check(a, rps=None, predictor=False, strip_bytes=65536):
    """Everything the issue asks of one file; returns (the file, the stored bytes per strip, the streams)."""
    f32 = a.dtype == np.float32
    if f32:
        blob = lars.encode_tiff_f32(a, rows_per_strip=rps, predictor=predictor, compression="deflate")
    else:
        blob = lars.encode_tiff(a, rows_per_strip=rps, predictor=predictor, compression="deflate")
    assert isinstance(blob, bytes)
    a3 = a.reshape(a.shape[0], a.shape[1], -1)
    h, w, c = a3.shape
    rows = min(rps, h) if rps else min(h, max(1, strip_bytes // (w * c * a.dtype.itemsize)))
    strips, want, _ = dm.stored_strips(a, rows, predictor)
    tags, ifd, _ = dm.directory(blob)
    assert list(tags) == list(want) == sorted(want)
    for tag in want:
        if tag not in SKIPPED_TAGS:
            assert tags[tag] == want[tag], tag
    assert tags[tiffio.COMPRESSION] == (3, (8,)) and tags[tiffio.ROWS_PER_STRIP] == (4, (rows,))
    offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
    assert len(offsets) == len(counts) == len(strips) == -(-h // rows)
    at, streams = 8, []
    for k, (o, n) in enumerate(zip(offsets, counts)):
        assert o == at and o % 2 == 0, k
        at += n + (n & 1)
        stream = dm.strip_stream(strips[k])
        assert blob[o:o + n] == stream, (k, a.shape, rps, predictor)
        assert n % 2 == 0 or blob[o + n] == 0
        streams.append(stream)
    assert at == ifd
    bound = lars.tiff_f32_bound(h, w, c, rps, compression="deflate") if f32 else lars.tiff_bound(h, w, c, a.dtype.itemsize, rps, compression="deflate")
    assert len(blob) <= bound
    shape = a.shape[:2] if c == 1 else a.shape           # the readers give [H, W] for one sample, also for a [H, W, 1] array
    for back in (tiffio.read_tiff(blob), lars.decode_tiff(blob, deflate=True)):
        assert back.dtype == a.dtype and back.shape == shape and back.tobytes() == a.tobytes()
    if c == 1 or (c == 3 and a.dtype == np.uint8):       # Pillow: not four samples with unspecified extras, not 16-bit RGB, one float band
        pil = np.asarray(Image.open(io.BytesIO(blob)))
        assert pil.dtype == a.dtype and pil.shape == shape and pil.tobytes() == a.tobytes()
    return blob, strips, streams


def forms(stream, n):
    """BTYPE of every part of a strip's stream of n stored bytes, by walking the model's parts."""
    out, at, data = [], 2, zlib.decompress(stream)
    for i in range(0, n, SEG):
        part = dm.part(data[i:i + SEG], i + SEG >= n)
        out.append((part[0] >> 1) & 3)
        at += len(part)
    assert at + 4 == len(stream)
    return out


def test_one_pixel():
    blob, _, (stream,) = check(np.array([[200]], np.uint8))
    assert len(stream) == 2 + 6 + 4                       # a stored block of one byte
    check(np.array([[200]], np.uint8), None, True)


@pytest.mark.parametrize("predictor", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_small_pictures_every_sample_count(dtype, predictor):
    for c in range(1, 6):
        a = sample(dtype, 37, 53, c, seed=10 * c + predictor)
        for rps in (1, 7, None):                          # 7: the last strip holds 2 rows; None: one strip of 37
            check(a, rps, predictor)
        if c == 1:
            check(a[..., None], 7, predictor)             # [H, W, 1] is the same file


def smooth(h, w, seed):
    return np.clip(np.random.default_rng(seed).normal(128, 6, (h, w)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("n", [32767, 32768, 32769, 65536, 65537])
def test_strips_at_the_part_border(n):
    """Strips of exactly n stored bytes (one row each), and a shorter last strip (rows_per_strip 2 of 3 rows)."""
    a = smooth(3, n, n)
    _, _, streams = check(a, 1)
    assert forms(streams[0], n)[0] == 2 and len(forms(streams[0], n)) == -(-n // SEG)      # dynamic blocks (a last part of one byte is stored)
    check(a, 2)
    check(a, 2, True)


def test_stored_parts_first_middle_and_last():
    rng = np.random.default_rng(21)
    a = np.concatenate([rng.integers(0, 256, (1, 3 * SEG + 100), dtype=np.uint8),                       # stored, stored, stored, stored
                        np.concatenate([smooth(1, SEG, 1), rng.integers(0, 256, (1, SEG), dtype=np.uint8), smooth(1, SEG + 100, 2)], axis=1),
                        np.concatenate([rng.integers(0, 256, (1, SEG), dtype=np.uint8), smooth(1, SEG, 3), rng.integers(0, 256, (1, SEG + 100), dtype=np.uint8)],
                                       axis=1)])
    _, _, streams = check(a, 1)
    n = 3 * SEG + 100
    assert forms(streams[0], n) == [0, 0, 0, 0] and forms(streams[1], n)[:2] == [2, 0] and forms(streams[2], n) == [0, 2, 0, 0]


def test_one_symbol_strips_and_adler_across_parts():
    _, _, (stream,) = check(np.full((1, 5000), 77, np.uint8))           # every byte equal: a code of one literal and end-of-block
    assert forms(stream, 5000) == [2]
    _, strips, (stream,) = check(np.full((16, 1 << 16), 0xFF, np.uint8), 16)      # 2^20 bytes of 0xFF in one strip: 32 parts
    assert len(strips[0]) == 1 << 20 and stream[-4:] == zlib.adler32(strips[0]).to_bytes(4, "big")
    check(np.full((384, 512), 77, np.uint8), None, True)


def test_a_stream_of_odd_length_gets_its_pad_byte():
    odd = 0
    for w in range(700, 712):
        a = smooth(3, w, w)
        blob, _, streams = check(a, 1)
        odd += sum(len(s) & 1 for s in streams)
    assert odd >= 3                                       # check() saw pad bytes (and that they are 0)


def test_more_parts_than_a_workgroup_has_threads():
    rng = np.random.default_rng(22)
    a = (rng.normal(0, 1, (1, 2_400_000)).cumsum(axis=1) / 100).astype(np.float32)      # 9 600 000 bytes in one strip: 293 parts
    blob, strips, _ = check(a, 1)
    assert len(strips) == 1 and -(-len(strips[0]) // SEG) == 293


def floats(h, w, c, seed):
    """Smooth values with every special kind sprinkled in: NaNs with payloads, +-0, infinities, denormals."""
    rng = np.random.default_rng(seed)
    a = (np.add.outer(np.arange(h), np.arange(w))[..., None] / 37 + rng.normal(0, 0.01, (h, w, c))).astype(np.float32)
    bits = a.view(np.uint32).reshape(-1)
    special = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF,
                        0x00400000], np.uint32)
    where = rng.choice(bits.size, min(bits.size, 4 * special.size), replace=False)
    bits[where] = special[np.arange(where.size) % special.size]
    return a if c > 1 else a[..., 0]


@pytest.mark.parametrize("predictor", [False, True])
def test_float32_with_special_values(predictor):
    for c in (1, 2, 3, 5):
        for rps in (1, 4, None):
            check(floats(9, 65, c, seed=c), rps, predictor)
    check(floats(130, 257, 1, seed=9), None, predictor)   # strips of 63 rows: two parts each, the last strip shorter


def test_default_strips_follow_the_knob():
    a = one_over_f(np.random.default_rng(10), 64, 100, 3)
    before = _ffi.get_tuning("tiff_strip_bytes")
    with _ffi.tuning(tiff_strip_bytes=8192):
        check(a, None, False, strip_bytes=8192)           # 27 rows
    b = smooth(40, 9000, 4)
    with _ffi.tuning(tiff_strip_bytes=262144):
        check(b, None, True, strip_bytes=262144)          # 29 rows: eight parts per strip
    check(a)
    assert _ffi.get_tuning("tiff_strip_bytes") == before


def rgnir(h, w, seed):
    rng = np.random.default_rng(seed)
    base = (np.add.outer(np.arange(h), 2 * np.arange(w))[..., None] * np.array([3, 5, 7])) % 256
    return np.where(rng.random((h, w, 1)) < 0.3, rng.integers(0, 256, (h, w, 3)), base).astype(np.uint8)


def test_process_image_want_tiff_deflate():
    img = rgnir(96, 160, 5)
    ref = lars.process_image(img, white_balance=True, want_hist=True)
    for mode, predictor in (("deflate+predictor", True), ("deflate", False)):
        got = lars.process_image(img, white_balance=True, want_hist=True, want_tiff=mode)
        assert np.array_equal(got["corrected"], ref["corrected"])
        for t in lars.api.INDEX_NAMES:
            entry = got["indices"][t]
            plane = entry["index"]
            assert plane.tobytes() == ref["indices"][t]["index"].tobytes() and entry["stats"] == ref["indices"][t]["stats"]
            assert entry["tiff"] == lars.encode_tiff_f32(plane, predictor=predictor, compression="deflate")
            tags, _, _ = dm.directory(entry["tiff"])
            assert tags[tiffio.COMPRESSION] == (3, (8,)) and (tags.get(tiffio.PREDICTOR) == (3, (3,))) == predictor
            assert tiffio.read_tiff(entry["tiff"]).tobytes() == plane.tobytes()
    lzw = lars.process_image(img, white_balance=True, want_tiff="predictor")         # the call as it was
    assert lzw["indices"]["NDVI"]["tiff"] == lars.encode_tiff_f32(lzw["indices"]["NDVI"]["index"], predictor=True)


def test_driver_device_deflate(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(one_over_f(np.random.default_rng(14), 90, 120, 3)).save(src / "field.png")
    kw = dict(process_wb=True, indices=["NDVI", "NDWI"], lut_format="tiff", index_tiff=True)
    for enc in ("device", "device+deflate"):
        driver.process_image(src / "field.png", tmp_path / enc, tiff_encoder=enc, **kw)
    rels = ("white_balanced/field_wb.tif", "NDVI/field_ndvi.tif", "NDWI/field_ndwi.tif", "NDVI/field_ndvi_f32.tif", "NDWI/field_ndwi_f32.tif")
    for rel in rels:
        a, b = tiffio.read_tiff(str(tmp_path / "device" / rel)), tiffio.read_tiff(str(tmp_path / "device+deflate" / rel))
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), rel
        assert dm.directory((tmp_path / "device" / rel).read_bytes())[0][tiffio.COMPRESSION] == (3, (5,))
        tags = dm.directory((tmp_path / "device+deflate" / rel).read_bytes())[0]
        assert tags[tiffio.COMPRESSION] == (3, (8,)) and (tags.get(tiffio.PREDICTOR) == (3, (3,))) == rel.endswith("_f32.tif")
    assert driver.main([str(src), str(tmp_path / "cli"), "--wb", "--ndvi", "--lut-format", "tiff", "--tiff-encoder", "device+deflate",
                        "--index-tiff", "--quiet", "--workers", "1"]) == 0
    for rel in rels:
        assert (tmp_path / "cli" / rel).read_bytes() == (tmp_path / "device+deflate" / rel).read_bytes()


def test_two_threads_encode_at_once():
    rng = np.random.default_rng(13)
    pics = [one_over_f(rng, 190, 200, 3), floats(120, 301, 1, seed=3)]
    encode = [lambda: lars.encode_tiff(pics[0], rows_per_strip=60, predictor=True, compression="deflate"),
              lambda: lars.encode_tiff_f32(pics[1], predictor=True, compression="deflate")]
    want = [f() for f in encode]
    got, errors = [None] * 2, []

    def work(k):
        try:
            for _ in range(4):
                got[k] = encode[k]()
                assert got[k] == want[k]
        except Exception as exc:                          # noqa: BLE001
            errors.append((k, exc))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == want
    assert tiffio.read_tiff(want[0]).tobytes() == pics[0].tobytes() and tiffio.read_tiff(want[1]).tobytes() == pics[1].tobytes()


def test_defaults_are_unchanged():
    a = one_over_f(np.random.default_rng(15), 70, 90, 3)
    blob = lars.encode_tiff(a)
    assert dm.directory(blob)[0][tiffio.COMPRESSION] == (3, (5,)) and blob == lars.encode_tiff(a, compression="lzw")
    f = floats(40, 50, 1, seed=2)
    blob = lars.encode_tiff_f32(f, predictor=True)
    assert dm.directory(blob)[0][tiffio.COMPRESSION] == (3, (5,)) and blob == lars.encode_tiff_f32(f, predictor=True, compression="lzw")
    assert lars.tiff_bound(70, 90, 3, 1) == lars.tiff_bound(70, 90, 3, 1, compression="lzw")
