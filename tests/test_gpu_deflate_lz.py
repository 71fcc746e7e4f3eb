"""String matching in the device Deflate coder (tuning knob ``deflate_matching``, ``lars.deflate_matching()``) on the device.
Every stream -- a TIFF strip, a PNG file's joined IDAT payloads -- must be, byte for byte, what tests/deflate_lz_model.py writes
for the same bytes; the files around the streams must be what they are without matching; tiffio.read_tiff, lars.decode_tiff /
decode_png and Pillow must give the array back; no file is longer than without matching.  No tolerance anywhere."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import deflate_lz_cases as cases
import deflate_lz_model as lm
import lars_image_processing_amd as lars
import tiff_deflate_encode_model as dm
from lars_image_processing_amd import _ffi, tiffio
from test_png_cpu import check_png, parse_chunks

pytestmark = pytest.mark.gpu

SEG = lm.SEG
SKIPPED_TAGS = (tiffio.STRIP_OFFSETS, tiffio.STRIP_BYTE_COUNTS)


def encode_tiff(a, rps, predictor):
    if a.dtype == np.float32:
        return lars.encode_tiff_f32(a, rows_per_strip=rps, predictor=predictor, compression="deflate")
    return lars.encode_tiff(a, rows_per_strip=rps, predictor=predictor, compression="deflate")


def check_tiff(a, rps=None, predictor=False, streams=None):
    """The file under the knob: every strip the model's stream (``streams``: computed before), the directory tiffio's, the strips on
    even offsets with zero pad bytes, the directory right behind them; the readers give ``a`` back; not longer than without the knob.
    Returns (the file, the file without the knob)."""
    assert _ffi.get_tuning("deflate_matching") == 0
    with lars.deflate_matching():
        assert _ffi.get_tuning("deflate_matching") == 1
        blob = encode_tiff(a, rps, predictor)
        again = encode_tiff(a, rps, predictor)
    assert _ffi.get_tuning("deflate_matching") == 0
    plain = encode_tiff(a, rps, predictor)
    assert isinstance(blob, bytes) and blob == again and len(blob) <= len(plain)
    a3 = a.reshape(a.shape[0], a.shape[1], -1)
    h, w, c = a3.shape
    rows = min(rps, h) if rps else min(h, max(1, 65536 // (w * c * a.dtype.itemsize)))
    strips, want, _ = dm.stored_strips(a, rows, predictor)
    tags, ifd, _ = dm.directory(blob)
    assert list(tags) == list(want) == sorted(want)
    for tag in want:
        if tag not in SKIPPED_TAGS:
            assert tags[tag] == want[tag], tag
    offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
    assert len(offsets) == len(counts) == len(strips) == -(-h // rows)
    at = 8
    for k, (o, n) in enumerate(zip(offsets, counts)):
        assert o == at and o % 2 == 0, k
        at += n + (n & 1)
        stream = streams[k] if streams else lm.stream(strips[k])
        assert blob[o:o + n] == stream, (k, a.shape, rps, predictor)
        assert n % 2 == 0 or blob[o + n] == 0
    assert at == ifd
    assert blob[:8] == plain[:4] + ifd.to_bytes(4, "little")
    bound = lars.tiff_f32_bound(h, w, c, rps, compression="deflate") if a.dtype == np.float32 else lars.tiff_bound(h, w, c, a.dtype.itemsize, rps, compression="deflate")
    assert len(blob) <= bound
    shape = a.shape[:2] if c == 1 else a.shape
    for back in (tiffio.read_tiff(blob), lars.decode_tiff(blob, deflate=True)):
        assert back.dtype == a.dtype and back.shape == shape and back.tobytes() == a.tobytes()
    if c == 1 or (c == 3 and a.dtype == np.uint8):
        pil = np.asarray(Image.open(io.BytesIO(blob)))
        assert pil.dtype == a.dtype and pil.shape == shape and pil.tobytes() == a.tobytes()
    return blob, plain


# ---------------------------------------------------------------------------------------------------------------------
# exact byte control: one strip = the case's bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.byte_cases()))
def test_strip_is_the_models_stream(name):
    data = cases.byte_cases()[name]
    stream, rec = cases.streams()[name]
    a = np.frombuffer(data, np.uint8).reshape(1, -1)
    blob, plain = check_tiff(a, 1, False, streams=[stream])
    if "matched" not in rec["forms"]:
        assert blob == plain                                  # matching gains nothing: the file without the knob, byte for byte
    else:
        assert len(blob) < len(plain)
    if name.startswith("zeros") and len(data) >= SEG:
        assert 10 * len(blob) < len(plain)                    # a flat segment: at least 4096 bytes as literals, under 100 as matches


# ---------------------------------------------------------------------------------------------------------------------
# pictures
# ---------------------------------------------------------------------------------------------------------------------
def smooth_field(h, w, seed):
    """A smooth field in [-1, 1]: a few low-frequency waves."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = sum(a * np.sin(2 * np.pi * (u * xx / w + v * yy / h) + p)
            for a, u, v, p in zip(rng.uniform(0.3, 1, 5), rng.uniform(0.2, 3, 5), rng.uniform(0.2, 3, 5), rng.uniform(0, 6.28, 5)))
    return (f / np.abs(f).max()).astype(np.float32)


def check_png_file(arr, palette=None):
    assert _ffi.get_tuning("deflate_matching") == 0
    with lars.deflate_matching():
        blob = lars.encode_png(arr, palette)
        again = lars.encode_png(arr, palette)
    assert _ffi.get_tuning("deflate_matching") == 0
    plain = lars.encode_png(arr, palette)
    assert blob == again and len(blob) <= len(plain)
    check_png(blob, arr, palette=palette)                     # chunks, CRCs, zlib, the filters, Pillow
    idat = b"".join(d for t, d in parse_chunks(blob) if t == b"IDAT")
    assert idat == lm.stream(zlib.decompress(idat))
    others = lambda b: [(t, d) for t, d in parse_chunks(b) if t != b"IDAT"]     # noqa: E731
    assert others(blob) == others(plain)
    got = lars.decode_png(blob)
    assert got.shape == arr.shape and got.tobytes() == arr.tobytes()
    return blob, plain


def test_png_rgba_colormap_picture():
    blob, plain = check_png_file(lars.colorize_index(smooth_field(96, 96, 3), "NDVI"))
    assert len(blob) < len(plain)


def test_png_two_class_palette_picture():
    mask = (smooth_field(200, 300, 4) > 0.1).astype(np.uint8)
    palette = np.array([[0, 0, 0, 0], [30, 200, 60, 255]], np.uint8)
    blob, plain = check_png_file(mask, palette)
    assert len(blob) < len(plain)


def test_png_flat_picture():
    blob, plain = check_png_file(np.full((64, 1024), 90, np.uint8))          # 65600 filtered bytes: three segments
    assert 10 * len(blob) < len(plain)


def test_tiff_uint16_rgb_with_predictor():
    rng = np.random.default_rng(6)
    f = smooth_field(40, 512, 5)
    a = (np.stack([f, np.roll(f, 7, 1), f * f], axis=-1) * 20000 + 30000 + rng.integers(0, 3, (40, 512, 3))).astype(np.uint16)
    a[10:30, 100:400] = 65535                                 # a saturated area
    check_tiff(a, None, True)


@pytest.mark.parametrize("predictor", [False, True])
def test_tiff_float32_plane(predictor):
    f = smooth_field(64, 256, 7)
    f[20:40, 50:200] = np.float32("nan")                      # a masked area
    f[:8] = 0.25
    blob, plain = check_tiff(f, None, predictor)
    assert len(blob) < len(plain)


# ---------------------------------------------------------------------------------------------------------------------
# through the pipeline
# ---------------------------------------------------------------------------------------------------------------------
def test_process_image_files_follow_the_knob():
    rng = np.random.default_rng(8)
    img = np.clip(np.stack([smooth_field(64, 64, 10 + k) for k in range(3)], axis=-1) * 100 + 128 + rng.integers(0, 4, (64, 64, 3)), 0, 255).astype(np.uint8)
    img[:20, :30] = 255                                       # a saturated corner: flat index values
    host = lars.process_image(img, want_rgba=True)                           # the pictures and planes the files hold
    entries = lars.process_image(img, want_entries=True)
    for t in lars.api.INDEX_NAMES:
        host["indices"][t]["entry"] = entries["indices"][t]["entry"]
    calls = {"png": dict(want_png=True), "pal": dict(want_png="palette"), "tif": dict(want_tiff="deflate+predictor")}

    def standalone(kind, t):
        entry = host["indices"][t]
        if kind == "png":
            return lars.encode_png(entry["rgba"])
        if kind == "pal":
            return lars.encode_png(entry["entry"], lars.colormap_lut(lars.api._colormap_for(t)))
        return lars.encode_tiff_f32(entry["index"], predictor=True, compression="deflate")

    key = {"png": "png", "pal": "png", "tif": "tiff"}
    plain = {kind: lars.process_image(img, **kw) for kind, kw in calls.items()}
    with lars.deflate_matching():
        got = {kind: lars.process_image(img, **kw) for kind, kw in calls.items()}
        for kind in calls:
            for t in lars.api.INDEX_NAMES:
                assert got[kind]["indices"][t][key[kind]] == standalone(kind, t), (kind, t)
    assert _ffi.get_tuning("deflate_matching") == 0
    smaller = 0
    for kind, kw in calls.items():
        again = lars.process_image(img, **kw)
        for t in lars.api.INDEX_NAMES:
            mine, today = got[kind]["indices"][t][key[kind]], plain[kind]["indices"][t][key[kind]]
            assert len(mine) <= len(today)
            smaller += len(mine) < len(today)
            assert again["indices"][t][key[kind]] == today == standalone(kind, t), (kind, t)      # outside the block: today's files
    assert smaller > 0


def test_knob_is_restored_and_the_bytes_repeat():
    a = np.frombuffer(cases.byte_cases()["planted"], np.uint8).reshape(1, -1)
    before = _ffi.get_tuning("deflate_matching")
    with lars.deflate_matching():
        one = lars.encode_tiff(a, rows_per_strip=1, compression="deflate")
    assert _ffi.get_tuning("deflate_matching") == before == 0
    with pytest.raises(ZeroDivisionError):
        with lars.deflate_matching():
            lars.encode_tiff(a, rows_per_strip=1, compression="deflate")
            1 / 0
    assert _ffi.get_tuning("deflate_matching") == 0
    with lars.deflate_matching():
        two = lars.encode_tiff(a, rows_per_strip=1, compression="deflate")
    assert one == two and one != lars.encode_tiff(a, rows_per_strip=1, compression="deflate")


def test_driver_values_write_the_files_of_the_knob(tmp_path):
    from lars_image_processing_amd import driver
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(9)
    img = np.clip(np.stack([smooth_field(90, 120, 20 + k) for k in range(3)], axis=-1) * 100 + 128 + rng.integers(0, 4, (90, 120, 3)), 0, 255).astype(np.uint8)
    img[:30, :50] = 255
    Image.fromarray(img).save(src / "field.png")
    kw = dict(process_wb=True, indices=["NDVI", "NDWI"], index_tiff=True, lut_format="png8")
    driver.process_image(src / "field.png", tmp_path / "plain", png_encoder="device", tiff_encoder="device+deflate", **kw)
    driver.process_image(src / "field.png", tmp_path / "lz", png_encoder="device+matching", tiff_encoder="device+deflate+matching", **kw)
    assert _ffi.get_tuning("deflate_matching") == 0
    with lars.deflate_matching():
        driver.process_image(src / "field.png", tmp_path / "knob", png_encoder="device", tiff_encoder="device+deflate", **kw)
    assert driver.main([str(src), str(tmp_path / "cli"), "--wb", "--ndvi", "--lut-format", "png8", "--png-encoder", "device+matching", "--tiff-encoder",
                        "device+deflate+matching", "--index-tiff", "--quiet", "--workers", "2"]) == 0
    assert _ffi.get_tuning("deflate_matching") == 0
    rels = ("white_balanced/field_wb.tif", "NDVI/field_ndvi.png", "NDWI/field_ndwi.png", "NDVI/field_ndvi_f32.tif", "NDWI/field_ndwi_f32.tif")
    smaller = 0
    for rel in rels:
        plain, lz = (tmp_path / "plain" / rel).read_bytes(), (tmp_path / "lz" / rel).read_bytes()
        assert lz == (tmp_path / "knob" / rel).read_bytes() == (tmp_path / "cli" / rel).read_bytes(), rel
        assert len(lz) <= len(plain), rel
        smaller += len(lz) < len(plain)
        if rel.endswith(".tif"):
            assert tiffio.read_tiff(lz).tobytes() == tiffio.read_tiff(plain).tobytes()
        else:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(lz)).convert("RGBA")), np.asarray(Image.open(io.BytesIO(plain)).convert("RGBA")))
    assert smaller >= 3
    blob = driver.export_zip(img, ["NDVI"], png_encoder="device+matching")
    import zipfile
    with zipfile.ZipFile(io.BytesIO(blob)) as zf, lars.deflate_matching():
        assert zf.read("white_balanced.png") == lars.encode_png(lars.fix_white_balance(img))
    assert _ffi.get_tuning("deflate_matching") == 0
