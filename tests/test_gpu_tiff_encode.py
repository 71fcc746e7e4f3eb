"""encode_tiff on the device.  Every strip of every file must be, byte for byte, lzw_writer.pack(lzw_writer.encode(raw strip,
clear_at=4094)) -- the greedy encoder's stream, which is libtiff's --, the directory must hold tiffio.write_tiff's tags and
values (but Compression, StripOffsets, StripByteCounts), and tiffio.read_tiff, lars.decode_tiff and, where it reads the
layout as stored, Pillow must give the array back.  No tolerance anywhere: greedy LZW has one right answer."""
import ctypes as C
import io
import threading

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
import lzw_writer as lz
from lars_image_processing_amd import _ffi, driver, tiffio
from test_gpu_tiff_decode import one_over_f, sample
from test_tiff_encode_cpu import directory, written

pytestmark = pytest.mark.gpu

SKIPPED_TAGS = (tiffio.COMPRESSION, tiffio.STRIP_OFFSETS, tiffio.STRIP_BYTE_COUNTS)


def raw_strip(a3, y0, rows, predictor):
    part = a3[y0:y0 + rows]
    if predictor:
        part = np.concatenate([part[:, :1], np.diff(part, axis=1)], axis=1)       # unsigned wrap-around = modulo 2^bits
    return np.ascontiguousarray(part).astype(a3.dtype.newbyteorder("<")).tobytes()


def check(a, rps=None, predictor=False, strip_bytes=65536):
    """Everything the issue asks of one file; returns (the file, the streams' codes per strip)."""
    blob = lars.encode_tiff(a, rows_per_strip=rps, predictor=predictor)
    assert isinstance(blob, bytes)
    a3 = a.reshape(a.shape[0], a.shape[1], -1)
    h, w, c = a3.shape
    rows = min(rps, h) if rps else min(h, max(1, strip_bytes // (w * c * a.dtype.itemsize)))
    tags, ifd = directory(blob)
    want, _ = directory(written(a, rows, predictor))
    assert list(tags) == list(want)
    for tag in want:
        if tag not in SKIPPED_TAGS:
            assert tags[tag] == want[tag], tag
    assert tags[tiffio.COMPRESSION] == (3, (5,)) and tags[tiffio.ROWS_PER_STRIP] == (4, (rows,))
    offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
    assert len(offsets) == len(counts) == -(-h // rows)
    at, all_codes = 8, []
    for k, (o, n) in enumerate(zip(offsets, counts)):
        assert o == at and o % 2 == 0, k
        at += n + (n & 1)
        codes = lz.encode(raw_strip(a3, k * rows, rows, predictor), clear_at=4094)
        assert blob[o:o + n] == lz.pack(codes), (k, a.shape, rps, predictor)
        assert n % 2 == 0 or blob[o + n] == 0
        all_codes.append(codes)
    assert at == ifd and len(blob) <= lars.tiff_bound(h, w, c, a.dtype.itemsize, rps)
    shape = a.shape[:2] if c == 1 else a.shape           # the readers give [H, W] for one sample, also for a [H, W, 1] array
    for back in (tiffio.read_tiff(blob), lars.decode_tiff(blob)):
        assert back.dtype == a.dtype and back.shape == shape and back.tobytes() == a.tobytes()
    if c == 1 or (c == 3 and a.dtype == np.uint8):       # Pillow: not four samples with unspecified extras, not 16-bit RGB
        pil = np.asarray(Image.open(io.BytesIO(blob)))
        assert pil.dtype == a.dtype and pil.shape == shape and pil.tobytes() == a.tobytes()
    return blob, all_codes


@pytest.mark.parametrize("predictor", [False, True])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_small_pictures_every_sample_count(dtype, predictor):
    for c in range(1, 6):
        a = sample(dtype, 37, 53, c, seed=10 * c + predictor)
        for rps in (1, 7, None):                          # 7: the last strip holds 2 rows; None: one strip of 37
            check(a, rps, predictor)
        if c == 1:
            check(a[..., None], 7, predictor)             # [H, W, 1] is the same file


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1)])
def test_degenerate_shapes(shape):
    rng = np.random.default_rng(5)
    for dtype in (np.uint8, np.uint16):
        a = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
        for predictor in (False, True):
            check(a, None, predictor)
            check(np.dstack([a, a, a]), 2, predictor)


def test_one_strip_of_random_bytes_all_widths_and_clears():
    a = np.random.default_rng(20261018).integers(0, 256, (1, 20000), dtype=np.uint8)
    blob, (codes,) = check(a)
    assert codes.count(lz.CLEAR) == 6                     # the leading one and five of a full table
    i, widths = 0, set()
    for code in codes:
        widths.add(lz.width_of(i))
        i = 0 if code == lz.CLEAR else i + 1
    assert widths == {9, 10, 11, 12}


def test_zeros_and_a_constant_picture():
    _, (codes,) = check(np.zeros((1, 20000), np.uint8))
    assert len(codes) < 250
    check(np.full((384, 512), 77, np.uint8))              # strips of 128 rows
    check(np.full((384, 512), 77, np.uint8), None, True)


def test_uint16_rgb_with_predictor():
    check(sample(np.uint16, 263, 257, 3, seed=3), None, True)      # strips of 42 rows, the last of 11


def test_three_hundred_strips_of_one_row():
    check(one_over_f(np.random.default_rng(8), 300, 64, 1)[..., 0], 1, True)


@pytest.mark.parametrize("predictor", [False, True])
def test_one_over_f_picture(predictor):
    check(one_over_f(np.random.default_rng(9), 240, 320, 3), None, predictor)


def test_default_strips_follow_the_knob():
    a = one_over_f(np.random.default_rng(10), 64, 100, 3)
    with _ffi.tuning(tiff_strip_bytes=8192):
        check(a, None, False, strip_bytes=8192)           # 27 rows
    with _ffi.tuning(tiff_strip_bytes=100):
        check(a, None, False, strip_bytes=100)            # less than a row: one row per strip
    check(a)


def call_host(a3, cap, rps=0, predictor=0):
    out = np.zeros(max(cap, 1), np.uint8)
    n = C.c_int64(-7)
    _ffi.call("lars_h_encode_tiff", _ffi.ptr(a3), a3.shape[0], a3.shape[1], a3.shape[2], a3.dtype.itemsize, rps, predictor, _ffi.ptr(out), cap,
              C.byref(n))
    return out[:n.value].tobytes()


def test_a_buffer_one_byte_short_is_refused_and_the_next_call_works():
    a = np.ascontiguousarray(one_over_f(np.random.default_rng(11), 50, 70, 3))
    blob = lars.encode_tiff(a, rows_per_strip=8)
    with pytest.raises(_ffi.LarsError) as e:
        call_host(a, len(blob) - 1, 8)
    assert e.value.code == -1 and f"the file needs {len(blob)} bytes, out_cap is {len(blob) - 1} (device status 1)" in str(e.value)
    assert call_host(a, len(blob), 8) == blob
    assert lars.encode_tiff(a, rows_per_strip=8) == blob


def test_device_entry_point_resets_its_status():
    """lars_d_encode_tiff twice into the same status words: out_cap one byte short (LARS_TIFE_NOSPACE, the needed length), then enough."""
    a = one_over_f(np.random.default_rng(12), 40, 60, 3)
    blob = lars.encode_tiff(a, rows_per_strip=16)
    d_img, d_out = _ffi.DeviceBuffer(a.nbytes), _ffi.DeviceBuffer(len(blob))
    d_scr = _ffi.DeviceBuffer(_ffi.load().lars_tiff_encode_scratch_bytes(40, 60, 3, 1, 16))
    d_ans = _ffi.DeviceBuffer(16)                         # int64 length, int32 status[2]
    try:
        d_img.upload(a)
        for cap, want_status in ((len(blob) - 1, 1), (len(blob), 0), (0, 1)):
            _ffi.call("lars_d_encode_tiff", C.c_void_p(d_img.ptr), 40, 60, 3, 1, 16, 0, C.c_void_p(d_out.ptr), cap, C.c_void_p(d_ans.ptr),
                      C.c_void_p(d_ans.ptr + 8), C.c_void_p(d_scr.ptr), None)
            _ffi.call("lars_synchronize", None)
            assert int(d_ans.download(np.int64, (1,))[0]) == len(blob)
            assert d_ans.download(np.int32, (2,), offset=8).tolist() == [want_status, 0]
            if want_status == 0:
                assert d_out.download(np.uint8, (len(blob),)).tobytes() == blob
    finally:
        for b in (d_img, d_out, d_scr, d_ans):
            b.free()


def test_eight_threads_encode_at_once():
    rng = np.random.default_rng(13)
    pics = [one_over_f(rng, 90 + 11 * k, 200 - 9 * k, 3) if k % 2 else sample(np.uint16, 60 + 5 * k, 71 + k, 1 + k % 4, seed=k) for k in range(8)]
    want = [lars.encode_tiff(p, rows_per_strip=5 + k, predictor=k % 3 == 0) for k, p in enumerate(pics)]
    got, errors = [None] * 8, []

    def work(k):
        try:
            for _ in range(4):
                got[k] = lars.encode_tiff(pics[k], rows_per_strip=5 + k, predictor=k % 3 == 0)
                assert got[k] == want[k]
        except Exception as exc:                          # noqa: BLE001
            errors.append((k, exc))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == want
    for k in (1, 2):
        assert tiffio.read_tiff(want[k]).tobytes() == pics[k].tobytes()


def test_driver_writes_the_same_pictures(tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(one_over_f(np.random.default_rng(14), 90, 120, 3)).save(src / "field.png")
    for enc in ("pillow", "device"):
        driver.process_image(src / "field.png", tmp_path / enc, process_wb=True, indices=["NDVI", "NDWI"], lut_format="tiff", tiff_encoder=enc)
    for rel in ("white_balanced/field_wb.tif", "NDVI/field_ndvi.tif", "NDWI/field_ndwi.tif"):
        a, b = tiffio.read_tiff(str(tmp_path / "pillow" / rel)), tiffio.read_tiff(str(tmp_path / "device" / rel))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), rel
        tags, _ = directory((tmp_path / "device" / rel).read_bytes())
        assert tags[tiffio.COMPRESSION] == (3, (5,))
    wb = np.asarray(Image.open(tmp_path / "device" / "white_balanced/field_wb.tif"))
    assert np.array_equal(wb, np.asarray(Image.open(tmp_path / "pillow" / "white_balanced/field_wb.tif")))
    # the command line and batch_process hand the choice on
    assert driver.main([str(src), str(tmp_path / "cli"), "--wb", "--ndvi", "--lut-format", "tiff", "--tiff-encoder", "device", "--quiet", "--workers", "1"]) == 0
    for rel in ("white_balanced/field_wb.tif", "NDVI/field_ndvi.tif", "NDWI/field_ndwi.tif"):
        assert (tmp_path / "cli" / rel).read_bytes() == (tmp_path / "device" / rel).read_bytes()
    with pytest.raises(ValueError, match="tiff_encoder must be 'pillow' or 'device'"):
        driver.process_image(src / "field.png", tmp_path / "x", tiff_encoder="gpu")
