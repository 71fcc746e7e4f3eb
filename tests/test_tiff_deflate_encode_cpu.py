"""encode_tiff(..., compression="deflate") without a device: the model of a strip's stream (tests/tiff_deflate_encode_model.py)
against zlib, the bound against the model's file size, and the new arguments' checks, which run before anything is launched."""
import zlib

import numpy as np
import pytest

import lars_image_processing_amd as lars
import tiff_deflate_encode_model as dm
from lars_image_processing_amd import _ffi, driver

RNG = np.random.default_rng(20261019)


def smooth(n, seed):
    """Bytes with a skewed histogram: dynamic blocks."""
    return np.clip(np.random.default_rng(seed).normal(128, 6, n), 0, 255).astype(np.uint8).tobytes()


def inflate(stream):
    d = zlib.decompressobj()
    out = d.decompress(stream)
    assert d.eof and d.unused_data == b""
    return out


@pytest.mark.parametrize("n", [1, 2, 300, 32767, 32768, 32769, 65536, 65537, 100000])
@pytest.mark.parametrize("kind", ["random", "equal", "smooth"])
def test_model_stream_inflates_to_the_strip(n, kind):
    data = RNG.integers(0, 256, n, dtype=np.uint8).tobytes() if kind == "random" else bytes([0xFF]) * n if kind == "equal" else smooth(n, n)
    stream = dm.strip_stream(data)
    assert stream[:2] == b"\x78\x01" and inflate(stream) == data
    assert stream == dm.strip_stream(data)                  # a function of the strip's bytes alone
    p = -(-n // dm.SEG)
    assert len(stream) <= 2 + n + 5 * p + 4                 # what the bound allows a strip


def test_model_takes_both_forms_and_flushes_between_parts():
    random = RNG.integers(0, 256, 3 * dm.SEG, dtype=np.uint8).tobytes()
    stream = dm.strip_stream(random)                        # first, middle and last part stored
    assert len(stream) == 2 + 3 * (dm.SEG + 5) + 4 and stream[2] == 0 and stream[2 + 2 * (dm.SEG + 5)] == 1
    data = smooth(2 * dm.SEG + 5000, 3)
    first = dm.part(data[:dm.SEG], False)
    assert first[-4:] == b"\x00\x00\xff\xff" and first[0] & 7 == 4          # BFINAL 0, BTYPE 2
    assert dm.part(data[2 * dm.SEG:], True)[0] & 7 == 5                     # BFINAL 1, BTYPE 2
    assert inflate(dm.strip_stream(data)) == data
    mixed = smooth(dm.SEG, 4) + random[:dm.SEG] + smooth(100, 5)            # dynamic, stored, dynamic
    assert inflate(dm.strip_stream(mixed)) == mixed


@pytest.mark.parametrize("shape, dtype, rps, predictor", [
    ((1, 1), np.uint8, 1, False), ((1, 1), np.uint8, 1, True), ((5, 1), np.uint8, 1, False), ((37, 53, 3), np.uint8, 7, True),
    ((37, 53, 5), np.uint16, 37, False), ((3, 40000), np.uint8, 1, False), ((2, 9000), np.float32, 2, True), ((300, 1), np.uint16, 1, False),
])
@pytest.mark.parametrize("kind", ["random", "equal"])
def test_bound_covers_the_model_file(shape, dtype, rps, predictor, kind):
    if dtype == np.float32:
        a = RNG.integers(0, 1 << 32, shape, dtype=np.uint32).view(np.float32) if kind == "random" else np.full(shape, 0.25, np.float32)
    else:
        a = RNG.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype) if kind == "random" else np.full(shape, 77, dtype)
    strips, tags, dir_size = dm.stored_strips(a, rps, predictor)
    streams = [dm.strip_stream(s) for s in strips]
    for s, raw in zip(streams, strips):
        assert inflate(s) == raw
    size = dm.file_size(streams, dir_size)
    h, w = shape[:2]
    c = shape[2] if len(shape) == 3 else 1
    if dtype == np.float32:
        bound = lars.tiff_f32_bound(h, w, c, rps, compression="deflate")
    else:
        bound = lars.tiff_bound(h, w, c, a.dtype.itemsize, rps, compression="deflate")
    assert size <= bound, (size, bound)


def test_bound_is_zero_where_the_lzw_bound_is():
    lib = _ffi.load()
    for h, w, c, item, rps in [(0, 5, 1, 1, 0), (5, 0, 1, 1, 0), (4, 4, 6, 1, 0), (4, 4, 1, 4, 0), (4, 4, 1, 3, 0), ((1 << 24) + 1, 4, 1, 1, 0),
                               (4, 4, 1, 1, -1), (1 << 12, 1 << 20, 1, 1, 1 << 12)]:
        assert lars.tiff_bound(h, w, c, item, rps) == 0
        assert lib.lars_tiff_deflate_bound(h, w, c, item, rps) == 0 and lib.lars_tiff_deflate_encode_scratch_bytes(h, w, c, item, rps) == 0
    assert lib.lars_tiff_float32_deflate_bound(4, 4, 6, 0) == 0 and lib.lars_tiff_float32_deflate_encode_scratch_bytes(0, 4, 1, 0) == 0
    assert lars.tiff_bound(4, 4, 1, 1, compression="deflate") > 0 and lars.tiff_f32_bound(4, 4, 1, compression="deflate") > 0
    assert lib.lars_tiff_deflate_encode_scratch_bytes(4, 4, 1, 1, 0) > 0 and lib.lars_tiff_float32_deflate_encode_scratch_bytes(4, 4, 1, 0) > 0


def test_bound_follows_its_derivation():
    n = 3 * 40000
    per = n + 5 * 4 + 6                                     # four parts
    assert lars.tiff_bound(2, 40000, 3, 1, 1, compression="deflate") == 8 + 2 * per + 2 + 12 * 13 + 4 + 4 * 3 + 8 * 2
    assert lars.tiff_bound(1, 1, 1, 1, compression="deflate") == 8 + (1 + 5 + 6) + 2 + 12 * 13 + 4 + 4 + 8


def test_arguments_are_checked_before_anything_is_launched():
    a = np.zeros((4, 4), np.uint8)
    for bad in ("zip", "LZW", "", None, 8, True):
        with pytest.raises(ValueError, match="compression must be 'lzw' or 'deflate'"):
            lars.encode_tiff(a, compression=bad)
        with pytest.raises(ValueError, match="compression must be 'lzw' or 'deflate'"):
            lars.encode_tiff_f32(a.astype(np.float32), compression=bad)
        with pytest.raises(ValueError, match="compression must be 'lzw' or 'deflate'"):
            lars.tiff_bound(4, 4, 1, 1, compression=bad)
        with pytest.raises(ValueError, match="compression must be 'lzw' or 'deflate'"):
            lars.tiff_f32_bound(4, 4, 1, compression=bad)
    with pytest.raises(TypeError):
        lars.encode_tiff(a.astype(np.float32), compression="deflate")
    with pytest.raises(TypeError):
        lars.encode_tiff_f32(a, compression="deflate")
    with pytest.raises(ValueError, match="1 to 5 samples"):
        lars.encode_tiff(np.zeros((2, 2, 6), np.uint8), compression="deflate")
    img = np.zeros((4, 4, 3), np.uint8)
    for bad in ("deflate+", "Deflate", "predictor+deflate", 3):
        with pytest.raises(ValueError, match="want_tiff must be False, True or 'predictor'"):
            lars.process_image(img, indices=["NDVI"], want_tiff=bad)
    with pytest.raises(ValueError, match="want_tiff or want_png, not both"):
        lars.process_image(img, indices=["NDVI"], want_tiff="deflate", want_png=True)
    assert driver.TIFF_ENCODERS == ("pillow", "device", "device+deflate")
    with pytest.raises(ValueError, match="tiff_encoder must be 'pillow' or 'device'"):
        driver.process_image("x.png", "out", tiff_encoder="deflate")
    with pytest.raises(ValueError, match="tiff_encoder must be"):
        driver.batch_process("in", "out", tiff_encoder="device+lzw")


def test_process_image_sibling_refuses_other_compressions_without_a_device():
    import ctypes as C
    img = np.zeros((4, 4, 3), np.uint8)
    tiffs = [np.zeros(4096, np.uint8), None, None]
    lens = np.zeros(3, np.int64)
    p_none, p_tiff = _ffi.ptr3([None] * 3), _ffi.ptr3(tiffs)
    for compression in (0, 1, 7, 32946):
        with pytest.raises(_ffi.LarsError, match="compression must be 5 \\(LZW\\) or 8 \\(Deflate\\)") as e:
            _ffi.call("lars_h_process_image_tiff_float32", _ffi.ptr(img), 4, 4, 3, _ffi.dtype_code(img.dtype), 1, 1, 0, None, C.byref(p_none),
                      None, None, C.byref(p_none), C.byref(p_none), compression, 1, 0, C.byref(p_tiff), 4096, _ffi.ptr(lens))
        assert e.value.code == -1
