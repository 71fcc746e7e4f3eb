"""decode_jpeg(data, scale) and thumbnail_jpeg(..., scaled=True) on the GPU: every array equals what Pillow returns after
``draft`` has switched libjpeg to 1/2, 1/4 or 1/8 scale, byte for byte; hand-built files equal the NumPy model too."""
import ctypes as C
import io
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_scaled_cases as K  # noqa: E402
import jpeg_scaled_model as S  # noqa: E402
import test_jpeg_handmade_cpu as H  # noqa: E402

pytestmark = pytest.mark.gpu


def same(b, scale, name=None, model=False):
    """decode_jpeg(b, scale) is Pillow's array after draft (and the model's, where asked)."""
    got, ref = lars.decode_jpeg(b, scale), S.pillow_scaled(b, scale)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, scale, got.shape, ref.shape)
    assert got.tobytes() == ref.tobytes(), f"{name} at 1/{scale}: {int((got != ref).sum())} of {ref.size} samples differ from Pillow"
    if model:
        assert got.tobytes() == S.decode(b, scale).tobytes(), f"{name} at 1/{scale}: differs from the model"


@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("mode", list(K.MODES))
def test_shapes_equal_pillow(mode, scale):
    for w, h in K.SHAPES:
        same(K.written(w, h, mode, 75), scale, (w, h, mode))
    same(K.written(67, 93, mode, 98), scale, (67, 93, mode, 98))
    same(K.written(67, 93, mode, 20), scale, (67, 93, mode, 20))


@pytest.mark.parametrize("mode", ["420", "422"])
def test_every_width_and_height_at_half_scale(mode):
    """Edge blocks, odd chroma widths and the chroma plane of at most two samples (widths 1-8 of 4:2:2)."""
    for n in range(1, 34):
        same(K.written(n, 9, mode), 2, (n, 9, mode))
        same(K.written(9, n, mode), 2, (9, n, mode))


@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("restart", [1, 7, 5000])
def test_restart_intervals(restart, scale):
    """The DC is summed from the start of its interval at every block size."""
    for mode in K.MODES:
        same(K.written(67, 93, mode, 75, restart), scale, (mode, restart))
        same(K.written(33, 5, mode, 75, restart), scale, (mode, restart))


def test_scale_1_through_the_new_exports_is_decode_jpeg():
    for mode in K.MODES:
        b = K.written(67, 93, mode)
        ref = lars.decode_jpeg(b)
        assert lars.decode_jpeg(b, 1).tobytes() == ref.tobytes() == S.pillow_scaled(b, 1).tobytes()
        file = np.frombuffer(b, np.uint8)
        out = np.zeros(ref.shape, np.uint8)
        _ffi.call("lars_h_decode_jpeg_scaled_u8", _ffi.ptr(file), file.size, 1, _ffi.ptr(out), out.nbytes)
        assert out.tobytes() == ref.tobytes()
        device_entry_point_with_guards(b, 1, ref)


def device_entry_point_with_guards(b, scale, ref):
    """lars_d_decode_jpeg_scaled_u8 on a caller's stream into the middle of a buffer: the status is clean, the output is
    ``ref`` and the 4096 bytes on either side of it are untouched."""
    lib = _ffi.load()
    info = _ffi.JpegInfo.array()
    file = np.frombuffer(b, np.uint8)
    assert lib.lars_jpeg_info(_ffi.ptr(file), file.size, info) == 0
    need = lib.lars_jpeg_decode_scaled_scratch_bytes(info, scale)
    assert need > 0
    guard, nbytes = 4096, ref.size
    d_file, d_out, d_scratch, d_status, stream = (C.c_void_p() for _ in range(5))
    _ffi.call("lars_malloc", C.byref(d_file), file.size)
    _ffi.call("lars_malloc", C.byref(d_out), nbytes + 2 * guard)
    _ffi.call("lars_malloc", C.byref(d_scratch), need)
    _ffi.call("lars_malloc", C.byref(d_status), 8)
    _ffi.call("lars_stream_create", C.byref(stream))
    try:
        _ffi.call("lars_memcpy_h2d", d_file, _ffi.ptr(file), file.size)
        _ffi.call("lars_memset", d_out, 0xA5, nbytes + 2 * guard, stream)
        head = np.ascontiguousarray(file[:_ffi.JpegInfo(*info).entropy_offset])
        _ffi.call("lars_d_decode_jpeg_scaled_u8", d_file, _ffi.ptr(head), info, scale, C.c_void_p(d_out.value + guard), d_status, d_scratch, stream)
        _ffi.call("lars_synchronize", stream)
        got = np.empty(nbytes + 2 * guard, np.uint8)
        status = np.empty(2, np.int32)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(got), d_out, got.size)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(status), d_status, 8)
    finally:
        _ffi.call("lars_stream_destroy", stream)
        for p in (d_file, d_out, d_scratch, d_status):
            _ffi.call("lars_free", p)
    assert status.tolist() == [0, 0]
    assert (got[:guard] == 0xA5).all() and (got[-guard:] == 0xA5).all()
    assert got[guard:-guard].tobytes() == ref.tobytes()


@pytest.mark.parametrize("scale", K.SCALES)
def test_device_entry_point_on_a_callers_stream_with_guards(scale):
    for mode, shape in (("420", (201, 333)), ("422", (67, 93)), ("L", (33, 5))):
        b = K.written(shape[0], shape[1], mode, 75, 7)
        device_entry_point_with_guards(b, scale, S.pillow_scaled(b, scale))


def test_the_library_refuses_other_scales():
    file = np.frombuffer(K.written(33, 5, "420"), np.uint8)
    out = np.zeros(33 * 5 * 3, np.uint8)
    for bad in (0, 3, 16, -1):
        with pytest.raises(_ffi.LarsError) as e:
            _ffi.call("lars_h_decode_jpeg_scaled_u8", _ffi.ptr(file), file.size, bad, _ffi.ptr(out), out.nbytes)
        assert e.value.code == -1 and "scale" in str(e.value)


def test_damaged_entropy_data_raises_value_error_at_every_scale():
    good = K.written(67, 93, "420", 98)
    cut = good[:len(good) * 2 // 3]
    with pytest.raises(ValueError):
        S.decode(cut, 2)                                    # damaged by the sequential model's judgement too
    for s in K.SCALES:
        with pytest.raises(ValueError, match="entropy data"):
            lars.decode_jpeg(cut, s)
        same(good, s)                                       # and the next good file decodes correctly afterwards


@pytest.mark.parametrize("scale", K.SCALES)
def test_fuzz_files(scale):
    for k in range(0, K.FUZZ_N, 3):
        name, b = K.fuzz_file(k)
        same(b, scale, name)


# ---------------------------------------------------------------------------------------------------------------------
# hand-built files
# ---------------------------------------------------------------------------------------------------------------------
HAND = [n for n in sorted(H.HANDMADE) if n.split()[0] in ("dqt16", "tables", "outside") or "fill before RSTn" in n or "fill 2" in n]


@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("group", ["dqt16", "tables", "outside", "restart", "header"])
def test_handmade_files_equal_pillow_and_the_model(group, scale):
    """16-bit DQT, own tables per component, blocks outside the ordinary range, fill bytes before RSTn."""
    names = [n for n in HAND if n.split()[0] == group]
    assert names
    for n in names:
        same(H.HANDMADE[n](), scale, n, model=True)


@pytest.mark.parametrize("scale", K.SCALES)
@pytest.mark.parametrize("mode", list(K.MODES))
def test_extreme_blocks_equal_pillow_and_the_model(mode, scale):
    """Products beyond 16 bits, the 4 x 4 short cut, the 2 x 2 pass's mixed narrowing, the 1 x 1 range-limit wrap."""
    for kind in K.EXTREME_KINDS:
        same(K.extreme(kind, mode), scale, (kind, mode), model=True)


@pytest.mark.parametrize("name", ["frame L 1 x 65500", "frame 420 1 x 65500", "frame 444 65500 x 1"])
def test_the_longest_frames_at_one_eighth(name):
    same(H.HANDMADE[name](), 8, name)


# ---------------------------------------------------------------------------------------------------------------------
# thumbnails
# ---------------------------------------------------------------------------------------------------------------------
def gallery_file(w, h, mode):
    return K.written(w, h, mode, 85)


def thumb_same(b, size, gap, scale):
    im = Image.open(io.BytesIO(b))
    im.thumbnail(size, Image.Resampling.LANCZOS, gap)
    assert (im.decoderconfig[0] if im.decoderconfig else 1) == scale, im.decoderconfig   # Pillow decoded at that scale too
    got = lars.thumbnail_jpeg(b, size, gap, scaled=True)
    ref = np.asarray(im)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), (size, gap, scale, int((got != ref).sum()))


@pytest.mark.parametrize("mode", ["L", "420", "422"])
@pytest.mark.parametrize("shape,scale", [((200, 170), 2), ((700, 500), 4), ((1400, 1300), 8), ((333, 201), 2), ((401, 333), 4), ((1401, 1303), 8),
                                         ((163, 2017), 2)])
def test_thumbnail_jpeg_scaled_matches_pillow(shape, scale, mode):
    """(40, 40) at gap 2.0: whole and fractional draft boxes at each scale, one tall picture."""
    assert api.jpeg_draft_scale(shape, (40, 40), 2.0) == scale
    thumb_same(gallery_file(shape[0], shape[1], mode), (40, 40), 2.0, scale)


@pytest.mark.parametrize("gap,scale", [(None, 1), (1.0, 8), (3.0, 2)])
def test_thumbnail_jpeg_scaled_at_other_gaps(gap, scale):
    for mode in ("L", "420"):
        b = gallery_file(333, 401, mode)
        assert api.jpeg_draft_scale((333, 401), (40, 40), gap) == scale
        thumb_same(b, (40, 40), gap, scale)


def test_thumbnail_jpeg_drafted_to_the_final_size():
    b = gallery_file(800, 800, "420")
    im = Image.open(io.BytesIO(b))
    im.thumbnail((100, 100), Image.Resampling.LANCZOS, 1.0)
    assert im.decoderconfig == (8, 0) and im.size == (100, 100)
    got = lars.thumbnail_jpeg(b, (100, 100), 1.0, scaled=True)
    assert got.tobytes() == np.asarray(im).tobytes() == lars.decode_jpeg(b, 8).tobytes()


def test_the_default_still_refuses():
    b = K.jpeg(np.full((2048, 2048), 90, np.uint8))
    with pytest.raises(NotImplementedError, match="scale"):
        lars.thumbnail_jpeg(b)
    with pytest.raises(NotImplementedError, match="1/2 scale"):
        lars.thumbnail_jpeg(b, scaled=False)
    thumb_same(b, (400, 400), 2.0, 2)
