"""CPU side of JPEG decoding at 1/2, 1/4 and 1/8 scale: the NumPy model (jpeg_scaled_model.py) against the installed Pillow
after ``draft`` -- on Pillow-written files, a seeded fuzz, every hand-built file of test_jpeg_handmade_cpu.py and the
extreme blocks of jpeg_scaled_cases.py -- and what ``decode_jpeg(scale=...)`` / ``thumbnail_jpeg(scaled=...)`` decide before
the library is called."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_model  # noqa: E402
import jpeg_scaled_cases as K  # noqa: E402
import jpeg_scaled_model as S  # noqa: E402
import test_jpeg_handmade_cpu as H  # noqa: E402


def check(b, name, scales=K.SCALES):
    """model == Pillow at every scale; the entropy decoder of the model runs once."""
    parsed = S.coefficients(b)
    for s in scales:
        ref, got = S.pillow_scaled(b, s), S.decode(parsed, s)
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, s, got.shape, ref.shape)
        assert got.tobytes() == ref.tobytes(), f"{name} at 1/{s}: {int((got != ref).sum())} of {ref.size} samples differ"


def _no_device(*_a, **_k):
    raise AssertionError("the library was called")


# ---------------------------------------------------------------------------------------------------------------------
# the model against Pillow
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES + K.MORE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_equals_pillow_on_written_files(shape):
    for q in K.QUALITIES:
        for mode in K.MODES:
            check(K.written(shape[0], shape[1], mode, q), (shape, mode, q))


@pytest.mark.parametrize("restart", [1, 7, 5000])
def test_model_equals_pillow_with_restart_intervals(restart):
    """Intervals of one MCU, of seven, and longer than the frame (no marker at all)."""
    for w, h in ((67, 93), (33, 5), (9, 17)):
        for mode in K.MODES:
            b = K.written(w, h, mode, 75, restart)
            assert jpeg_model.parse(b)[3] == restart
            assert (b"\xff\xd0" in b) == (restart < S.coefficients(b)[4].shape[0]), (w, h, mode)
            check(b, (w, h, mode, restart))


def test_scale_1_of_the_model_is_the_full_scale_model():
    b = K.written(67, 93, "420")
    assert S.decode(b, 1).tobytes() == jpeg_model.decode(b).tobytes() == S.pillow_scaled(b, 1).tobytes()
    with pytest.raises(ValueError):
        S.decode(b, 3)


def test_draft_is_asked_where_it_grants_the_scale():
    """pillow_scaled goes through ``draft`` itself wherever both sides are at least ``scale``; smaller pictures get the
    settings ``draft`` would write.  Both ways give the decoder the same configuration."""
    b = K.written(67, 93, "422")
    for s in K.SCALES:
        im = Image.open(io.BytesIO(b))
        assert im.draft(None, (67 // s, 93 // s)) == ("RGB", (0, 0, 67 / s, 93 / s)) and im.decoderconfig == (s, 0)
        assert np.asarray(im).tobytes() == S.pillow_scaled(b, s).tobytes()
    assert S.pillow_scaled(K.written(2, 200, "420"), 8).shape == (25, 1, 3)
    assert S.pillow_scaled(K.written(1, 1, "L"), 4).shape == (1, 1)


@pytest.mark.parametrize("part", range(6))
def test_model_equals_pillow_on_the_fuzz(part):
    """Seed and count: jpeg_scaled_cases.FUZZ_SEED, FUZZ_N (tests/golden/FUZZ_JPEG_SCALED.md)."""
    assert K.FUZZ_N % 6 == 0
    for k in range(part * K.FUZZ_N // 6, (part + 1) * K.FUZZ_N // 6):
        name, b = K.fuzz_file(k)
        check(b, name)


@pytest.mark.parametrize("name", sorted(H.HANDMADE))
def test_model_equals_pillow_on_handmade_files(name):
    """Every hand-built file of the full-scale suite, the "outside" and "huge" ones included, at every scale."""
    check(H.HANDMADE[name](), name)


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("kind", K.EXTREME_KINDS)
def test_model_equals_pillow_on_extreme_blocks(kind, mode):
    check(K.extreme(kind, mode), (kind, mode))


def test_extreme_files_leave_the_ordinary_range():
    """The group is what it says: dequantised coefficients beyond 11 bits signed in every kind but "huge q1" (dense blocks of
    +-1023: the outputs leave 0-255 by far, the coefficients stay within 11 bits), and beyond 16 bits (the product wraps) where the kind says so."""
    for kind in K.EXTREME_KINDS:
        _h, _w, comps, q, coefs, _mw, _mh = S.coefficients(K.extreme(kind, "L"))
        peak = int(np.abs(coefs[:, 0].reshape(-1, 8, 8) * np.array(q[comps[0][3]], np.int64).reshape(8, 8)).max())
        assert (peak <= 1023) == (kind == "huge q1"), (kind, peak)
        if kind in ("huge q255", "small q16bit", "DC q255", "DC q16bit", "DC q65535", "row 0 only", "rows 0 and 4"):
            assert peak > 32767, (kind, peak)


def test_fancy_upsampling_is_off_at_one_eighth():
    """4:2:2 at 1/8 is replication: the triangle filter would give other chroma on this file, and Pillow sides with the model."""
    b = K.written(67, 93, "422", 98)
    h, w, _comps, P, sizes = S.planes(b, 8)
    assert sizes == [1, 1, 1] and (h, w) == (12, 9)
    assert (jpeg_model.upsample(P[1], w, h, 2, 1) != np.repeat(P[1], 2, axis=1)[:h, :w]).any()
    assert S.decode(b, 8).tobytes() == S.pillow_scaled(b, 8).tobytes()


def test_block_sizes_follow_libjpegs_rule():
    comps = {"L": [(1, 1, 1, 0)], "444": [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)], "422": [(1, 2, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)],
             "420": [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]}
    for s, m in ((2, 4), (4, 2), (8, 1)):
        assert S.block_sizes(comps["L"], s) == [m]
        assert S.block_sizes(comps["444"], s) == [m, m, m]
        assert S.block_sizes(comps["422"], s) == [m, m, m]
        assert S.block_sizes(comps["420"], s) == [m, 2 * m, 2 * m]
    assert S.block_sizes(comps["420"], 1) == [8, 8, 8]


# ---------------------------------------------------------------------------------------------------------------------
# what the Python layer decides before the library is called
# ---------------------------------------------------------------------------------------------------------------------
def test_decode_jpeg_scale_argument(monkeypatch):
    monkeypatch.setattr(_ffi, "call", _no_device)
    b = K.written(33, 5, "420")
    for bad in (0, 3, 16, -2, "2", 2.0, True, None):
        with pytest.raises(ValueError, match="scale 1, 2, 4 or 8"):
            lars.decode_jpeg(b, bad)
        with pytest.raises(ValueError, match="scale 1, 2, 4 or 8"):
            lars.decode_jpeg(b, scale=bad)
    with pytest.raises(TypeError):
        lars.decode_jpeg(12, 2)


def test_decode_jpeg_hands_the_scale_and_the_scaled_shape_to_the_library(monkeypatch):
    got = []
    monkeypatch.setattr(_ffi, "call", lambda name, *a: got.append((name, a)) or 0)
    b = K.written(201, 333, "422")
    assert lars.decode_jpeg(b, np.int64(4)).shape == (84, 51, 3)
    assert lars.decode_jpeg(b, 8).shape == (42, 26, 3)
    assert lars.decode_jpeg(K.written(130, 3, "L"), 2).shape == (2, 65)
    assert lars.decode_jpeg(b, 1).shape == lars.decode_jpeg(b).shape == (333, 201, 3)
    assert [g[0] for g in got] == ["lars_h_decode_jpeg_scaled_u8"] * 3 + ["lars_h_decode_jpeg_u8"] * 2
    assert [g[1][2] for g in got[:3]] == [4, 8, 2] and got[0][1][4] == 84 * 51 * 3


GALLERY = [((200, 170), 2), ((700, 500), 4), ((1400, 1300), 8), ((333, 201), 2), ((401, 333), 4), ((170, 90), 1)]   # (w, h) at (40, 40), gap 2.0


@pytest.mark.parametrize("shape,scale", GALLERY)
def test_jpeg_draft_scale_is_the_scale_pillow_decodes_at(shape, scale):
    b = K.jpeg(np.full((shape[1], shape[0]), 70, np.uint8))
    im = Image.open(io.BytesIO(b))
    im.thumbnail((40, 40), Image.Resampling.LANCZOS, 2.0)
    assert im.decoderconfig == (scale, 0)
    assert api.jpeg_draft_scale(shape, (40, 40), 2.0) == scale


def test_thumbnail_jpeg_scaled_argument(monkeypatch):
    got = {}

    def capture(name, *args):
        got["name"], got["args"] = name, args
        return 0

    monkeypatch.setattr(_ffi, "call", capture)
    w, h = 333, 201
    b = K.jpeg(np.full((h, w, 3), 70, np.uint8))
    for bad in ("yes", 1, None, 2.0):
        with pytest.raises(TypeError, match="scaled"):
            lars.thumbnail_jpeg(b, (40, 40), 2.0, scaled=bad)
    assert not got
    with pytest.raises(NotImplementedError, match="1/2 scale"):      # the default has not moved
        lars.thumbnail_jpeg(b, (40, 40), 2.0)
    with pytest.raises(NotImplementedError, match="scale"):
        lars.thumbnail_jpeg(b, (40, 40), 2.0, scaled=False)
    assert not got
    out = lars.thumbnail_jpeg(b, (40, 40), 2.0, scaled=True)
    # the plan is the one thumbnail() computes for the image Pillow drafted, fractional box included
    im = Image.open(io.BytesIO(b))
    mode_box = im.draft(None, (80, 80))
    assert mode_box == ("RGB", (0, 0, w / 2, h / 2)) and im.size == (167, 101)
    plan = api.thumbnail_plan((w, h), (40, 40), 2.0, mode_box[1], im.size)
    assert got["name"] == "lars_h_thumbnail_jpeg_scaled_u8" and out.shape == (plan.size[1], plan.size[0], 3) == (24, 40, 3)
    _file, n, scale, fx, fy, rbox, box, new_h, new_w, vfirst, _out = got["args"]
    assert (n, scale, (fx, fy), (new_h, new_w), vfirst) == (len(b), 2, plan.factor, (24, 40), int(plan.vertical_first))
    assert tuple(rbox) == plan.reduce_box and tuple(box) == plan.box
    # scale 1: both settings end in the full-scale entry point
    got.clear()
    lars.thumbnail_jpeg(b, (100, 100), 2.0, scaled=True)
    assert got["name"] == "lars_h_thumbnail_jpeg_u8"


def test_thumbnail_jpeg_drafted_to_the_final_size_is_the_scaled_decode(monkeypatch):
    """As test_jpeg_drafted_to_final_size_is_returned_as_is for ``thumbnail``: 800 x 800 at (100, 100), gap 1.0 is drafted to
    100 x 100, nothing is left to resize."""
    got = []
    monkeypatch.setattr(_ffi, "call", lambda name, *a: got.append((name, a)) or 0)
    b = K.jpeg(np.full((800, 800, 3), 90, np.uint8))
    ref = Image.open(io.BytesIO(b))
    ref.thumbnail((100, 100), Image.Resampling.LANCZOS, 1.0)
    assert ref.decoderconfig == (8, 0) and ref.size == (100, 100)
    out = lars.thumbnail_jpeg(b, (100, 100), 1.0, scaled=True)
    assert out.shape == (100, 100, 3) and [g[0] for g in got] == ["lars_h_decode_jpeg_scaled_u8"] and got[0][1][2] == 8


# ---------------------------------------------------------------------------------------------------------------------
# host parts of the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_scratch_size_of_the_scaled_decoder():
    lib = _ffi.load()
    for mode in K.MODES:
        file = np.frombuffer(K.written(201, 333, mode), np.uint8)
        info = _ffi.JpegInfo.array()
        assert lib.lars_jpeg_info(_ffi.ptr(file), file.size, info) == 0
        full = lib.lars_jpeg_decode_scratch_bytes(info)
        assert full > 0 and lib.lars_jpeg_decode_scaled_scratch_bytes(info, 1) == full
        sizes = [lib.lars_jpeg_decode_scaled_scratch_bytes(info, s) for s in (2, 4, 8)]
        assert full > sizes[0] > sizes[1] > sizes[2] > 0, (mode, full, sizes)   # the planes shrink, the entropy stage does not
        for bad in (0, 3, 5, 16, -1):
            assert lib.lars_jpeg_decode_scaled_scratch_bytes(info, bad) == 0
    assert lib.lars_jpeg_decode_scaled_scratch_bytes(None, 2) == 0


@pytest.mark.skipif(_ffi.device_count() > 0, reason="only meaningful without a GPU")
def test_no_cpu_fallback_for_the_scaled_decoder():
    b = K.written(33, 5, "420")
    with pytest.raises(_ffi.LarsError) as e:
        lars.decode_jpeg(b, 2)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
    with pytest.raises(_ffi.LarsError):
        lars.thumbnail_jpeg(K.written(201, 333, "420"), (40, 40), 2.0, scaled=True)
