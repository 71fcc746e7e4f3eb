"""encode_jpeg / jpeg_encoder="device" on the GPU (csrc/jpeg_encode.hip): every file equals Pillow's, byte for byte."""
import ctypes as C
import io
import sys
import threading
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_forward_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")
QUALITIES = (1, 10, 50, 75, 90, 95, 100)


def pillow(arr, quality=75, subsampling="4:2:0"):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG", quality=quality, subsampling=subsampling)
    return f.getvalue()


def same(arr, quality=75, subsampling="4:2:0", name=None):
    got, ref = lars.encode_jpeg(arr, quality, subsampling), pillow(arr, quality, subsampling)
    if got != ref:
        first = next((i for i in range(min(len(got), len(ref))) if got[i] != ref[i]), min(len(got), len(ref)))
        raise AssertionError(f"{name or arr.shape} q{quality} {subsampling}: {len(got)} bytes against Pillow's {len(ref)}, first difference at {first}")
    return got


def picture(kind, h, w, c, seed=0):
    shape = (h, w, c) if c > 1 else (h, w)
    if kind == "flat":
        a = np.empty((h, w, 3), np.uint8)
        a[:] = (200, 90, 30)
        return a if c > 1 else a[:, :, 0].copy()
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        a = np.dstack([(y * 2 + x) % 256, (x * 3) % 256, 255 - (y * 2) % 256]).astype(np.uint8)
        return a if c > 1 else a[:, :, 0].copy()
    if kind == "1f":
        return fm.one_over_f(h, w, c, seed + h * w) if min(h, w) > 1 else np.full(shape, 77, np.uint8)
    if kind == "noise":
        return np.random.default_rng(seed + h + w).integers(0, 256, shape, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "ones":
        return np.full(shape, 255, np.uint8)
    assert kind == "primaries"                               # saturated primaries and their complements in 5 x 7 patches
    colours = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)], np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    a = colours[(y // 5 * 3 + x // 7) % 8]
    return a if c > 1 else a[:, :, 0].copy()


KINDS = ("flat", "smooth", "1f", "noise", "zeros", "ones", "primaries")


@pytest.mark.parametrize("kind", KINDS)
def test_files_equal_pillows(kind):
    """L and RGB, the three samplings, seven qualities; the saturated contents exercise the + 32767 rounding of Cb / Cr."""
    for h, w in ((97, 131), (64, 64)):
        for quality in QUALITIES:
            same(picture(kind, h, w, 1), quality, "4:4:4", kind)
            for s in SAMPLINGS:
                same(picture(kind, h, w, 3), quality, s, kind)


def test_every_small_size_at_420():
    """Every height and width from 1 to 33: both bottom-edge rules (H % 16 == 8) and the dummy luminance blocks."""
    for h in range(1, 34):
        for w in range(1, 34):
            same(picture("noise", h, w, 3, seed=7), 75, "4:2:0")


def test_small_sizes_at_422_444_and_l():
    for h in (1, 2, 7, 8, 9, 15, 16, 17, 24, 33):
        for w in range(1, 34):
            a = picture("noise", h, w, 3, seed=3)
            same(a, 90, "4:2:2")
            same(a, 30, "4:4:4")
            for s in (0, 1, 2):                             # one component: only the frame header shows the sampling
                same(a[:, :, 1].copy(), 75, s)


def test_subsampling_numbers_are_pillows_names():
    a = picture("1f", 40, 56, 3)
    for n, s in enumerate(SAMPLINGS):
        assert lars.encode_jpeg(a, 75, n) == lars.encode_jpeg(a, subsampling=s) == pillow(a, 75, s)
    assert lars.encode_jpeg(a) == pillow(a)
    assert lars.encode_jpeg(a[:, :, :1]) == lars.encode_jpeg(a[:, :, 0].copy()) == pillow(a[:, :, 0].copy())


@pytest.mark.parametrize("h, w, c", [(1536, 2048, 3), (4096, 4096, 3), (1, 65500, 3), (65500, 1, 3), (1, 65500, 1), (65500, 1, 1)])
def test_large_and_extreme_shapes(h, w, c):
    a = picture("1f", h, w, c) if min(h, w) > 1 else picture("noise", h, w, c)
    same(a)
    if (h, w) == (1536, 2048):
        same(a, 95, "4:4:4")
        same(a[:, :, 0].copy(), 50, "4:4:4")
        same(picture("noise", h, w, 3), 100, "4:2:2")


def test_round_trip_through_both_device_codecs():
    for c, s in ((1, "4:4:4"), (3, "4:4:4"), (3, "4:2:2"), (3, "4:2:0")):
        a = picture("1f", 120, 171, c)
        b = lars.encode_jpeg(a, 85, s)
        ref = np.asarray(Image.open(io.BytesIO(pillow(a, 85, s))))
        got = lars.decode_jpeg(b)
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


def device_entry_point_with_guards(a, quality, sub):
    """lars_d_encode_jpeg_u8 on a caller's stream, output and scratch in the middle of guarded buffers: the reported length is the
    file's, the file is Pillow's, nothing outside is written."""
    h, w = a.shape[:2]
    c = 1 if a.ndim == 2 else 3
    lib = _ffi.load()
    cap, need = lib.lars_jpeg_bound(h, w, c, sub), lib.lars_jpeg_encode_scratch_bytes(h, w, c, sub)
    assert cap > 0 and need > 0
    guard = 4096
    d_in, d_out, d_scratch, d_len, stream = (C.c_void_p() for _ in range(5))
    _ffi.call("lars_malloc", C.byref(d_in), a.nbytes)
    _ffi.call("lars_malloc", C.byref(d_out), cap + 2 * guard)
    _ffi.call("lars_malloc", C.byref(d_scratch), need + 2 * guard)
    _ffi.call("lars_malloc", C.byref(d_len), 8)
    _ffi.call("lars_stream_create", C.byref(stream))
    try:
        _ffi.call("lars_memcpy_h2d", d_in, _ffi.ptr(a), a.nbytes)
        _ffi.call("lars_memset", d_out, 0xA5, cap + 2 * guard, stream)
        _ffi.call("lars_memset", d_scratch, 0x5A, need + 2 * guard, stream)
        _ffi.call("lars_d_encode_jpeg_u8", d_in, h, w, c, quality, sub, C.c_void_p(d_out.value + guard), cap, d_len,
                  C.c_void_p(d_scratch.value + guard), stream)
        _ffi.call("lars_synchronize", stream)
        out = np.empty(cap + 2 * guard, np.uint8)
        scr = np.empty(need + 2 * guard, np.uint8)
        n = np.zeros(1, np.int64)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(out), d_out, out.size)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(scr), d_scratch, scr.size)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(n), d_len, 8)
    finally:
        _ffi.call("lars_stream_destroy", stream)
        for p in (d_in, d_out, d_scratch, d_len):
            _ffi.call("lars_free", p)
    ref = pillow(a, quality, sub)
    assert int(n[0]) == len(ref) <= cap
    assert out[guard:guard + len(ref)].tobytes() == ref
    assert (out[:guard] == 0xA5).all() and (out[guard + len(ref):] == 0xA5).all()      # nothing before, nothing past the file
    assert (scr[:guard] == 0x5A).all() and (scr[-guard:] == 0x5A).all()


def test_noise_at_quality_100_fits_the_bound_and_the_guards_hold():
    for h, w, c, sub in ((100, 150, 3, 0), (64, 64, 1, 0), (33, 47, 3, 2), (120, 9, 3, 1), (1, 1, 3, 2), (256, 256, 3, 0)):
        a = picture("noise", h, w, c)
        b = lars.encode_jpeg(a, 100, sub)
        assert len(b) <= api.jpeg_bound(h, w, c, sub)
        device_entry_point_with_guards(a, 100, sub)
    device_entry_point_with_guards(picture("1f", 97, 131, 3), 75, 2)
    device_entry_point_with_guards(picture("ones", 40, 40, 3), 1, 2)


def test_entry_point_refuses_a_short_output_buffer():
    d = C.c_void_p()
    _ffi.call("lars_malloc", C.byref(d), 1 << 20)
    try:
        cap = _ffi.load().lars_jpeg_bound(16, 16, 3, 2)
        with pytest.raises(_ffi.LarsError, match="lars_jpeg_bound"):
            _ffi.call("lars_d_encode_jpeg_u8", d, 16, 16, 3, 75, 2, d, cap - 1, d, d, None)
        with pytest.raises(_ffi.LarsError, match="quality"):
            _ffi.call("lars_d_encode_jpeg_u8", d, 16, 16, 3, 0, 2, d, cap, d, d, None)
    finally:
        _ffi.call("lars_free", d)


def test_white_balance_file_written_by_the_device(tmp_path):
    src = tmp_path / "camera.JPG"
    Image.fromarray(picture("1f", 240, 320, 3)).save(src, quality=92)
    assert lars.fix_white_balance_rgnir(src, tmp_path / "a_corrected.jpg") is None
    assert lars.fix_white_balance_rgnir(src, tmp_path / "b_corrected.jpg", jpeg_encoder="device") is None
    a, b = (tmp_path / "a_corrected.jpg").read_bytes(), (tmp_path / "b_corrected.jpg").read_bytes()
    assert len(a) > 1000 and a == b
    assert b == lars.encode_jpeg(lars.fix_white_balance_rgnir(src))


def test_same_input_same_bytes():
    a = picture("1f", 301, 457, 3)
    first = lars.encode_jpeg(a, 90)
    for _ in range(5):
        assert lars.encode_jpeg(a, 90) == first
    small = picture("noise", 9, 9, 3)
    big = picture("noise", 200, 300, 3)
    want = lars.encode_jpeg(small)
    lars.encode_jpeg(big, 100, "4:4:4")                      # a larger call in between leaves nothing behind in the workspace
    assert lars.encode_jpeg(small) == want == pillow(small)


def test_concurrent_calls_from_threads():
    nthreads, rounds = 4, 6
    pictures = [picture("1f" if k % 2 else "noise", 150 + 37 * k, 200 + 53 * k, 3 if k % 3 else 1, seed=k) for k in range(nthreads)]
    settings = [(75, "4:2:0"), (95, "4:4:4"), (40, "4:2:2"), (100, "4:2:0")]
    refs = [pillow(p, *s) for p, s in zip(pictures, settings)]
    errors, barrier = [], threading.Barrier(nthreads)

    def session(k):
        try:
            barrier.wait()
            for _ in range(rounds):
                if lars.encode_jpeg(pictures[k], *settings[k]) != refs[k]:
                    errors.append(f"thread {k}: bytes differ")
        except Exception as e:                               # noqa: BLE001
            errors.append(f"thread {k}: {e!r}")

    threads = [threading.Thread(target=session, args=(k,)) for k in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
