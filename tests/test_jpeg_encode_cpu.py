"""CPU side of the device JPEG encoder (api.encode_jpeg): argument checks before the library is called, the host-built header
and tables against Pillow's files for every quality, the NumPy forward model (tests/jpeg_forward_model.py) against the
coefficients of Pillow's own files, lars_jpeg_bound, the exports, and the sanitizer build replaying the host code."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_forward_model as fm  # noqa: E402
import jpeg_writer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lars_image_processing_amd", "csrc")
ASAN_BIN = os.path.join(ROOT, "build", "asan", "lars_host_asan")
SUB = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def _no_device(*_a, **_k):
    raise AssertionError("the library was called")


def noise(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------------------
RGB = np.zeros((8, 8, 3), np.uint8)


@pytest.mark.parametrize("args, kwargs, exc", [
    ((np.zeros((8, 8, 3), np.uint16),), {}, TypeError),
    ((np.zeros((8, 8, 3), np.float32),), {}, TypeError),
    ((np.zeros((8, 8, 4), np.uint8),), {}, TypeError),                      # RGBA: Pillow refuses it too
    ((np.zeros((8,), np.uint8),), {}, ValueError),
    ((np.zeros((8, 8, 2), np.uint8),), {}, ValueError),
    ((np.zeros((2, 8, 8, 3), np.uint8),), {}, ValueError),
    ((RGB,), {"quality": 0}, ValueError),
    ((RGB,), {"quality": 101}, ValueError),
    ((RGB,), {"quality": 7.5}, TypeError),
    ((RGB,), {"subsampling": "4:1:1"}, ValueError),
    ((RGB,), {"subsampling": 3}, ValueError),
    ((RGB,), {"subsampling": None}, ValueError),
    ((np.zeros((0, 8, 3), np.uint8),), {}, ValueError),
    ((np.zeros((8, 0), np.uint8),), {}, ValueError),
    ((np.zeros((65501, 1), np.uint8),), {}, ValueError),
    ((np.zeros((1, 65501, 3), np.uint8),), {}, ValueError),
])
def test_encode_jpeg_refuses_before_the_library(monkeypatch, args, kwargs, exc):
    monkeypatch.setattr(_ffi, "call", _no_device)
    with pytest.raises(exc, match="encode_jpeg"):
        api.encode_jpeg(*args, **kwargs)


def test_bad_jpeg_encoder_refused_before_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_ffi, "call", _no_device)
    from PIL import Image
    src = tmp_path / "a.png"
    Image.fromarray(noise(8, 8, 3)).save(src)
    for bad in ("gpu", None, "Device"):
        with pytest.raises(ValueError, match="jpeg_encoder"):
            api.fix_white_balance_rgnir(src, tmp_path / "out.jpg", jpeg_encoder=bad)
    assert not (tmp_path / "out.jpg").exists()


def test_device_encoder_is_used_for_jpeg_paths_only(monkeypatch, tmp_path):
    """The switch sends .jpg / .jpeg save paths to encode_jpeg and every other path, and the default, to Pillow (the white balance
    itself is replaced here: it needs the device)."""
    from PIL import Image
    src = tmp_path / "a.png"
    a = noise(16, 24, 3)
    Image.fromarray(a).save(src)
    calls = []
    monkeypatch.setattr(api, "_wb_array", lambda arr, variant: arr)
    monkeypatch.setattr(api, "encode_jpeg", lambda arr: calls.append(arr.shape) or fm.pillow_file(arr))
    api.fix_white_balance_rgnir(src, tmp_path / "x.JPG", jpeg_encoder="device")
    api.fix_white_balance_rgnir(src, str(tmp_path / "y.jpeg"), jpeg_encoder="device")
    assert calls == [(16, 24, 3)] * 2
    api.fix_white_balance_rgnir(src, tmp_path / "z.png", jpeg_encoder="device")
    api.fix_white_balance_rgnir(src, tmp_path / "w.jpg")
    assert calls == [(16, 24, 3)] * 2
    assert (tmp_path / "x.JPG").read_bytes() == (tmp_path / "w.jpg").read_bytes() == fm.pillow_file(a)
    assert np.array_equal(np.array(Image.open(tmp_path / "z.png")), a)


def test_encode_jpeg_is_exported():
    assert "encode_jpeg" in api.__all__
    assert lars.encode_jpeg is api.encode_jpeg
    for name in ("lars_jpeg_bound", "lars_jpeg_header", "lars_jpeg_encode_scratch_bytes", "lars_d_encode_jpeg_u8", "lars_h_encode_jpeg_u8"):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name)


# ---------------------------------------------------------------------------------------------------------------------
# header and tables (host code)
# ---------------------------------------------------------------------------------------------------------------------
def lib_header(h, w, c, sub, quality, cap=640):
    out = np.zeros(max(cap, 1), np.uint8)
    n = _ffi.load().lars_jpeg_header(h, w, c, sub, quality, _ffi.ptr(out), cap)
    return out[:n].tobytes() if n > 0 else None


def pillow_header(arr, **save):
    d = fm.pillow_file(arr, **save)
    return d[:fm.segments(d)[1]]


def test_header_equals_pillows_for_every_quality(monkeypatch):
    monkeypatch.setattr(_ffi, "call", _no_device)
    for quality in range(1, 101):
        assert lib_header(9, 13, 1, 0, quality) == pillow_header(noise(9, 13, 1), quality=quality), quality
        assert lib_header(9, 13, 1, 2, quality) == pillow_header(noise(9, 13, 1), quality=quality, subsampling="4:2:0"), quality
        for name, sub in SUB.items():
            want = pillow_header(noise(9, 13, 3), quality=quality, subsampling=name)
            assert lib_header(9, 13, 3, sub, quality) == want, (quality, name)


@pytest.mark.parametrize("h, w", [(1, 1), (8, 8), (255, 256), (257, 1), (1, 300), (1030, 515)])
def test_header_frame_fields(h, w):
    for c in (1, 3):
        a = np.zeros((h, w, c) if c > 1 else (h, w), np.uint8)
        assert lib_header(h, w, c, 2, 75) == pillow_header(a, subsampling=2)
        assert lib_header(h, w, c, 1, 30) == pillow_header(a, quality=30, subsampling=1)


def test_header_of_the_largest_sides():
    """65500 is libjpeg's limit; only the frame header depends on the size, so Pillow's small file is patched to it."""
    for h, w in ((65500, 1), (1, 65500), (65500, 32000)):
        ref = bytearray(pillow_header(np.zeros((8, 8), np.uint8), subsampling=0))
        sof = ref.index(b"\xff\xc0")
        ref[sof + 5:sof + 9] = struct.pack(">HH", h, w)
        assert lib_header(h, w, 1, 0, 75) == bytes(ref)


def test_header_refuses_bad_arguments():
    assert lib_header(8, 8, 3, 2, 75, cap=100) is None
    assert lib_header(8, 8, 3, 2, 75, cap=622) is None and len(lib_header(8, 8, 3, 2, 75, cap=623)) == 623
    for h, w, c, sub, q in ((0, 8, 3, 2, 75), (8, 65501, 1, 0, 75), (8, 8, 4, 2, 75), (8, 8, 2, 0, 75), (8, 8, 3, 3, 75),
                            (8, 8, 3, -1, 75), (8, 8, 3, 2, 0), (8, 8, 3, 2, 101), (40000, 40000, 3, 2, 75)):
        assert lib_header(h, w, c, sub, q) is None, (h, w, c, sub, q)
    assert _ffi.load().lars_jpeg_header(8, 8, 3, 2, 75, None, 640) == 0


def test_model_tables_are_pillows():
    for quality in (1, 2, 24, 25, 49, 50, 51, 75, 90, 99, 100):
        _coefs, q = fm.pillow_coefs(fm.pillow_file(noise(8, 8, 3), quality=quality))
        assert q == fm.quant_tables(quality), quality


# ---------------------------------------------------------------------------------------------------------------------
# the forward model against Pillow's coefficients
# ---------------------------------------------------------------------------------------------------------------------
def content(kind, h, w, c):
    if kind == "1f":
        return fm.one_over_f(h, w, c, h * w) if min(h, w) > 1 else np.full((h, w, c) if c > 1 else (h, w), 77, np.uint8)
    return noise(h, w, c, h + w)


MODEL_SIZES = [(97, 131), (64, 64), (8, 8), (1, 1), (17, 250), (120, 9), (2, 2), (20, 40), (30, 15), (44, 33), (10, 100), (22, 7)]
MODEL_SAVES = [("RGB", {}), ("RGB", dict(quality=95)), ("RGB", dict(quality=90, subsampling=1)), ("RGB", dict(quality=30, subsampling=0)),
               ("L", {}), ("L", dict(quality=100)), ("RGB", dict(quality=100, subsampling=2)), ("RGB", dict(quality=1))]


def check_model(arr, save):
    d = fm.pillow_file(arr, **save)
    want, _q = fm.pillow_coefs(d)
    got, sampling = fm.forward(arr, save.get("quality", 75), save.get("subsampling", 2))
    assert got.shape == want.shape and np.array_equal(got, want), (arr.shape, save, int((got != want).sum()))
    return d, got, sampling


@pytest.mark.parametrize("h, w", MODEL_SIZES)
def test_forward_model_gives_pillows_coefficients(h, w):
    """The 192 cases the model was first checked on: 12 sizes x 8 ways of saving x 1/f scenes and noise."""
    for mode, save in MODEL_SAVES:
        for kind in ("1f", "noise"):
            check_model(content(kind, h, w, 1 if mode == "L" else 3), save)


@pytest.mark.parametrize("subsampling", [2, 1])
def test_forward_model_on_every_edge_residue(subsampling):
    """Every height and width from 1 to 40 at 4:2:0 and 4:2:2: both bottom-edge rules (H % 16 == 8 at 4:2:0) and the dummy
    luminance blocks of an odd block count."""
    for h in range(1, 41):
        for w in range(1, 41):
            check_model(noise(h, w, 3, 41 * h + w), dict(subsampling=subsampling))


def split_file(d):
    segs, p = fm.segments(d)
    return [s for _m, s in segs], d[p:]


@pytest.mark.parametrize("mode, save", MODEL_SAVES + [("RGB", dict(subsampling=1)), ("RGB", dict(quality=10, subsampling=0))])
def test_model_coefficients_make_pillows_file(mode, save):
    """Model coefficients + the suite's writer + the standard tables, no restart interval = Pillow's file.  For one component
    that is the whole file, byte for byte.  For three the writer puts its DHT segments in the order DC 0, DC 1, AC 0, AC 1 and
    Pillow DC 0, AC 0, DC 1, AC 1: there the same segments are required in any order, SOI / APP0 / DQTs / SOF0 and SOS in
    place, and everything from the entropy data to EOI byte for byte."""
    _q, hts = fm.standard_tables()
    for h, w in ((97, 131), (8, 40), (24, 17), (1, 1)):
        arr = content("1f", h, w, 1 if mode == "L" else 3)
        d, coefs, sampling = check_model(arr, save)
        qts = fm.quant_tables(save.get("quality", 75))
        if mode == "L":
            got = jpeg_writer.write(w, h, None, coefs, qts, {k: v for k, v in hts.items() if k[1] == 0}, tq=(0,), td=(0,), ta=(0,), ri=0, split=True)
            assert got == d
            continue
        got = jpeg_writer.write(w, h, sampling, coefs, qts, hts, ri=0, split=True)
        gs, gdata = split_file(got)
        ws, wdata = split_file(d)
        assert gdata == wdata
        assert len(gs) == len(ws) == 9 and sorted(gs) == sorted(ws)
        assert gs[:4] == ws[:4] and gs[8] == ws[8]
        assert got[:2] == d[:2] == b"\xff\xd8"


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
def test_bound_is_monotonic_and_zero_for_what_cannot_be_encoded():
    b = _ffi.load().lars_jpeg_bound
    for c, sub in ((1, 0), (3, 0), (3, 1), (3, 2)):
        prev = 0
        for n in (1, 7, 8, 9, 16, 17, 100, 1000, 4096):
            assert b(n, 33, c, sub) >= b(max(n - 1, 1), 33, c, sub) and b(33, n, c, sub) >= b(33, max(n - 1, 1), c, sub)
            assert b(n, n, c, sub) >= prev > -1
            prev = b(n, n, c, sub)
        assert b(8, 8, c, sub) < b(17, 17, c, sub) < b(100, 100, c, sub) < b(100, 4096, c, sub) < b(4096, 4096, c, sub)
    assert api.jpeg_bound(8, 8, 1) == b(8, 8, 1, 0) > 0
    for h, w, c, sub in ((0, 8, 1, 0), (8, 0, 3, 2), (65501, 8, 1, 0), (8, 65501, 3, 0), (8, 8, 2, 0), (8, 8, 4, 2), (8, 8, 3, 3),
                         (8, 8, 3, -1), (-1, 8, 1, 0), (46341, 46341, 1, 0), (30000, 30000, 3, 2)):
        assert b(h, w, c, sub) == 0, (h, w, c, sub)
    assert b(65500, 1, 1, 0) > 0 and b(1, 65500, 3, 2) > 0 and b(46340, 46340, 1, 2) > 0


def test_bound_holds_for_noise_at_quality_100():
    b = _ffi.load().lars_jpeg_bound
    for h, w in ((1, 1), (8, 8), (17, 33), (100, 150), (256, 256)):
        for c in (1, 3):
            assert len(fm.pillow_file(noise(h, w, c), quality=100, subsampling=0)) <= b(h, w, c, 0)
    # the longest block there is: every coefficient at the category-10 code of 16 bits, behind a 9 + 11 bit DC term
    assert b(8, 8, 1, 0) == len(lib_header(8, 8, 1, 0, 75)) + 2 * ((9 + 11 + 63 * 26 + 7) // 8) + 2


# ---------------------------------------------------------------------------------------------------------------------
# the sanitizer build (same skip rules as test_asan_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan_bin():
    if _ffi.device_count() > 0:
        pytest.skip("sanitizer target is for the build container, not the GPU box")
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", CSRC, "asan"], stdout=subprocess.DEVNULL)
    return ASAN_BIN


def fnv(data):
    h = 1469598103934665603
    for byte in bytes(data):
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_sanitizer_replays_header_and_bound(asan_bin, tmp_path):
    cases = []                                               # (cap, h, w, channels, subsampling, quality)
    for quality in range(1, 101):
        cases += [(640, 9, 13, 1, 0, quality)] + [(640, 9, 13, 3, sub, quality) for sub in (0, 1, 2)]
    for h, w in ((1, 1), (65500, 1), (1, 65500), (65500, 65500), (4096, 4096), (0, 5), (5, 65501), (40000, 40000)):
        cases += [(640, h, w, 1, 0, 75), (640, h, w, 3, 2, 75)]
    cases += [(cap, 8, 8, c, 2, 75) for c in (1, 3) for cap in (0, 1, 100, 329, 330, 331, 622, 623, 624)]   # exact-size buffers
    cases += [(640, 8, 8, c, sub, q) for c, sub, q in ((2, 0, 75), (4, 2, 75), (3, 3, 75), (3, -1, 75), (3, 2, 0), (3, 2, 101))]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for cap, *v in cases:
            f.write(struct.pack("<4I", 5, cap, 0, 20) + struct.pack("<5i", *v))
    run = subprocess.run([asan_bin, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == f"done {len(cases)} cases"
    ok = 0
    for line, (cap, h, w, c, sub, q) in zip(lines, cases):
        head = lib_header(h, w, c, sub, q, cap)
        n, hh = (len(head), fnv(head)) if head else (0, 0)
        assert line.split(" ", 1)[1] == f"jpeghead n={n} h={hh:016x} bound={_ffi.load().lars_jpeg_bound(h, w, c, sub)}", line
        ok += n > 0
    assert ok >= 400
