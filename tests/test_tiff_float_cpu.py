"""Float32 TIFF without a device: the NumPy model of the floating-point predictor (tiff_float_model.py) against itself and
against Pillow's libtiff, tiffio.read_tiff / write_float_tiff against Pillow and against each other in every layout,
lars_tiff_info against read_tiff, the refusals that stay, the encoder's bound and its argument errors.  Equality is always on
the 32-bit patterns: NaN payloads, infinities, denormals and -0.0 have to survive."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
import lzw_writer as lz
import tiff_float_model as fm
from lars_image_processing_amd import _ffi, api, codecs, tiffio
from test_abi_cpu import exported_symbols, header_symbols
from test_tiff_decode_cpu import agree, asan_bin, fnv  # noqa: F401  (asan_bin is a fixture)

F32_NAMES = ("lars_tiff_f32_bound", "lars_tiff_f32_encode_scratch_bytes", "lars_d_encode_tiff_f32", "lars_h_encode_tiff_f32",
             "lars_h_process_image_tiff_f32")


def same_bits(got, want):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def written(a, **kw):
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "f.tif")
        n = tiffio.write_float_tiff(p, a, **kw)
        with open(p, "rb") as f:
            blob = f.read()
    assert n == len(blob)
    return blob


def pillow_file(a, compression=None, predictor=1):
    buf = io.BytesIO()
    kw = {}
    if compression:
        kw["compression"] = compression
    if predictor != 1:
        kw["tiffinfo"] = {317: predictor}
    Image.fromarray(a).save(buf, format="TIFF", **kw)
    return buf.getvalue()


def strips_of(blob):
    tags = tiffio._read_ifd(memoryview(blob), "<")
    return tags, [blob[o:o + n] for o, n in zip(tags[tiffio.STRIP_OFFSETS], tags[tiffio.STRIP_BYTE_COUNTS])]


@pytest.mark.parametrize("samples", [1, 2, 3, 5])
def test_model_round_trip_on_random_bit_patterns(samples):
    for w in (1, 2, 7, 16):
        a = fm.values("bits", (5, w * samples), seed=samples * 100 + w)
        stored = fm.forward(a, samples)
        assert stored.shape == (5, 4 * w * samples) and stored.dtype == np.uint8
        assert np.array_equal(fm.inverse(stored, samples), a.view(np.uint32))
        # the first `samples` bytes of a row are the most significant bytes of its first pixel, as they are
        assert np.array_equal(stored[:, :samples], (a.view(np.uint32)[:, :samples] >> 24).astype(np.uint8))
    # across a plane border: one pixel of one sample, bytes MSB first, each minus the one before
    one = np.array([[0x11223344]], dtype=np.uint32)
    assert fm.forward(one, 1).tolist() == [[0x11, 0x11, 0x11, 0x11]]


@pytest.mark.parametrize("kind", ["smooth", "bits"])
def test_model_against_pillow(kind):
    """Pillow's (libtiff's) LZW + Predictor 3 strips are undone by a plain LZW decoder plus the model, and the model plus the
    greedy encoder reproduce them byte for byte."""
    a = fm.values(kind, (70, 90), seed=3)
    blob = pillow_file(a, "tiff_lzw", 3)
    tags, strips = strips_of(blob)
    assert tags[tiffio.PREDICTOR] == (3,) and tags[tiffio.BITS_PER_SAMPLE] == (32,) and tags[tiffio.SAMPLE_FORMAT] == (3,)
    rps = min(tags[tiffio.ROWS_PER_STRIP][0], 70)
    assert len(strips) == -(-70 // rps)
    for k, strip in enumerate(strips):
        rows = a[k * rps:(k + 1) * rps]
        plain = lz.plaintext(lz.unpack(strip))
        stored = np.frombuffer(plain, dtype=np.uint8).reshape(rows.shape[0], 4 * 90)
        assert np.array_equal(fm.inverse(stored, 1), rows.view(np.uint32)), k
        assert lz.pack(lz.encode(fm.forward(rows, 1).tobytes(), clear_at=4094)) == strip, k
        assert fm.strip_bytes(a[..., None], k * rps, rps, True) == plain


@pytest.mark.parametrize("compression", ["tiff_lzw", "tiff_adobe_deflate"])
@pytest.mark.parametrize("predictor", [1, 2, 3])
def test_read_tiff_on_pillow_files(compression, predictor):
    for kind, shape in (("bits", (33, 47)), ("smooth", (70, 90)), ("constant", (9, 300)), ("bits", (1, 1))):
        a = fm.values(kind, shape, seed=predictor)
        blob = pillow_file(a, compression, predictor)
        assert tiffio._read_ifd(memoryview(blob), "<").get(tiffio.PREDICTOR, (1,)) == (predictor,)
        got = tiffio.read_tiff(blob)
        same_bits(got, a)
        same_bits(got, np.asarray(Image.open(io.BytesIO(blob))))
    same_bits(tiffio.read_tiff(pillow_file(a)), a)                      # uncompressed


LAYOUTS = [{"rows_per_strip": 4}, {}, {"tile": (16, 16)}, {"tile": (32, 48)}]


def every_combination():
    """(name, array, file) for samples 1 / 3 / 5, strips / tiles, chunky / planar, both byte orders, none / LZW / Deflate,
    predictor 1 / 2 / 3, on a 20 x 34 picture: both tile sizes are cropped on the right and at the bottom."""
    seed = 0
    for c in (1, 3, 5):
        for layout in LAYOUTS:
            for planar in (1, 2):
                for byteorder in ("<", ">"):
                    for comp in ("none", "lzw", "deflate"):
                        for predictor in (1, 2, 3):
                            seed += 1
                            a = fm.values(("bits", "smooth")[seed % 2], (20, 34) if c == 1 else (20, 34, c), seed)
                            kw = dict(layout, planar=planar, byteorder=byteorder, predictor=predictor, lzw=comp == "lzw", deflate=comp == "deflate")
                            yield f"c{c}{layout}{planar}{byteorder}{comp}{predictor}", a, written(a, **kw), kw


@pytest.fixture(scope="module")
def combos():
    return list(every_combination())


def test_read_tiff_reads_every_write_float_tiff_combination(combos):
    assert len(combos) == 3 * 4 * 2 * 2 * 3 * 3
    for name, a, blob, kw in combos:
        same_bits(tiffio.read_tiff(blob), a)
        tags = tiffio._read_ifd(memoryview(blob), kw["byteorder"])
        c = a.shape[2] if a.ndim == 3 else 1
        assert tags[tiffio.BITS_PER_SAMPLE] == (32,) * c and tags[tiffio.SAMPLE_FORMAT] == (3,) * c, name
        assert tags[tiffio.COMPRESSION] == ({"none": 1, "lzw": 5, "deflate": 8}["lzw" if kw["lzw"] else "deflate" if kw["deflate"] else "none"],)
        assert tags.get(tiffio.PREDICTOR, (1,)) == (kw["predictor"],)


def test_pillow_reads_write_float_tiff_files(combos):
    """Every little-endian single-sample file.  LZW and Deflate files go through libtiff, which undoes the predictor: the same
    bits.  An uncompressed file Pillow reads with its own raw decoder, which knows no predictor (measured: for Predictor 2 and
    3 it hands back the stored differences; libtiff itself applies a predictor only inside its LZW / Deflate codecs), so there
    Pillow vouches for the stored bytes and the model undoes them: the same bits again.  read_tiff applies the tag whatever the
    compression, as it always has for Predictor 2 on integer files."""
    seen = 0
    for name, a, blob, kw in combos:
        if a.ndim == 2 and kw["byteorder"] == "<":
            got = np.asarray(Image.open(io.BytesIO(blob)))
            if not (kw["lzw"] or kw["deflate"]) and kw["predictor"] != 1 and "tile" not in kw:
                stored = np.ascontiguousarray(got).view(np.uint32)
                if kw["predictor"] == 2:
                    got = np.cumsum(stored, axis=1, dtype=np.uint32).view(np.float32)
                else:
                    got = fm.inverse(stored.astype("<u4").view(np.uint8).reshape(a.shape[0], -1), 1).view(np.float32)
                same_bits(got, a)
            elif not (kw["lzw"] or kw["deflate"]) and kw["predictor"] != 1:
                assert got.shape == a.shape and got.dtype == np.float32      # tiles: the padding columns take part, Pillow crops them
            else:
                same_bits(got, a)
            seen += 1
    assert seen == 4 * 2 * 3 * 3


def test_lzw_strips_of_write_float_tiff_are_libtiffs():
    a = fm.values("smooth", (40, 50, 3), seed=1)
    for predictor in (1, 3):
        _tags, strips = strips_of(written(a, rows_per_strip=7, lzw=True, predictor=predictor))
        for k, strip in enumerate(strips):
            assert strip == lz.pack(lz.encode(fm.strip_bytes(a, 7 * k, 7, predictor == 3), clear_at=4094))
    noise = np.random.default_rng(1).integers(0, 256, 20000, dtype=np.uint8).tobytes()
    assert tiffio._lzw_encode(noise) == lz.pack(lz.encode(noise, clear_at=4094))          # five Clears of a full table
    assert tiffio._lzw_encode(b"") == lz.pack([lz.CLEAR, lz.EOI])


def test_write_float_tiff_arguments(tmp_path):
    p = tmp_path / "x.tif"
    ok = np.zeros((4, 4), np.float32)
    for bad in (ok.astype(np.float64), ok.astype(np.uint16), np.zeros((0, 4), np.float32), np.zeros(5, np.float32)):
        with pytest.raises(tiffio.TiffError, match="float32"):
            tiffio.write_float_tiff(p, bad)
    for kw in ({"predictor": 0}, {"predictor": 4}, {"predictor": True}, {"lzw": True, "deflate": True}, {"byteorder": "="}, {"planar": 3},
               {"tile": (8, 16)}):
        with pytest.raises(tiffio.TiffError):
            tiffio.write_float_tiff(p, ok, **kw)
    with pytest.raises(tiffio.TiffError):
        tiffio.write_tiff(p, np.zeros((4, 4, 3), np.float32))          # the integer writer goes on refusing floats


def test_tiff_info_agrees_with_read_tiff(combos):
    for name, a, blob, kw in combos:
        deflate = kw["deflate"]
        outcome = agree(name, blob)                                     # dtype and shape; supported unless Deflate
        assert outcome == "read"
        for flag in (False, True):
            info = api.tiff_info(blob, deflate=flag)
            assert info["dtype"] == np.float32 and info["shape"] == a.shape and info["bits"] == 32, name
            assert info["supported"] == (flag or not deflate) and (info["reason"] is None) == info["supported"], name
            assert info["big_endian"] == (kw["byteorder"] == ">")
            if info["supported"]:                                       # the walk stops at the compression of a file it refuses
                assert info["predictor"] == kw["predictor"] and info["planar"] == kw["planar"] and info["tiled"] == ("tile" in kw), name
    for predictor in (1, 2, 3):
        blob = pillow_file(fm.values("smooth", (30, 40), 2), "tiff_lzw", predictor)
        assert agree("pillow", blob) == "read" and api.tiff_info(blob)["predictor"] == predictor


def patched(blob, tag, value):
    """The little-endian file with the first (inline SHORT) value of ``tag`` replaced."""
    out = bytearray(blob)
    (ifd,) = struct.unpack_from("<I", blob, 4)
    for i in range(struct.unpack_from("<H", blob, ifd)[0]):
        at = ifd + 2 + 12 * i
        if struct.unpack_from("<H", blob, at)[0] == tag:
            assert struct.unpack_from("<HI", blob, at + 2) == (3, 1)
            struct.pack_into("<H", out, at + 8, value)
            return bytes(out)
    raise AssertionError(f"no tag {tag}")


def test_refusals_that_stay(tmp_path):
    reasons = codecs._TIFF_REASONS
    f32 = written(fm.values("smooth", (8, 8), 0), predictor=3)
    assert api.tiff_info(f32)["supported"]
    # predictor 3 without float samples
    for dtype in (np.uint8, np.uint16):
        tiffio.write_tiff(tmp_path / "u.tif", np.zeros((8, 8), dtype), predictor=True)
        bad = patched((tmp_path / "u.tif").read_bytes(), tiffio.PREDICTOR, 3)
        assert agree("p3-int", bad) == reasons["PREDICTOR"]
        with pytest.raises(tiffio.TiffError, match="predictor 3"):
            tiffio.read_tiff(bad)
    assert agree("p4", patched(f32, tiffio.PREDICTOR, 4)) == reasons["PREDICTOR"]
    # 32-bit integers, signed or not, and a 32-bit file that does not say what it holds
    for fmt in (1, 2):
        assert agree("int32", patched(f32, tiffio.SAMPLE_FORMAT, fmt)) == reasons["SAMPLE_FORMAT"]
    assert agree("no-format", patched(f32, tiffio.SAMPLE_FORMAT, 3).replace(struct.pack("<HHI", tiffio.SAMPLE_FORMAT, 3, 1), struct.pack("<HHI", 65000, 3, 1))) \
        == reasons["SAMPLE_FORMAT"]
    # floats that are not 32 bits wide
    tiffio.write_tiff(tmp_path / "h.tif", np.zeros((8, 8), np.uint16))
    assert agree("half", patched((tmp_path / "h.tif").read_bytes(), tiffio.SAMPLE_FORMAT, 3)) == reasons["SAMPLE_FORMAT"]
    assert agree("double", patched(f32, tiffio.BITS_PER_SAMPLE, 64)) == reasons["BITS"]
    info = api.tiff_info(patched(f32, tiffio.BITS_PER_SAMPLE, 64))
    assert info["dtype"] is None and info["shape"] is None and not info["supported"]
    with pytest.raises(NotImplementedError, match="not all 8, all 16 or all 32"):
        api.decode_tiff(patched(f32, tiffio.BITS_PER_SAMPLE, 64))
    # a thumbnail of a float file is refused in the words for every file that is not 8-bit, before the device is touched
    with pytest.raises(TypeError, match="thumbnail_tiff: 8-bit TIFF files in mode L or RGB"):
        api.thumbnail_tiff(f32, size=(4, 4))


def strip_cap(n):
    b = (12 * (n + n // 3836 + 2) + 7) // 8
    return b + (b & 1)


def derived_bound(h, w, c, rps=None, strip_bytes=65536):
    rowb = w * c * 4
    rps = min(rps or max(1, strip_bytes // rowb), h)
    nstrips = -(-h // rps)
    last = (h - (nstrips - 1) * rps) * rowb
    return 8 + (nstrips - 1) * strip_cap(rps * rowb) + strip_cap(last) + 2 + 12 * 13 + 4 + 4 * c + 8 * nstrips


def test_bound_equals_its_derivation():
    for h, w, c, rps in ((1, 1, 1, None), (33, 47, 1, None), (33, 47, 1, 4), (4096, 4096, 1, None), (2048, 1536, 1, None), (9, 129, 5, 1),
                         (300, 7, 3, 1000), (1, 1 << 24, 1, None)):
        assert lars.tiff_f32_bound(h, w, c, rps) == derived_bound(h, w, c, rps), (h, w, c, rps)
    assert lars.tiff_f32_bound(4096, 4096, 1) == lars.tiff_f32_bound(4096, 4096, 1, 4)            # 16 KiB rows, 64 KiB strips
    with _ffi.tuning(tiff_strip_bytes=8192):
        assert lars.tiff_f32_bound(64, 100, 1) == derived_bound(64, 100, 1, strip_bytes=8192)
    for h, w, c, rps in ((0, 4, 1, None), (4, 0, 1, None), (4, 4, 0, None), (4, 4, 6, None), ((1 << 24) + 1, 4, 1, None), (4, 4, 1, -1),
                         (8, 1 << 24, 5, 4)):                                                   # strips of more than 2^30 bytes
        assert lars.tiff_f32_bound(h, w, c, rps) == 0, (h, w, c, rps)
        assert _ffi.load().lars_tiff_f32_encode_scratch_bytes(h, w, c, rps or 0) == 0
    assert _ffi.load().lars_tiff_f32_encode_scratch_bytes(33, 47, 1, 4) > 0
    # the integer entry points did not learn a fourth item size
    assert lars.tiff_bound(4, 4, 1, 4) == 0 and _ffi.load().lars_tiff_encode_scratch_bytes(4, 4, 1, 4, 0) == 0


def test_argument_errors_need_no_device():
    ok = np.zeros((4, 4, 3), np.float32)
    for bad in (ok.astype(np.float64), ok.astype(np.float16), ok.astype(np.uint8), ok.astype(np.uint32), ok.astype(np.int32)):
        with pytest.raises(TypeError, match="float32"):
            lars.encode_tiff_f32(bad)
    for bad in (np.zeros(5, np.float32), np.zeros((2, 2, 2, 2), np.float32), np.float32(3)):
        with pytest.raises(ValueError, match=r"\[H, W\] or \[H, W, C\]"):
            lars.encode_tiff_f32(bad)
    for bad in (np.zeros((0, 4), np.float32), np.zeros((4, 0, 3), np.float32)):
        with pytest.raises(ValueError, match="empty"):
            lars.encode_tiff_f32(bad)
    with pytest.raises(ValueError, match="1 to 5 samples"):
        lars.encode_tiff_f32(np.zeros((4, 4, 6), np.float32))
    with pytest.raises(ValueError, match="rows_per_strip must be positive"):
        lars.encode_tiff_f32(ok, rows_per_strip=0)
    with pytest.raises(TypeError, match="rows_per_strip must be an int"):
        lars.encode_tiff_f32(ok, rows_per_strip=2.0)
    with pytest.raises(TypeError, match="uint8 or uint16"):
        lars.encode_tiff(ok)                                            # the integer encoder goes on refusing floats
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(ValueError, match="want_tiff must be False, True or 'predictor'"):
        lars.process_image(img, want_tiff="lzw")
    with pytest.raises(ValueError, match="want_tiff or want_png"):
        lars.process_image(img, want_tiff=True, want_png=True)


def test_header_binding_and_exports_agree_on_the_new_names():
    declared, exported = header_symbols(), exported_symbols(_ffi.LIB_PATH)
    for name in F32_NAMES:
        assert name in declared and name in exported and name in _ffi.SIGNATURES and hasattr(_ffi.load(), name), name
    assert [n for n in declared if "f32" in n and "tiff" in n] == sorted(F32_NAMES)
    assert "encode_tiff_f32" in api.__all__ and lars.encode_tiff_f32 is api.encode_tiff_f32 and lars.tiff_f32_bound is api.tiff_f32_bound
    assert lars.write_float_tiff is tiffio.write_float_tiff


def test_parser_under_the_sanitizers_on_float_files(asan_bin, tmp_path, combos):  # noqa: F811
    """The tiff-info mode of the stand-alone sanitizer driver on float files, truncations of them and the refused variants: no
    report, and the shipped library's answers."""
    rng = np.random.default_rng(2)
    f32 = written(fm.values("smooth", (8, 8), 0), predictor=3)
    blobs = [blob for _n, _a, blob, _kw in combos[::9]]
    blobs += [patched(f32, tiffio.PREDICTOR, 4), patched(f32, tiffio.SAMPLE_FORMAT, 1), patched(f32, tiffio.BITS_PER_SAMPLE, 64)]
    cases = []
    for blob in blobs:
        cases.append((6, 64, blob))
        for cut in sorted({8, len(blob) - 1, len(blob) // 2, *rng.integers(0, len(blob), 4).tolist()}):
            cases.append((6, 64, blob[:cut]))
        bad = bytearray(blob)
        ifd = struct.unpack_from("<I" if blob[:2] == b"II" else ">I", blob, 4)[0]
        bad[int(rng.integers(min(ifd, len(bad) - 1), len(bad)))] = int(rng.integers(0, 256))
        cases.append((6, 3, bytes(bad)))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for kind, a, data in cases:
            fh.write(struct.pack("<4I", kind, a, 0, len(data)) + data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([asan_bin, str(path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == f"done {len(cases)} cases"
    lib = _ffi.load()
    accepted = 0
    for i, ((_kind, a, data), line) in enumerate(zip(cases, lines)):
        words = dict(w.split("=") for w in line.split()[2:])
        arr = np.frombuffer(data or b"\0", dtype=np.uint8)
        info = _ffi.TiffInfo.array()
        table = np.zeros(a * 2 + 1, dtype=np.int64)
        rc = lib.lars_tiff_info(_ffi.ptr(arr), len(data), info, _ffi.ptr(table), a)
        assert int(words["rc"]) == rc, (i, line)
        if rc == 0:
            assert int(words["h"], 16) == fnv(bytes(info)) and int(words["t"], 16) == fnv(table[:a * 2].tobytes()), (i, line)
            accepted += info[14] == 1 and info[3] == 32
    assert accepted >= len(blobs) // 2
