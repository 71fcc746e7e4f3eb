"""decode_tiff / thumbnail_tiff with deflate=True on the GPU against tiffio.read_tiff (zlib, every file) and Pillow (where it
reads the file the same way).  Every comparison is of bytes, dtype and shape; every refusal is compared by kind with
read_tiff's.  The streams are those test_tiff_deflate_cpu.py has already held against zlib and the model on the CPU."""
import io
import threading
import zlib

import numpy as np
import pytest
from PIL import Image

import deflate_writer as dw
import lars_image_processing_amd as lars
import test_tiff_deflate_cpu as cpu
import tiff_cases as tc
from lars_image_processing_amd import _ffi, tiffio
from test_gpu_tiff_decode import one_over_f, pil_lzw, same, sample

pytestmark = pytest.mark.gpu


def check(blob, pillow=False):
    want = tiffio.read_tiff(blob)
    got = lars.decode_tiff(blob, deflate=True)
    same(got, want)
    if pillow:
        same(got, np.asarray(Image.open(io.BytesIO(blob))))
    return got


def pil_deflate(a, predictor=False):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="TIFF", compression="tiff_adobe_deflate", **({"tiffinfo": {317: 2}} if predictor else {}))
    return buf.getvalue()


def kind_of(text):
    if "corrupt Deflate data" in text:
        return "corrupt"
    if "inflates past" in text:
        return "past"
    assert "expected" in text, text
    return "short"


def outcome(blob):
    """("bytes", array) or (kind, message) of read_tiff, and the same of the device; asserts that they agree."""
    try:
        want = tiffio.read_tiff(blob)
    except tiffio.TiffError as e:
        with pytest.raises(tiffio.TiffError) as got:
            lars.decode_tiff(blob, deflate=True)
        kind = kind_of(str(e))
        assert kind_of(str(got.value)) == kind, (str(e), str(got.value))
        if kind == "short":
            assert str(e) in str(got.value)                                  # "strip / tile holds N bytes, M expected"
        if kind == "past":
            assert str(e).split("inflates")[1] in str(got.value)             # "past its N bytes"
        return kind
    same(lars.decode_tiff(blob, deflate=True), want)
    return "bytes"


LAYOUTS = [{}, {"rows_per_strip": 7}, {"tile": (16, 16)}, {"tile": (32, 48)}]


@pytest.mark.parametrize("dtype,byteorder", [(np.uint8, "<"), (np.uint8, ">"), (np.uint16, "<"), (np.uint16, ">")])
def test_every_layout(dtype, byteorder):
    seed = 0
    for planar in (1, 2):
        for predictor in (False, True):
            for layout in LAYOUTS:
                seed += 1
                a = sample(dtype, 37, 53, 3, seed)
                same(check(tc.written(a, deflate=True, byteorder=byteorder, planar=planar, predictor=predictor, **layout)), a)
    for c in (1, 2, 3, 4, 5):
        for planar in (1, 2):
            a = sample(dtype, 9, 11, c, 40 + c)
            same(check(tc.written(a, deflate=True, byteorder=byteorder, planar=planar, predictor=True, rows_per_strip=4)), a)
    for shape in ((1, 1), (1, 300), (300, 1)):
        a = sample(dtype, shape[0], shape[1], 1, 50)
        same(check(tc.written(a, deflate=True, byteorder=byteorder)), a)


def test_pillow_written_files_and_the_old_tag():
    rng = np.random.default_rng(3)
    rgb = one_over_f(rng, 480, 640, 3)
    for predictor in (False, True):
        blob = pil_deflate(rgb, predictor)
        info = lars.tiff_info(blob, deflate=True)
        assert info["compression"] == 8 and info["chunks"] >= 5 and info["supported"] and info["predictor"] == (2 if predictor else 1)
        same(check(blob, pillow=True), rgb)
    for a in (np.full((1, 1), 9, np.uint8), rng.integers(0, 256, (61, 97), dtype=np.uint8), np.full((384, 512, 3), 77, np.uint8)):
        same(check(pil_deflate(a), pillow=True), a)
    old = cpu.with_compression(tc.written(sample(np.uint16, 37, 53, 3, 1), deflate=True, rows_per_strip=7), 32946)
    assert lars.tiff_info(old, deflate=True)["compression"] == 32946
    same(check(old), sample(np.uint16, 37, 53, 3, 1))


def test_hand_built_streams_as_read_tiff_reads_them():
    good = pil_deflate(np.arange(600, dtype=np.uint8).reshape(20, 30))
    kinds = {}
    for name, stream, want in cpu.corpus():
        kind = outcome(cpu.deflate_strip_tiff(stream, want))
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind != "bytes":
            same(lars.decode_tiff(good, deflate=True), tiffio.read_tiff(good))   # the status was reset, the workspace is intact
    assert min(kinds.get(k, 0) for k in ("bytes", "corrupt", "past", "short")) >= 10, kinds


def test_far_matches_and_a_match_that_ends_the_strip():
    rng = np.random.default_rng(17)
    window = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    syms = [("copy", 258, 32768)] * 28 + [("copy", 8, 32768)]
    plain = window + dw.plaintext(syms, window)
    assert len(plain) == 40000
    sink = dw.BitSink()
    dw.stored_block(sink, window)
    dw.fixed_block(sink, syms, final=True)
    stream = dw.zlib_stream(sink.getvalue(), plain)
    got = check(cpu.deflate_strip_tiff(stream, 40000))
    assert got.tobytes() == plain
    with pytest.raises(tiffio.TiffError, match="inflates past its 39999 bytes"):
        lars.decode_tiff(cpu.deflate_strip_tiff(stream, 39999), deflate=True)
    assert outcome(cpu.deflate_strip_tiff(stream, 39999)) == "past"
    assert outcome(cpu.deflate_strip_tiff(stream, 40001)) == "short"


def test_mutated_streams_as_read_tiff_reads_them():
    """The first 300 cases of the CPU fuzz: bounded streams inside a well-formed file, each already accepted or refused by zlib
    and the model on the CPU."""
    kinds = {}
    for _kind, stream, want in cpu.fuzz()[:300]:
        kind = outcome(cpu.deflate_strip_tiff(stream, want))
        kinds[kind] = kinds.get(kind, 0) + 1
    assert kinds.get("bytes", 0) >= 75 and 300 - kinds.get("bytes", 0) >= 75, kinds


def test_the_first_bad_strip_is_reported():
    a = sample(np.uint8, 64, 50, 3, 2)
    blob = tc.written(a, deflate=True, rows_per_strip=8)
    tags = tiffio._read_ifd(memoryview(blob), "<")
    streams = [blob[o:o + c] for o, c in zip(tags[tiffio.STRIP_OFFSETS], tags[tiffio.STRIP_BYTE_COUNTS])]
    assert len(streams) == 8
    same(check(cpu.restreamed(blob, {})), a)
    flipped = lambda s: s[:-1] + bytes([s[-1] ^ 0x10])                          # noqa: E731  (a wrong Adler-32)
    corrupt2, corrupt5 = flipped(streams[2]), flipped(streams[5])
    for s in (corrupt2, corrupt5):
        assert cpu.chunk_outcome(s, 8 * 50 * 3) == ("corrupt",)
    for third, sixth, kind in ((corrupt2, corrupt5, "corrupt"), (streams[2][:20], corrupt5, "short"), (corrupt2, streams[5][:20], "corrupt"),
                               (zlib.compress(bytes(8 * 50 * 3 + 1)), corrupt5, "past")):
        bad = cpu.restreamed(blob, {2: third, 5: sixth})
        assert outcome(bad) == kind
        with pytest.raises(tiffio.TiffError) as e:
            lars.decode_tiff(bad, deflate=True)
        assert "chunk 2" in str(e.value) or kind == "short"
    same(check(blob), a)


@pytest.mark.parametrize("mode", ["L", "RGB"])
def test_thumbnail_equals_pillow(mode):
    rng = np.random.default_rng(12)
    a = one_over_f(rng, 480, 640, 3 if mode == "RGB" else 1)
    a = a if mode == "RGB" else a[..., 0]
    for blob in (pil_deflate(a), pil_deflate(a, True), tc.written(a, deflate=True, tile=(64, 64))):
        for size in ((100, 100), (400, 400), (640, 480), (1000, 1000)):
            im = Image.open(io.BytesIO(blob))
            im.thumbnail(size, Image.LANCZOS, reducing_gap=2.0)
            same(lars.thumbnail_tiff(blob, size, deflate=True), np.asarray(im))
    with pytest.raises(NotImplementedError, match="Deflate"):
        lars.thumbnail_tiff(pil_deflate(a), (100, 100))
    lzw = pil_lzw(a)
    same(lars.thumbnail_tiff(lzw, (100, 100), deflate=True), lars.thumbnail_tiff(lzw, (100, 100)))


def test_the_default_has_not_moved():
    rgb = sample(np.uint8, 20, 30, 3, 1)
    for blob in (tc.written(rgb, deflate=True), pil_deflate(rgb)):
        with pytest.raises(NotImplementedError, match="Deflate"):
            lars.decode_tiff(blob)
        with pytest.raises(NotImplementedError, match="Deflate"):
            lars.decode_tiff(blob, deflate=False)
        assert not lars.tiff_info(blob)["supported"]
        same(lars.decode_tiff(blob, deflate=True), rgb)
    for blob in (pil_lzw(rgb), tc.written(rgb, tile=(16, 16))):                 # other files: the flag changes nothing
        same(lars.decode_tiff(blob, deflate=True), lars.decode_tiff(blob))


def test_threads_decode_at_once():
    rng = np.random.default_rng(31)
    files = [pil_deflate(one_over_f(rng, 150 + 13 * k, 260 - 7 * k, 3), k % 2 == 1) for k in range(3)]
    files += [pil_lzw(one_over_f(rng, 150 + 13 * k, 260 - 7 * k, 3)) for k in range(2)]
    files += [tc.written(sample(np.uint16, 90, 70, 3, 4), deflate=True, tile=(16, 32), predictor=True)]
    out = [None] * 6

    def run(k):
        for _ in range(3):
            out[k] = lars.decode_tiff(files[k], deflate=True)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(6)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(6):
        same(out[k], tiffio.read_tiff(files[k]))


def test_nothing_outside_the_picture_is_written():
    guard = 4096
    for a, kw in ((sample(np.uint8, 37, 53, 3, 1), {"tile": (16, 16)}), (sample(np.uint16, 37, 53, 2, 2), {"rows_per_strip": 7, "predictor": True}),
                  (sample(np.uint8, 1, 1, 1, 3), {})):
        blob = np.frombuffer(tc.written(a, deflate=True, **kw), dtype=np.uint8)
        buf = np.full(a.nbytes + 2 * guard, 0xA5, dtype=np.uint8)
        inner = buf[guard:guard + a.nbytes]
        _ffi.call("lars_h_decode_tiff_deflate", _ffi.ptr(blob), blob.size, _ffi.ptr(inner), a.nbytes)
        assert inner.tobytes() == a.tobytes()
        assert (buf[:guard] == 0xA5).all() and (buf[guard + a.nbytes:] == 0xA5).all()
        with pytest.raises(_ffi.LarsError):
            _ffi.call("lars_h_decode_tiff_deflate", _ffi.ptr(blob), blob.size, _ffi.ptr(inner), a.nbytes - 1)
        assert (buf[:guard] == 0xA5).all() and (buf[guard + a.nbytes:] == 0xA5).all()
