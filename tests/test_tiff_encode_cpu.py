"""encode_tiff without a device: the NumPy model of the kernels (tests/tiff_encode_model.py) against the specification of the
stream, lzw_writer.encode(data, clear_at=4094) -- the greedy encoder whose strips libtiff writes byte for byte --, the model's
file against tiffio.read_tiff and tiffio.write_tiff's directory, lars.tiff_bound against the model's file on incompressible
input, and the argument errors, which are raised before anything is launched."""
import os
import struct
import tempfile

import numpy as np
import pytest

import lars_image_processing_amd as lars
from lars_image_processing_amd import tiffio

import lzw_writer as lz
import tiff_encode_model as model


def strip_of(data):
    """(geometry, byte view) of ``data`` as one strip: a one-row uint8 picture."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    return model.Geometry(1, a.size, 1, 1, rows_per_strip=1), a


def model_codes(data, events=None):
    g, a = strip_of(data)
    codes, stream, over = model.encode_strip(a, None, g, 0, events)
    assert not over and stream == lz.pack(codes)
    return codes


def spec(data):
    return lz.encode(bytes(data), clear_at=4094)


def data_codes_in_last_segment(codes):
    """Codes after the last Clear, EOI not counted."""
    last = len(codes) - 1 - codes[::-1].index(lz.CLEAR)
    return len(codes) - last - 2


def length_with(data, want, key):
    """The smallest prefix length of ``data`` for which key(codes) >= want (key grows with the length)."""
    lo, hi = 1, len(data)
    assert key(spec(data[:hi])) >= want
    while lo < hi:
        mid = (lo + hi) // 2
        if key(spec(data[:mid])) >= want:
            hi = mid
        else:
            lo = mid + 1
    return lo


RNG = np.random.default_rng(20261018)
RANDOM = RNG.integers(0, 256, 20000, dtype=np.uint8).tobytes()


def test_random_bytes_all_widths_and_clears():
    ev = model.new_events()
    codes = model_codes(RANDOM, ev)
    assert codes == spec(RANDOM)
    assert ev["widths"] == {9, 10, 11, 12} and ev["clears"] == 5 == codes.count(lz.CLEAR) - 1      # 6 Clears with the leading one
    assert ev["max_taken"] == model.SEG_CODES and ev["wrapped"]
    assert lz.plaintext(codes) == RANDOM


CASES = [
    ("zeros", bytes(20000)),
    ("kwkwk", b"".join(bytes([b]) * n for b, n in ((7, 1), (7, 2), (9, 300), (7, 5), (200, 1000), (9, 299), (0, 64), (255, 65)))),
    ("abab", b"ab" * 3000),
    ("ramp", bytes(i % 251 for i in range(20000))),
    ("one byte", b"\x80"),
    ("two equal", b"\x00\x00"),
    ("64", bytes(range(64))),
    ("65", bytes(range(65))),
]


@pytest.mark.parametrize("name, data", CASES, ids=[c[0] for c in CASES])
def test_model_codes_equal_the_greedy_encoder(name, data):
    codes = model_codes(data)
    assert codes == spec(data), name
    assert lz.plaintext(codes) == data


@pytest.mark.parametrize("index", [253, 254, 765, 766, 1789, 1790])
def test_lengths_that_end_at_a_width_change(index):
    """The last data code of the stream has this index in its segment (EOI the next): either side of 9 -> 10, 10 -> 11, 11 -> 12 bits."""
    n = length_with(RANDOM[:5000], index + 1, lambda c: len(c) - 2)
    data = RANDOM[:n]
    want = spec(data)
    assert want.count(lz.CLEAR) == 1 and len(want) - 2 == index + 1
    codes = model_codes(data)
    assert codes == want
    g, a = strip_of(data)
    assert model.encode_strip(a, None, g, 0)[1] == lz.pack(want)


def test_lengths_round_the_table_full_clear():
    """The shortest input whose stream holds a table-full Clear: its last code is the 3836th of the segment, no entry follows it,
    and libtiff clears the table all the same (the Clear, EOI at 9 bits).  One byte less (no Clear), one more (the Clear, one
    literal, EOI), two and three more."""
    n = length_with(RANDOM[:8000], 2, lambda c: c.count(lz.CLEAR))
    for m in (n - 1, n, n + 1, n + 2, n + 3):
        data = RANDOM[:m]
        want = spec(data)
        assert want.count(lz.CLEAR) == (1 if m < n else 2)
        ev = model.new_events()
        assert model_codes(data, ev) == want and ev["final_clear"] == (m == n) and ev["clears"] == (m >= n)
        assert lz.plaintext(want) == data
    at = spec(RANDOM[:n])
    assert at[-2] == lz.CLEAR and at[-3] != lz.CLEAR and len(at) == 1 + model.SEG_CODES + 2
    assert lz.bit_length(at) == lz.bit_length(at[:-2]) + 12 + 9           # the Clear has 12 bits, EOI behind it 9
    after = spec(RANDOM[:n + 1])
    assert after[-3] == lz.CLEAR and after[-2] < 256 and len(after) == 1 + model.SEG_CODES + 3 and after[:-2] == at[:-1]
    assert data_codes_in_last_segment(spec(RANDOM[:n - 1])) < model.SEG_CODES


def directory(blob):
    """{tag: (type, values)} of a little-endian classic TIFF, and the directory's offset."""
    assert blob[:4] == b"II*\0"
    (ifd,) = struct.unpack_from("<I", blob, 4)
    (count,) = struct.unpack_from("<H", blob, ifd)
    tags = {}
    for i in range(count):
        tag, typ, n = struct.unpack_from("<HHI", blob, ifd + 2 + 12 * i)
        size = {3: 2, 4: 4}[typ]
        where = ifd + 10 + 12 * i if size * n <= 4 else struct.unpack_from("<I", blob, ifd + 10 + 12 * i)[0]
        tags[tag] = (typ, struct.unpack_from("<%d%s" % (n, "H" if typ == 3 else "I"), blob, where))
    assert struct.unpack_from("<I", blob, ifd + 2 + 12 * count)[0] == 0
    return tags, ifd


def written(a, rows_per_strip, predictor):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "w.tif")
        tiffio.write_tiff(p, a, rows_per_strip=rows_per_strip, predictor=predictor)
        with open(p, "rb") as f:
            return f.read()


@pytest.mark.parametrize("shape, dtype, rps, predictor", [
    ((5, 7), np.uint8, None, False), ((5, 7, 2), np.uint8, 2, True), ((6, 9, 3), np.uint16, 4, True), ((3, 5, 4), np.uint16, 1, False),
    ((4, 3, 5), np.uint8, 3, True), ((1, 1), np.uint16, None, True), ((9, 11, 3), np.uint8, 1, False),
])
def test_model_file_reads_back_and_has_write_tiff_directory(shape, dtype, rps, predictor):
    a = RNG.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    status, blob, size = model.encode_file(a, rps, predictor)
    assert status == 0 and len(blob) == size
    back = tiffio.read_tiff(blob)
    assert back.dtype == a.dtype and back.shape == a.shape and np.array_equal(back, a)
    tags, ifd = directory(blob)
    want, _ = directory(written(a, rps or shape[0], predictor))
    assert list(tags) == list(want) == sorted(want)
    for tag in want:
        if tag not in (tiffio.COMPRESSION, tiffio.STRIP_OFFSETS, tiffio.STRIP_BYTE_COUNTS):
            assert tags[tag] == want[tag], tag
    assert tags[tiffio.COMPRESSION] == (3, (5,))
    offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
    assert len(offsets) == len(counts) == len(want[tiffio.STRIP_OFFSETS][1])
    at = 8
    a3 = a.reshape(a.shape[0], a.shape[1], -1)
    rows = tags[tiffio.ROWS_PER_STRIP][1][0]
    for k, (o, n) in enumerate(zip(offsets, counts)):
        assert o == at and o % 2 == 0
        at += n + (n & 1)
        part = a3[k * rows:(k + 1) * rows]
        if predictor:
            part = np.concatenate([part[:, :1], np.diff(part, axis=1)], axis=1)
        raw = np.ascontiguousarray(part).astype(a.dtype.newbyteorder("<")).tobytes()
        assert blob[o:o + n] == lz.pack(spec(raw)), k
    assert at == ifd


def test_model_refuses_a_buffer_one_byte_short():
    a = RNG.integers(0, 256, (6, 10, 3), dtype=np.uint8)
    status, blob, size = model.encode_file(a, 2, False)
    assert model.encode_file(a, 2, False, out_cap=size - 1) == (1, None, size)
    assert model.encode_file(a, 2, False, out_cap=size)[1] == blob


@pytest.mark.parametrize("shape, dtype, rps", [((1, 20000), np.uint8, None), ((40, 301, 3), np.uint8, 7), ((23, 129, 5), np.uint16, 1),
                                               ((37, 53), np.uint16, None), ((1, 1), np.uint8, None)])
def test_bound_covers_incompressible_input(shape, dtype, rps):
    a = RNG.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    h, w = shape[:2]
    c = shape[2] if len(shape) == 3 else 1
    bound = lars.tiff_bound(h, w, c, a.dtype.itemsize, rps)
    g = model.Geometry(h, w, c, a.dtype.itemsize, rps)
    assert bound == model.bound(g)
    status, blob, size = model.encode_file(a, rps, False)
    assert status == 0 and bound >= size > a.nbytes
    # the per-strip share of the bound holds for every strip, and no tighter whole number of 12-bit codes would
    n = g.strip_bytes(0)
    assert model.strip_cap(n) >= max(len(model.encode_strip(a.reshape(-1).view(np.uint8), None, g, k)[1]) for k in range(min(g.nstrips, 3)))


def test_bound_follows_the_strip_knob():
    from lars_image_processing_amd import _ffi
    assert _ffi.get_tuning("tiff_strip_bytes") == 65536
    assert lars.tiff_bound(1536, 2048, 3, 1) == lars.tiff_bound(1536, 2048, 3, 1, 10)           # 154 strips of 10 rows
    with _ffi.tuning(tiff_strip_bytes=8192):
        assert lars.tiff_bound(1536, 2048, 3, 1) == lars.tiff_bound(1536, 2048, 3, 1, 1)
    for bad in (0, -1, (1 << 30) + 1):
        with pytest.raises(_ffi.LarsError, match=r"tiff_strip_bytes is 1 \.\. 1073741824"):
            _ffi.set_tuning(tiff_strip_bytes=bad)
    assert _ffi.get_tuning("tiff_strip_bytes") == 65536
    assert lars.tiff_bound(0, 4, 1, 1) == 0 and lars.tiff_bound(4, 4, 6, 1) == 0 and lars.tiff_bound(4, 4, 1, 4) == 0


def test_argument_errors_need_no_device():
    ok = np.zeros((4, 4, 3), np.uint8)
    for bad in (ok.astype(np.float32), ok.astype(np.int16), ok.astype(np.uint32), ok.astype(bool)):
        with pytest.raises(TypeError, match="uint8 or uint16"):
            lars.encode_tiff(bad)
    for bad in (np.zeros(5, np.uint8), np.zeros((2, 2, 2, 2), np.uint8), np.uint8(3)):
        with pytest.raises(ValueError, match=r"\[H, W\] or \[H, W, C\]"):
            lars.encode_tiff(bad)
    for bad in (np.zeros((0, 4), np.uint8), np.zeros((4, 0, 3), np.uint16), np.zeros((4, 4, 0), np.uint8)):
        with pytest.raises(ValueError, match="empty"):
            lars.encode_tiff(bad)
    with pytest.raises(ValueError, match="1 to 5 samples"):
        lars.encode_tiff(np.zeros((4, 4, 6), np.uint8))
    with pytest.raises(ValueError, match="rows_per_strip must be positive"):
        lars.encode_tiff(ok, rows_per_strip=0)
    with pytest.raises(TypeError, match="rows_per_strip must be an int"):
        lars.encode_tiff(ok, rows_per_strip=2.5)
