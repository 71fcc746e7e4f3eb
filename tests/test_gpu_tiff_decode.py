"""decode_tiff / thumbnail_tiff / tiff_decoder="device" on the GPU against tiffio.read_tiff (every file) and Pillow (where it
reads the file the same way).  Every comparison is of bytes, dtype and shape."""
import io
import threading

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
import tiff_cases as tc
import tiff_lzw_model as model
from lars_image_processing_amd import api, tiffio
from test_tiffio import lzw_encode

pytestmark = pytest.mark.gpu


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


def check(blob, pillow=False):
    want = tiffio.read_tiff(blob)
    got = lars.decode_tiff(blob)
    same(got, want)
    if pillow:
        same(got, np.asarray(Image.open(io.BytesIO(blob))))
    return got


def pil_lzw(a, predictor=False):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="TIFF", compression="tiff_lzw", **({"tiffinfo": {317: 2}} if predictor else {}))
    return buf.getvalue()


def one_over_f(rng, h, w, c):
    f = np.fft.fft2(rng.normal(size=(c, h, w)))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    f /= np.maximum(np.hypot(fy, fx), 1.0 / max(h, w))
    x = np.real(np.fft.ifft2(f))
    x = (x - x.min()) / (x.max() - x.min())
    return np.moveaxis((x * 255).astype(np.uint8), 0, -1)


def sample(dtype, h, w, c, seed):
    rng = np.random.default_rng(seed)
    smooth = (np.add.outer(np.arange(h), np.arange(w))[..., None] * np.array([257, 1031, 4099, 17, 65521][:c])) % (np.iinfo(dtype).max + 1)
    noise = rng.integers(0, np.iinfo(dtype).max + 1, (h, w, c))
    a = np.where((np.arange(w) % 11 < 4)[None, :, None], noise, smooth).astype(dtype)
    return a[..., 0] if c == 1 else a


@pytest.mark.parametrize("predictor", [False, True])
def test_pillow_written_lzw_files(predictor):
    rng = np.random.default_rng(3)
    grad = np.stack([np.add.outer(np.arange(200), np.arange(300)) % 256, np.add.outer(np.arange(200), 2 * np.arange(300)) % 256,
                     np.add.outer(3 * np.arange(200), np.arange(300)) % 256], axis=2).astype(np.uint8)
    pics = [np.full((1, 1), 9, np.uint8), rng.integers(0, 256, (300, 1), dtype=np.uint8), rng.integers(0, 256, (1, 300, 3), dtype=np.uint8),
            rng.integers(0, 256, (61, 97), dtype=np.uint8), rng.integers(0, 200, (61, 97, 3), dtype=np.uint8), grad,
            rng.integers(0, 256, (384, 512, 3), dtype=np.uint8), np.full((384, 512, 3), 77, np.uint8), np.full((384, 512), 0, np.uint8),
            one_over_f(rng, 240, 320, 3)]
    for a in pics:
        same(check(pil_lzw(a, predictor), pillow=True), a)
    g16 = (rng.integers(0, 65536, (500, 700)) & 0xFFC0).astype(np.uint16)
    g16[:, 100:400] = (np.add.outer(np.arange(500), np.arange(300)) * 37 % 65536).astype(np.uint16)
    same(check(pil_lzw(g16, predictor), pillow=True), g16)
    info = lars.tiff_info(pil_lzw(pics[6]))
    assert info["chunks"] >= 9 and info["compression"] == 5 and info["supported"] and info["shape"] == (384, 512, 3)


LAYOUTS = [{"rows_per_strip": 1}, {"rows_per_strip": 7}, {}, {"tile": (16, 16)}, {"tile": (32, 48)}]


@pytest.mark.parametrize("lzw", [True, False])
@pytest.mark.parametrize("dtype,byteorder", [(np.uint8, "<"), (np.uint8, ">"), (np.uint16, "<"), (np.uint16, ">")])
def test_every_layout(dtype, byteorder, lzw):
    """write_tiff's layouts, compressed with the test encoder (as test_sixteen_bit_rgb_lzw_tiff does) or left uncompressed (the
    assembly kernel alone): planar 1 / 2, 1 to 5 samples, predictor off / on, strips of 1, 7 and all rows, tiles of 16 x 16
    and 32 x 48, on a width and height that are multiples of none of them."""
    seed = 0
    for planar in (1, 2):
        for c in (1, 2, 3, 4, 5):
            for predictor in (False, True):
                for layout in LAYOUTS:
                    seed += 1
                    a = sample(dtype, 37, 53, c, seed)
                    kw = dict(layout, byteorder=byteorder, planar=planar, predictor=predictor)
                    blob = tc.lzw_tiff(a, **kw) if lzw else tc.written(a, **kw)
                    same(check(blob), a)


def test_largest_case_and_pillow_readable_layouts():
    a = sample(np.uint16, 263, 257, 3, 5)
    same(check(tc.lzw_tiff(a, rows_per_strip=50, predictor=True)), a)
    same(check(tc.lzw_tiff(a, tile=(64, 80), predictor=True, byteorder=">", planar=2)), a)
    rgb = sample(np.uint8, 61, 97, 3, 6)
    same(check(tc.written(rgb, rows_per_strip=9), pillow=True), rgb)
    same(check(tc.written(rgb, tile=(16, 32)), pillow=True), rgb)
    g16 = sample(np.uint16, 61, 97, 1, 7)
    same(check(tc.written(g16, rows_per_strip=9), pillow=True), g16)


def test_many_chunks_odd_counts_and_a_stream_without_eoi():
    rng = np.random.default_rng(9)
    a = rng.integers(0, 9, (300, 41, 3), dtype=np.uint8)
    blob = tc.lzw_tiff(a, rows_per_strip=1)                                   # 300 chunks
    assert lars.tiff_info(blob)["chunks"] == 300
    same(check(blob), a)
    row = np.arange(123, dtype=np.uint8)[None, :] % 5                       # one chunk of an odd size, streams of odd and even length
    for pad in (b"", b"\0"):
        stream = lzw_encode(row.tobytes()) + pad
        same(check(tc.one_strip_tiff(stream, 123)), row)
    codes = tc.unpack(lzw_encode(row.tobytes()))
    assert codes[-1] == model.EOI
    same(check(tc.one_strip_tiff(tc.pack(codes[:-1]), 123)), row)             # ends without EOI exactly at the chunk's size
    with pytest.raises(tiffio.TiffError, match="bytes, 123 expected"):
        lars.decode_tiff(tc.one_strip_tiff(tc.pack(codes[:-3]), 123))
    same(check(blob), a)


def test_damaged_streams_raise_where_read_tiff_does():
    """20 streams of the CPU corpus that model and host decoder call corrupt and 20 mutated ones they decode, each as the only
    strip of a file.  Every one has passed the model's range assertions (here again, before it is decoded)."""
    good = pil_lzw(np.arange(600, dtype=np.uint8).reshape(20, 30))
    mutated = [(k, s, n) for k, s, n in tc.corpus() if k != "valid" and not (len(s) >= 2 and s[0] == 0 and s[1] & 1)]
    judged = [(s, n, model.decode(s, n)) for _k, s, n in mutated[::7]]
    corrupt = [(s, n) for s, n, (_b, bad) in judged if bad][:20]
    valid = [(s, n) for s, n, (b, bad) in judged if not bad and len(b) == n][:20]
    short = [(s, n) for s, n, (b, bad) in judged if not bad and len(b) < n][:5]
    assert len(corrupt) == 20 and len(valid) == 20 and len(short) == 5
    raised = 0
    for stream, n in corrupt + valid + short:
        blob = tc.one_strip_tiff(stream, n)
        try:
            want = tiffio.read_tiff(blob)
        except tiffio.TiffError as e:
            with pytest.raises(tiffio.TiffError) as got:
                lars.decode_tiff(blob)
            if "expected" in str(e):
                assert str(e) in str(got.value)                              # "strip / tile holds N bytes, M expected"
            raised += 1
            same(lars.decode_tiff(good), tiffio.read_tiff(good))             # the status was reset, the workspace is intact
        else:
            same(lars.decode_tiff(blob), want)
    assert raised == 25


def test_unsupported_files_raise_before_anything_is_launched():
    rgb = sample(np.uint8, 20, 30, 3, 1)
    with pytest.raises(NotImplementedError, match="Deflate"):
        lars.decode_tiff(tc.written(rgb, deflate=True))
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="TIFF", compression="packbits")
    with pytest.raises(NotImplementedError, match="PackBits"):
        lars.decode_tiff(buf.getvalue())
    with pytest.raises(NotImplementedError, match="BigTIFF"):
        lars.decode_tiff(b"II" + bytes([43, 0, 8, 0, 0, 0]) + bytes(40))
    with pytest.raises(tiffio.TiffError):
        lars.decode_tiff(b"II*\0" + bytes(20))
    with pytest.raises(TypeError):
        lars.decode_tiff("a.tif")


@pytest.mark.parametrize("mode", ["L", "RGB"])
def test_thumbnail_equals_pillow(mode):
    rng = np.random.default_rng(12)
    a = one_over_f(rng, 480, 640, 3 if mode == "RGB" else 1)
    a = a if mode == "RGB" else a[..., 0]
    for blob in (pil_lzw(a), pil_lzw(a, True), tc.written(a, tile=(64, 64))):
        for size in ((100, 100), (400, 400), (640, 480), (1000, 1000)):
            im = Image.open(io.BytesIO(blob))
            im.thumbnail(size, Image.LANCZOS, reducing_gap=2.0)
            same(lars.thumbnail_tiff(blob, size), np.asarray(im))
    with pytest.raises(TypeError):
        lars.thumbnail_tiff(tc.written(sample(np.uint16, 40, 50, 3, 1)))
    with pytest.raises(TypeError):
        lars.thumbnail_tiff(tc.written(sample(np.uint8, 40, 50, 4, 1)))


def test_read_image_routing(tmp_path):
    rgb = one_over_f(np.random.default_rng(2), 90, 120, 3)
    (tmp_path / "rgb.tif").write_bytes(pil_lzw(rgb))
    a16 = sample(np.uint16, 45, 67, 3, 3)
    (tmp_path / "a16.tiff").write_bytes(tc.lzw_tiff(a16, rows_per_strip=8, predictor=True))
    (tmp_path / "z.tif").write_bytes(tc.written(a16, deflate=True))
    Image.fromarray(rgb).save(tmp_path / "png.tif", format="PNG")
    calls = []
    real = api.decode_tiff
    api.decode_tiff = lambda data: (calls.append(1), real(data))[1]
    try:
        for name, full in (("rgb.tif", False), ("a16.tiff", True), ("z.tif", True), ("png.tif", False)):
            same(tiffio.read_image(tmp_path / name, full_depth=full, tiff_decoder="device"), tiffio.read_image(tmp_path / name, full_depth=full))
        assert len(calls) == 2                                               # the 8-bit RGB file, and the 16-bit one at full depth
    finally:
        api.decode_tiff = real
    same(tiffio.read_image(tmp_path / "a16.tiff", full_depth=True, tiff_decoder="device"), a16)
    with pytest.raises(ValueError, match="tiff_decoder"):
        tiffio.read_image(tmp_path / "rgb.tif", tiff_decoder="gpu")


def test_threads_decode_at_once():
    rng = np.random.default_rng(31)
    files = [pil_lzw(one_over_f(rng, 150 + 13 * k, 260 - 7 * k, 3), k % 2 == 1) for k in range(6)]
    files += [tc.written(sample(np.uint16, 90, 70, 3, k), tile=(16, 32), predictor=True) for k in range(2)]
    out = [None] * 8

    def run(k):
        for _ in range(3):
            out[k] = lars.decode_tiff(files[k])

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(8):
        same(out[k], tiffio.read_tiff(files[k]))
