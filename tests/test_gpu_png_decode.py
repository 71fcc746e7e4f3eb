"""decode_png / thumbnail_png / png_decoder="device" on the GPU: every array equals Pillow's, byte for byte."""
import io
import struct
import sys
import threading
import zlib
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import api, driver

sys.path.insert(0, str(Path(__file__).resolve().parent))
import deflate_writer  # noqa: E402
from test_png_cpu import SIG, filter_rows  # noqa: E402

pytestmark = pytest.mark.gpu

CHANNELS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "P": 1}


def pil_png(arr, mode, **save):
    if mode == "P":
        im = Image.fromarray(arr, "P")
        im.putpalette(bytes(range(256)) * 3)                  # 256 entries: an 8-bit palette file
    else:
        im = Image.fromarray(arr, mode)
    b = io.BytesIO()
    im.save(b, "PNG", **save)
    return b.getvalue()


def want(b):
    return np.asarray(Image.open(io.BytesIO(b)))


def same(b):
    got, ref = lars.decode_png(b), want(b)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    assert got.tobytes() == ref.tobytes()


def shape_of(mode, h, w):
    c = CHANNELS[mode]
    return (h, w) if c == 1 else (h, w, c)


def noise(rng, mode, h, w):
    return rng.integers(0, 256, shape_of(mode, h, w), dtype=np.uint8)


def gradient(mode, h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 3 + y * 5) & 255).astype(np.uint8)
    c = CHANNELS[mode]
    return base if c == 1 else np.stack([(base + 40 * k) & 255 for k in range(c)], axis=2).astype(np.uint8)


def field(rng, h, w, c, beta=2.0):
    """1/f noise field (as test_gpu_png.py's smooth pictures)."""
    fy = np.fft.fftfreq(h)[:, None]
    fx = np.fft.rfftfreq(w)[None, :]
    f = np.sqrt(fx * fx + fy * fy)
    f[0, 0] = 1.0
    out = []
    for _ in range(c):
        spec = (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)) / f ** (beta / 2)
        x = np.fft.irfft2(spec, s=(h, w))
        x = (x - x.min()) / max(x.max() - x.min(), 1e-12)
        out.append((x * 255).astype(np.uint8))
    return out[0] if c == 1 else np.stack(out, axis=2)


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


def build_png(w, h, ctype, stream, idat_sizes=None, before=()):
    """A PNG file around a given zlib stream: IDATs of the given sizes, ancillary chunks before / between them."""
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0))
    for t, d in before:
        out += chunk(t, d)
    sizes = idat_sizes or [len(stream)]
    pos, k = 0, 0
    while pos < len(stream):
        n = sizes[min(k, len(sizes) - 1)]
        out += chunk(b"IDAT", stream[pos:pos + n])
        pos += n
        k += 1
    return out + chunk(b"IEND", b"")


def raw_rows(img, filt=None):
    """The filtered stream of img ([h][w][c] or [h][w]) with one filter forced on every row (None: libpng's choice)."""
    a = img.reshape(img.shape[0], -1)
    bpp = 1 if img.ndim == 2 else img.shape[2]
    f, choice = filter_rows(a, bpp)
    rows = []
    for y in range(a.shape[0]):
        k = int(choice[y]) if filt is None else filt
        rows.append(bytes([k]) + f[k, y].tobytes())
    return b"".join(rows)


CTYPE = {"L": 0, "RGB": 2, "P": 3, "LA": 4, "RGBA": 6}


@pytest.mark.parametrize("mode", ["L", "LA", "RGB", "RGBA", "P"])
@pytest.mark.parametrize("h", [1, 2, 67])
def test_every_mode_and_small_shapes(mode, h):
    rng = np.random.default_rng(h * 7 + len(mode))
    for w in range(1, 68):
        img = noise(rng, mode, h, w) if w % 2 else gradient(mode, h, w)
        same(pil_png(img, mode))


@pytest.mark.parametrize("h,w", [(1, 5000), (5000, 1)])
def test_thin_shapes(h, w):
    rng = np.random.default_rng(5)
    for mode in ("L", "RGB", "RGBA"):
        same(pil_png(noise(rng, mode, h, w), mode))
        same(pil_png(gradient(mode, h, w), mode))


def test_4096_rgba():
    rng = np.random.default_rng(9)
    img = field(rng, 4096, 4096, 4)
    same(pil_png(img, "RGBA", compress_level=1))


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_compress_levels(level):
    rng = np.random.default_rng(level)
    for img, mode in ((noise(rng, "RGB", 96, 130), "RGB"), (gradient("RGBA", 120, 77), "RGBA"),
                      (field(rng, 200, 150, 3), "RGB"), (field(rng, 64, 300, 1), "L")):
        same(pil_png(img, mode, compress_level=level))


def test_optimize():
    rng = np.random.default_rng(2)
    same(pil_png(field(rng, 256, 320, 3), "RGB", optimize=True))
    same(pil_png(gradient("L", 100, 100), "L", optimize=True))


def test_flat_4096_rgb_long_copy_chains():
    img = np.empty((4096, 4096, 3), np.uint8)
    img[...] = (37, 201, 90)
    same(pil_png(img, "RGB"))


def test_smooth_fields():
    rng = np.random.default_rng(11)
    for beta in (1.0, 2.0, 3.0):
        same(pil_png(field(rng, 333, 517, 3, beta), "RGB"))
        same(pil_png(field(rng, 257, 129, 4, beta), "RGBA"))


def test_gallery_images():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    from thumbbench import gallery
    for img in gallery():
        arr = np.asarray(img) if not isinstance(img, np.ndarray) else img
        b = pil_png(arr, "RGB")
        same(b)


def test_files_made_by_encode_png():
    rng = np.random.default_rng(4)
    for h, w in ((1, 1), (3, 7), (64, 64), (129, 67), (300, 1000)):
        for c in (1, 3, 4):
            img = noise(rng, "L" if c == 1 else "RGB" if c == 3 else "RGBA", h, w) if (h + w) % 2 else field(rng, h, w, c)
            same(lars.encode_png(img))
        pal = rng.integers(0, 256, (256, 4), dtype=np.uint8)
        same(lars.encode_png(rng.integers(0, 256, (h, w), dtype=np.uint8), palette=pal))


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
def test_forced_filters(filt):
    rng = np.random.default_rng(filt)
    for mode in ("L", "RGB", "RGBA", "LA"):
        img = field(rng, 70, 90, CHANNELS[mode])
        b = build_png(90, 70, CTYPE[mode], zlib.compress(raw_rows(img, filt), 6))
        same(b)
        assert np.array_equal(lars.decode_png(b), img)


def test_idat_splits():
    rng = np.random.default_rng(3)
    img = field(rng, 40, 50, 3)
    stream = zlib.compress(raw_rows(img), 6)
    same(build_png(50, 40, 2, stream, idat_sizes=[1]))
    same(build_png(50, 40, 2, stream, idat_sizes=[len(stream)]))
    same(build_png(50, 40, 2, stream, idat_sizes=[7, 1, 300]))


def test_ancillary_chunks_before_and_between():
    rng = np.random.default_rng(6)
    img = field(rng, 40, 50, 3)
    stream = zlib.compress(raw_rows(img), 6)
    anc = [(b"tEXt", b"Comment\x00hello"), (b"gAMA", struct.pack(">I", 45455)), (b"pHYs", struct.pack(">IIB", 3780, 3780, 1))]
    b = build_png(50, 40, 2, stream, before=anc)
    same(b)
    # after the IDAT run, before IEND
    cut = b.rindex(b"IEND") - 4
    same(b[:cut] + chunk(b"tEXt", b"k\x00v") + b[cut:])


@pytest.mark.parametrize("h,w", [(64, 64), (512, 512)])
def test_fixed_huffman_stream(h, w):
    rng = np.random.default_rng(h)
    img = field(rng, h, w, 3)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    stream = co.compress(raw_rows(img)) + co.flush()
    same(build_png(w, h, 2, stream))


def test_mixed_block_types():
    rng = np.random.default_rng(8)
    img = field(rng, 120, 100, 3)
    raw = raw_rows(img)
    parts = [raw[i:i + 5000] for i in range(0, len(raw), 5000)]
    co = zlib.compressobj(6)
    stream = b""
    for k, p in enumerate(parts):
        stream += co.compress(p) + co.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH)
    stream += co.flush()
    # a stream that mixes stored, fixed and dynamic blocks: raw deflate pieces of different strategies
    pieces = []
    for k, p in enumerate(parts):
        strat = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY)[k % 3]
        lvl = 0 if k % 4 == 3 else 6
        c = zlib.compressobj(lvl, zlib.DEFLATED, -15, 8, strat)
        pieces.append(c.compress(p) + c.flush(zlib.Z_SYNC_FLUSH))
    body = b"".join(pieces) + b"\x03\x00"                     # empty fixed final block
    mixed = b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(raw))
    assert zlib.decompress(mixed) == raw
    same(build_png(100, 120, 2, stream))
    same(build_png(100, 120, 2, mixed))


def test_trailing_data_after_the_image():
    rng = np.random.default_rng(12)
    img = field(rng, 30, 40, 3)
    stream = zlib.compress(raw_rows(img) + b"\x00" * 500, 6)
    b = build_png(40, 30, 2, stream)
    same(b)


def fixed_block(symbols):
    """One final fixed-Huffman block of ("lit", byte) / ("copy", length, distance) symbols, byte-aligned at the end."""
    sink = deflate_writer.BitSink()
    deflate_writer.fixed_block(sink, symbols, final=True)
    return sink.getvalue()


def _image_and_stream():
    rng = np.random.default_rng(21)
    img = field(rng, 50, 60, 3)
    raw = raw_rows(img)
    return img, raw, zlib.compress(raw, 6)


def test_damage_raises_value_error():
    img, raw, stream = _image_and_stream()
    b = build_png(60, 50, 2, stream)
    idat = b.index(b"IDAT") + 4
    flipped = bytearray(b)
    flipped[idat + len(stream) // 2] ^= 0x20
    with pytest.raises(ValueError, match="CRC"):
        lars.decode_png(bytes(flipped))
    bad = bytearray(stream)
    bad[len(stream) // 2] ^= 0x20
    with pytest.raises(ValueError, match="deflate|Adler|decoded|filter"):
        lars.decode_png(build_png(60, 50, 2, bytes(bad)))
    wrong_adler = stream[:-4] + struct.pack(">I", zlib.adler32(raw) ^ 1)
    with pytest.raises(ValueError, match="Adler"):
        lars.decode_png(build_png(60, 50, 2, wrong_adler))
    short = zlib.compress(raw[:-(1 + 60 * 3)], 6)
    with pytest.raises(ValueError, match="too few decoded bytes"):
        lars.decode_png(build_png(60, 50, 2, short))
    bad_filter = bytearray(raw)
    bad_filter[(1 + 60 * 3) * 7] = 5
    with pytest.raises(ValueError, match="filter byte"):
        lars.decode_png(build_png(60, 50, 2, zlib.compress(bytes(bad_filter), 6)))
    # a fixed block whose first symbol is a copy (length 3, distance 1) from before the stream start
    far = b"\x78\x01" + fixed_block([("copy", 3, 1), ("lit", 0)] * 4) + b"\x00\x00\x00\x00"
    with pytest.raises(ValueError, match="too far back"):
        lars.decode_png(build_png(60, 50, 2, far))
    with pytest.raises(ValueError, match="zlib header"):
        lars.decode_png(build_png(60, 50, 2, b"\x78\x00" + stream[2:]))


@pytest.mark.parametrize("mode", ["L", "RGB", "RGBA"])
@pytest.mark.parametrize("shape", [(1536, 2048), (3000, 500), (300, 2500)])
@pytest.mark.parametrize("gap", [None, 1.0, 2.0, 3.0])
def test_thumbnail_png_matches_pillow(mode, shape, gap):
    rng = np.random.default_rng(shape[0] + len(mode))
    img = field(rng, shape[0], shape[1], CHANNELS[mode])
    b = pil_png(img, mode, compress_level=1)
    im = Image.open(io.BytesIO(b))
    im.thumbnail((400, 400), Image.Resampling.LANCZOS, gap)
    got = lars.thumbnail_png(b, (400, 400), gap)
    assert got.tobytes() == np.asarray(im).tobytes() and got.shape == np.asarray(im).shape
    assert np.array_equal(got, lars.thumbnail(lars.decode_png(b), (400, 400), gap))


def test_thumbnail_png_small_file_and_modes():
    img = gradient("RGB", 100, 120)
    b = pil_png(img, "RGB")
    assert np.array_equal(lars.thumbnail_png(b), img)
    with pytest.raises(TypeError):
        lars.thumbnail_png(pil_png(gradient("LA", 500, 500), "LA"))
    with pytest.raises(TypeError):
        lars.thumbnail_png(pil_png(gradient("P", 500, 500), "P"))


def test_threads_decode_at_once():
    rng = np.random.default_rng(31)
    files = [pil_png(field(rng, 200 + 13 * k, 300 - 7 * k, 3 if k % 2 else 4), "RGB" if k % 2 else "RGBA") for k in range(8)]
    out = [None] * 8

    def run(k):
        for _ in range(3):
            out[k] = lars.decode_png(files[k])

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(8):
        assert out[k].tobytes() == want(files[k]).tobytes()


def test_batch_process_with_the_device_decoder(tmp_path, monkeypatch):
    rng = np.random.default_rng(41)
    decoded, lock = [], threading.Lock()
    real_decode = api.decode_png

    def counting_decode(data):
        out = real_decode(data)
        with lock:
            decoded.append(out.shape)
        return out

    monkeypatch.setattr(api, "decode_png", counting_decode)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(field(rng, 96, 128, 3)).save(src / "a.png")
    Image.fromarray(field(rng, 80, 64, 4), "RGBA").save(src / "b.png")
    Image.fromarray(field(rng, 64, 64, 3)).save(src / "c.tif")
    Image.fromarray(field(rng, 64, 96, 3)).save(src / "d.jpg", quality=90)
    Image.fromarray(np.ascontiguousarray(field(rng, 40, 50, 3)[:, :, 0]).astype(np.uint16) * 257).save(src / "e16.png")
    assert not api.png_info((src / "e16.png").read_bytes())["supported"]
    Image.fromarray(field(rng, 48, 40, 3)).save(src / "f_jpeg_named.png", "JPEG", quality=90)   # not a PNG: Pillow's
    res = {}
    for dec in ("pillow", "device"):
        out = tmp_path / dec
        res[dec] = driver.batch_process(src, out, process_wb=True, process_ndvi=True, verbose=False, png_decoder=dec)
        # the device decoder ran for a.png and b.png only: never for the 16-bit PNG, the TIFF, the JPEGs, or with "pillow"
        assert sorted(decoded) == ([] if dec == "pillow" else [(80, 64, 4), (96, 128, 3)]), (dec, decoded)
    assert not isinstance(res["device"]["f_jpeg_named.png"], Exception)
    assert set(res["pillow"]) == set(res["device"])
    for k, v in res["pillow"].items():
        if isinstance(v, Exception):
            assert type(res["device"][k]) is type(v)
        else:
            assert v == res["device"][k], k
    files = sorted(p.relative_to(tmp_path / "pillow") for p in (tmp_path / "pillow").rglob("*") if p.is_file())
    assert files == sorted(p.relative_to(tmp_path / "device") for p in (tmp_path / "device").rglob("*") if p.is_file())
    for f in files:
        assert (tmp_path / "pillow" / f).read_bytes() == (tmp_path / "device" / f).read_bytes(), f


def test_seeded_fuzz():
    rng = np.random.default_rng(20261016)
    for _ in range(200):
        mode = ["L", "LA", "RGB", "RGBA", "P"][rng.integers(5)]
        h, w = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        kind = rng.integers(3)
        if kind == 0:
            img = noise(rng, mode, h, w)
        elif kind == 1:
            img = gradient(mode, h, w)
        else:
            img = field(rng, h, w, CHANNELS[mode])
        save = {"compress_level": int(rng.integers(0, 10))} if rng.integers(4) else {"optimize": True}
        same(pil_png(img, mode, **save))
