"""CPU side of the device PNG encoder (api.encode_png, lars_png_bound) and the independent PNG checker the GPU tests use.

The checker never trusts Pillow alone (Pillow skips IDAT CRCs): it parses every chunk, checks every CRC with zlib.crc32,
inflates the joined IDATs with zlib (which checks the stream and its Adler-32), checks each row's filter byte against a
NumPy rendering of libpng's heuristic and the filtered rows against the same rendering, and un-filters the rows in NumPy.
"""
import struct
import zlib

import numpy as np
import pytest

from lars_image_processing_amd import _ffi, api, driver

SIG = b"\x89PNG\r\n\x1a\n"
COLOR_TYPES = {0: 1, 2: 3, 6: 4, 3: 1}                       # PNG colour type -> samples per pixel
SEG = 32768                                                  # png.hip PNG_SEG


# ---------------------------------------------------------------------------------------------------------------------
# the independent checker
# ---------------------------------------------------------------------------------------------------------------------
def parse_chunks(b):
    """[(type, data)] of a PNG file; every length and CRC checked."""
    assert b[:8] == SIG, b[:8]
    pos, chunks = 8, []
    while pos < len(b):
        assert pos + 12 <= len(b), "truncated chunk"
        (n,) = struct.unpack(">I", b[pos:pos + 4])
        typ, data = b[pos + 4:pos + 8], b[pos + 8:pos + 8 + n]
        assert len(data) == n, "truncated chunk data"
        (crc,) = struct.unpack(">I", b[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(typ + data) == crc, f"bad CRC in {typ} at byte {pos}"
        chunks.append((typ, data))
        pos += 12 + n
    assert pos == len(b)
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    return chunks


def filter_rows(img2d, bpp):
    """All five PNG filters of every row ([5][h][L] uint8) and libpng's choice per row: the smallest sum of |byte as int8|,
    ties to the lowest filter id."""
    x = img2d.astype(np.int16)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, bpp:] = b[:, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    f = np.stack([x, x - a, x - b, x - (a + b) // 2, x - pred]) & 255
    cost = np.minimum(f, 256 - f).sum(axis=2)                 # [5][h]
    return f.astype(np.uint8), np.argmin(cost, axis=0)        # argmin: the first minimum


def unfilter(raw, h, rowb, bpp):
    """Rows back from the inflated stream, in NumPy (per pixel for Average and Paeth)."""
    out = np.zeros((h, rowb), dtype=np.uint8)
    prev = np.zeros(rowb, dtype=np.int32)
    for y in range(h):
        ft, f = raw[y, 0], raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = f
        elif ft == 1:
            cur = np.zeros(rowb, dtype=np.int32)
            for k in range(bpp):
                cur[k::bpp] = np.cumsum(f[k::bpp]) & 255
        elif ft == 2:
            cur = (f + prev) & 255
        else:
            cur = np.zeros(rowb, dtype=np.int32)
            for i in range(rowb):
                a = cur[i - bpp] if i >= bpp else 0
                bb = prev[i]
                if ft == 3:
                    cur[i] = (f[i] + (a + bb) // 2) & 255
                else:
                    cc = prev[i - bpp] if i >= bpp else 0
                    p = a + bb - cc
                    pa, pb, pc = abs(p - a), abs(p - bb), abs(p - cc)
                    cur[i] = (f[i] + (a if pa <= pb and pa <= pc else (bb if pb <= pc else cc))) & 255
        assert ft <= 4, ft
        out[y] = cur
        prev = cur
    return out


def check_png(b, arr, palette=None, unfilter_limit=1 << 16):
    """Everything the device file must satisfy for the picture ``arr`` (uint8 [H, W] or [H, W, C])."""
    import io

    from PIL import Image
    arr = np.asarray(arr)
    h, w = arr.shape[:2]
    ch = 1 if arr.ndim == 2 else arr.shape[2]
    chunks = parse_chunks(b)
    ihdr = chunks[0][1]
    W, H, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", ihdr)
    assert (W, H, depth, comp, filt, interlace) == (w, h, 8, 0, 0, 0)
    assert COLOR_TYPES[ctype] == ch and (ctype == 3) == (palette is not None)
    types = [t for t, _ in chunks]
    if palette is not None:
        pal = np.asarray(palette, dtype=np.uint8)
        assert types[1:3] == [b"PLTE", b"tRNS"]
        assert chunks[1][1] == pal[:, :3].tobytes() and chunks[2][1] == pal[:, 3].tobytes()
    idat = [d for t, d in chunks if t == b"IDAT"]
    assert types[len(types) - len(idat) - 1:-1] == [b"IDAT"] * len(idat), "IDATs must be consecutive"
    assert idat[0][:2] == b"\x78\x01"
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)   # stream + Adler-32 checked by zlib
    rowb = w * ch
    assert raw.size == h * (rowb + 1)
    raw = raw.reshape(h, rowb + 1)
    img2d = arr.reshape(h, rowb)
    choices = []
    for y0 in range(0, h, 512):                               # blocks of rows (with the row above) bound the memory
        lo = max(0, y0 - 1)
        f, choice = filter_rows(img2d[lo:y0 + 512], ch)
        f, choice = f[:, y0 - lo:], choice[y0 - lo:]
        assert np.array_equal(raw[y0:y0 + 512, 0], choice), f"filter bytes differ from libpng's heuristic (rows {y0}+)"
        assert np.array_equal(raw[y0:y0 + 512, 1:], f[choice, np.arange(choice.size)]), f"filtered rows differ (rows {y0}+)"
        choices.append(choice)
    choice = np.concatenate(choices)
    if h * rowb <= unfilter_limit:
        assert np.array_equal(unfilter(raw, h, rowb, ch), img2d)
    im = Image.open(io.BytesIO(b))
    assert np.array_equal(np.asarray(im), arr)
    if palette is not None:
        assert np.array_equal(np.asarray(im.convert("RGBA")), np.asarray(palette, dtype=np.uint8)[arr])
    return choice


def deflate_blocks(b):
    """BTYPE of every deflate block of the file, in order (for the stored / dynamic split)."""
    data = b"".join(d for t, d in parse_chunks(b) if t == b"IDAT")[2:]
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")
    # only walks files whose blocks are all stored (BTYPE 0): enough to see the fallback
    pos, out = 0, []
    while True:
        final, btype = bits[pos], bits[pos + 1] | (bits[pos + 2] << 1)
        out.append(int(btype))
        if btype != 0:
            return out
        pos = (pos + 3 + 7) // 8 * 8
        n = int.from_bytes(np.packbits(bits[pos:pos + 16], bitorder="little").tobytes(), "little")
        pos += 32 + 8 * n
        if final:
            return out


# ---------------------------------------------------------------------------------------------------------------------
# tests without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def bound(h, w, c):
    return _ffi.load().lars_png_bound(h, w, c)


@pytest.mark.parametrize("h,w,c", [(1, 1, 1), (1, 1, 3), (1, 1, 4), (7, 5, 3), (64, 67, 4), (4096, 4096, 4), (2048, 2048, 3),
                                   (1, 20000, 4), (100000, 1, 1)])
def test_png_bound_allows_raw_segments(h, w, c):
    """Every 32 KiB segment may be stored: raw filtered bytes + 5 per segment + 12 per IDAT, zlib header and Adler-32,
    signature, IHDR, a 256-entry PLTE + tRNS for one channel, IEND."""
    raw = h * (w * c + 1)
    nseg = -(-raw // SEG)
    head = 8 + 25 + (24 + 4 * 256 if c == 1 else 0)
    assert bound(h, w, c) == raw + 17 * nseg + 6 + head + 12
    assert _ffi.load().lars_png_scratch_bytes(h, w, c) >= raw + nseg * SEG


@pytest.mark.parametrize("h,w,c", [(0, 5, 3), (5, 0, 3), (-1, 5, 3), (5, 5, 2), (5, 5, 5), (5, 5, 0), ((1 << 24) + 1, 1, 1),
                                   (1, (1 << 24) + 1, 1)])
def test_png_bound_refuses_bad_shapes(h, w, c):
    assert bound(h, w, c) == 0
    assert _ffi.load().lars_png_scratch_bytes(h, w, c) == 0


def test_png_bound_grows_with_the_picture():
    assert bound(1, 1, 4) < bound(1, 2, 4) < bound(2, 2, 4)
    assert bound(100, 100, 3) < bound(100, 100, 4)


def _no_device(*_a, **_k):
    raise AssertionError("the library was asked for a device")


@pytest.mark.parametrize("want_png", ["rgba", "yes", 1, 0, None, "PALETTE", 2.0])
def test_bad_want_png_raises_before_the_library(monkeypatch, want_png):
    monkeypatch.setattr(_ffi, "call", _no_device)
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="want_png"):
        api.process_image(img, want_png=want_png)


def test_want_png_excludes_host_pictures(monkeypatch):
    monkeypatch.setattr(_ffi, "call", _no_device)
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    for kw in ({"want_rgba": True}, {"want_entries": True}):
        with pytest.raises(ValueError, match="want_png"):
            api.process_image(img, want_png=True, **kw)


@pytest.mark.parametrize("enc", ["zlib", "gpu", "", None, "Device"])
def test_bad_png_encoder_raises_before_the_library(monkeypatch, tmp_path, enc):
    monkeypatch.setattr(_ffi, "call", _no_device)
    with pytest.raises(ValueError, match="png_encoder"):
        driver.process_image(tmp_path / "missing.tif", tmp_path, indices=["NDVI"], png_encoder=enc)
    with pytest.raises(ValueError, match="png_encoder"):
        driver.batch_process(tmp_path, tmp_path / "out", png_encoder=enc, verbose=False)
    with pytest.raises(ValueError, match="png_encoder"):
        driver.export_zip(np.zeros((4, 4, 3), dtype=np.uint8), ["NDVI"], png_encoder=enc)


def test_cli_offers_the_png_encoder(capsys):
    with pytest.raises(SystemExit):
        driver.main(["--help"])
    assert "--png-encoder" in capsys.readouterr().out


@pytest.mark.parametrize("arr,palette,exc", [
    (np.zeros((4, 4), dtype=np.uint16), None, TypeError),
    (np.zeros((4, 4), dtype=np.float32), None, TypeError),
    (np.zeros((4, 4, 2), dtype=np.uint8), None, ValueError),
    (np.zeros((4, 4, 5), dtype=np.uint8), None, ValueError),
    (np.zeros((4,), dtype=np.uint8), None, ValueError),
    (np.zeros((0, 4), dtype=np.uint8), None, ValueError),
    (np.zeros((4, 4, 3), dtype=np.uint8), np.zeros((4, 4), dtype=np.uint8), ValueError),
    (np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 3), dtype=np.uint8), ValueError),
    (np.zeros((4, 4), dtype=np.uint8), np.zeros((257, 4), dtype=np.uint8), ValueError),
    (np.zeros((4, 4), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8), ValueError),
])
def test_encode_png_refuses_before_the_library(monkeypatch, arr, palette, exc):
    monkeypatch.setattr(_ffi, "call", _no_device)
    with pytest.raises(exc):
        api.encode_png(arr, palette)


def test_encode_png_is_exported():
    import lars_image_processing_amd as lars
    assert lars.encode_png is api.encode_png


def test_checker_accepts_zlib_files_and_rejects_damage():
    """The checker itself, on files built here with zlib from the same filtered rows."""
    rng = np.random.default_rng(3)
    arr = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    arr[4:] = arr[3]
    f, choice = filter_rows(arr.reshape(9, -1), 3)
    raw = np.concatenate([choice[:, None].astype(np.uint8), f[choice, np.arange(9)]], axis=1)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    z = zlib.compress(raw.tobytes(), 1)
    z = b"\x78\x01" + z[2:]
    good = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", 13, 9, 8, 2, 0, 0, 0)) + chunk(b"IDAT", z[:10]) + \
        chunk(b"IDAT", z[10:]) + chunk(b"IEND", b"")
    check_png(good, arr)
    bad = bytearray(good)
    bad[45] ^= 1                                              # a byte inside the first IDAT
    with pytest.raises(AssertionError):
        check_png(bytes(bad), arr)
    with pytest.raises(AssertionError):
        check_png(good, arr[::-1].copy())
