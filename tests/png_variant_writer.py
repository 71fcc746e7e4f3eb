"""A PNG writer for the variants Pillow cannot write: any valid (colour type, bit depth), Adam7 interlace, a chosen or seeded
filter type per row, PLTE for palettes, IDAT splitting.  Pillow reads every file built here, and Pillow's array is what the
tests expect, so this writer is never the oracle; tests/test_png_variants_cpu.py checks its files against Pillow first."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]     # x0, y0, dx, dy


def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


def bpp_of(ctype, depth):
    return max(1, CHANNELS[ctype] * depth // 8)


def random_samples(rng, h, w, ctype, depth):
    """Samples ``[h, w, channels]`` of the full range of the depth."""
    return rng.integers(0, 1 << depth, (h, w, CHANNELS[ctype]), dtype=np.uint16 if depth == 16 else np.uint8)


def pack_rows(sub, depth):
    """``[ph, pw, channels]`` samples -> ``[ph, row_bytes]`` bytes: MSB first below 8 bits, big-endian at 16."""
    ph, pw, c = sub.shape
    if depth == 8:
        return sub.reshape(ph, pw * c).astype(np.uint8)
    if depth == 16:
        return sub.astype(">u2").view(np.uint8).reshape(ph, pw * c * 2)
    bits = ((sub.reshape(ph, pw * c, 1).astype(np.uint8) >> np.arange(depth - 1, -1, -1, dtype=np.uint8)) & 1).reshape(ph, pw * c * depth)
    return np.packbits(bits, axis=1)                                     # pads the last byte of every row with zeros


def filter_row(ftype, raw, prior, bpp):
    raw = raw.astype(np.int32)
    b = prior.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), raw[:-bpp]]) if bpp < len(raw) else np.zeros_like(raw)
    c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if bpp < len(raw) else np.zeros_like(raw)
    if ftype == 0:
        pred = 0
    elif ftype == 1:
        pred = a
    elif ftype == 2:
        pred = b
    elif ftype == 3:
        pred = (a + b) >> 1
    else:
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return ((raw - pred) & 255).astype(np.uint8)


def filtered_stream(samples, ctype, depth, interlace=False, filters=None, seed=0):
    """The bytes zlib compresses.  ``filters``: None for a seeded type per row, an int for that type on every row, or a
    callable ``(pass number, row) -> type`` (values above 4 are written as they are, for damage tests)."""
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[:, :, None]
    h, w, c = samples.shape
    assert c == CHANNELS[ctype] and (ctype, depth) in PAIRS
    rng = np.random.default_rng(seed)
    bpp = bpp_of(ctype, depth)
    out = []
    for k, (x0, y0, dx, dy) in enumerate(ADAM7 if interlace else [(0, 0, 1, 1)]):
        sub = samples[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        rows = pack_rows(sub, depth)
        prior = np.zeros(rows.shape[1], np.uint8)
        for r, raw in enumerate(rows):
            f = int(rng.integers(0, 5)) if filters is None else filters if isinstance(filters, int) else filters(k + 1 if interlace else 0, r)
            out.append(bytes([f]) + filter_row(f if f <= 4 else 0, raw, prior, bpp).tobytes())
            prior = raw
    return b"".join(out)


def write_png(samples, ctype, depth, interlace=False, filters=None, seed=0, palette=None, idat_split=None, level=6, stream=None):
    """The file.  ``palette``: ``[n, 3]`` uint8 for colour type 3 (default: a seeded one with 2^depth entries);
    ``idat_split``: the compressed stream is cut into IDAT chunks of that many bytes; ``stream``: filtered bytes to
    compress instead of the samples' (damage tests)."""
    samples = np.asarray(samples)
    h, w = samples.shape[:2]
    raw = filtered_stream(samples, ctype, depth, interlace, filters, seed) if stream is None else stream
    z = zlib.compress(raw, level)
    out = [SIG, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 1 if interlace else 0))]
    if ctype == 3:
        if palette is None:
            palette = np.random.default_rng(seed + 1).integers(0, 256, (1 << depth, 3), dtype=np.uint8)
        out.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    n = idat_split or max(1, len(z))
    out += [chunk(b"IDAT", z[i:i + n]) for i in range(0, len(z), n)]
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def expected_array(samples, ctype, depth):
    """What Pillow's ``np.asarray`` gives for the samples (the table of the extended decoder), for the writer's own check."""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[:, :, None]
    if ctype == 3:
        return s[:, :, 0].astype(np.uint8)
    if ctype == 0:
        if depth == 1:
            return s[:, :, 0].astype(bool)
        if depth == 16:
            return s[:, :, 0].astype(np.uint16)
        return (s[:, :, 0].astype(np.uint8) * {2: 85, 4: 17, 8: 1}[depth]).astype(np.uint8)
    hi = (s >> 8).astype(np.uint8) if depth == 16 else s.astype(np.uint8)
    if ctype == 4 and depth == 16:
        return np.dstack([hi[:, :, 0], hi[:, :, 0], hi[:, :, 0], hi[:, :, 1]])
    return hi
