"""The exact stream the device writes for one strip of a Deflate TIFF file (csrc/tiff_encode.hip, k_tz_deflate and k_tz_join), and
the size of the file around the strips.

A strip of n stored bytes has p = ceil(n / 32768) parts.  Lane 0's decisions for a part -- code lengths, codes, the dynamic
block's header, stored or dynamic -- are png_encode_model.segment()'s, since the kernel is the PNG encoder's segment coder
(csrc/deflate_device.h).  The literals are packed here, with NumPy; the flushes between the parts, the 78 01 header and the
Adler-32 are added here.  zlib judges the result in tests/test_tiff_deflate_encode_cpu.py."""
import os
import struct
import tempfile
import zlib

import numpy as np

import png_encode_model as pm
from lars_image_processing_amd import tiffio

SEG = pm.SEG


def part(data, last):
    """The bytes of one part: the block, and behind a dynamic block that is not the strip's last the empty stored block."""
    data = bytes(data)
    n = len(data)
    seg = pm.segment(data, last)
    if seg["stored"]:
        return bytes([1 if last else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + data
    lengths = np.array([length for length, _ in seg["table"]], dtype=np.int64)
    codes = np.array([code for _, code in seg["table"]], dtype=np.int64)
    symbols = np.concatenate([np.frombuffer(data, dtype=np.uint8).astype(np.int64), [256]])
    ln, cd = lengths[symbols], codes[symbols]
    assert ln.min() > 0
    start = seg["hdr_bits"] + np.concatenate([[0], np.cumsum(ln)[:-1]])
    end = int(start[-1] + ln[-1])
    nbytes = (end + 7) // 8 if last else (end + 3 + 7) // 8
    bits = np.zeros(8 * nbytes, dtype=np.uint8)
    for j in range(seg["hdr_bits"]):
        bits[j] = (seg["header"] >> j) & 1
    for j in range(15):                                     # bit j of every code that has one (codes are stored bit-reversed: LSB first)
        has = ln > j
        bits[start[has] + j] = (cd[has] >> j) & 1
    out = np.packbits(bits, bitorder="little").tobytes()
    if not last:
        out += b"\x00\x00\xff\xff"
    assert len(out) == seg["huff_bytes"]
    return out


def strip_stream(data):
    """The zlib stream of one strip."""
    data = bytes(data)
    assert len(data) >= 1
    out = [b"\x78\x01"]
    for at in range(0, len(data), SEG):
        out.append(part(data[at:at + SEG], at + SEG >= len(data)))
    out.append(struct.pack(">I", zlib.adler32(data)))
    return b"".join(out)


def reference_file(a, rows_per_strip, predictor):
    """tiffio's own Deflate file of ``a`` (write_tiff or, for float32, write_float_tiff): its directory is the device's, and
    its strips inflate to the stored bytes."""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "w.tif")
        if a.dtype == np.float32:
            tiffio.write_float_tiff(p, a, rows_per_strip=rows_per_strip, deflate=True, predictor=3 if predictor else 1)
        else:
            tiffio.write_tiff(p, a, rows_per_strip=rows_per_strip, deflate=True, predictor=bool(predictor))
        with open(p, "rb") as f:
            return f.read()


def directory(blob):
    """{tag: (type, values)} of a little-endian classic TIFF, the directory's offset, and the bytes the directory and its
    arrays take."""
    assert blob[:4] == b"II*\0"
    (ifd,) = struct.unpack_from("<I", blob, 4)
    (count,) = struct.unpack_from("<H", blob, ifd)
    tags, size = {}, 2 + 12 * count + 4
    for i in range(count):
        tag, typ, n = struct.unpack_from("<HHI", blob, ifd + 2 + 12 * i)
        item = {3: 2, 4: 4}[typ]
        inline = item * n <= 4
        where = ifd + 10 + 12 * i if inline else struct.unpack_from("<I", blob, ifd + 10 + 12 * i)[0]
        tags[tag] = (typ, struct.unpack_from("<%d%s" % (n, "H" if typ == 3 else "I"), blob, where))
        size += 0 if inline else item * n
    assert struct.unpack_from("<I", blob, ifd + 2 + 12 * count)[0] == 0
    return tags, ifd, size


def stored_strips(a, rows_per_strip, predictor):
    """(the stored bytes of every strip, the reference file's tags, the directory's size)."""
    ref = reference_file(a, rows_per_strip, predictor)
    tags, _, size = directory(ref)
    offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
    return [zlib.decompress(ref[o:o + n]) for o, n in zip(offsets, counts)], tags, size


def file_size(streams, directory_size):
    """The device file's length: header, strips on even offsets, directory."""
    return 8 + sum(len(s) + (len(s) & 1) for s in streams) + directory_size
