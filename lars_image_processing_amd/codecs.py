"""The file codecs: PNG, JPEG and TIFF files built and decoded on the device, their ``*_info`` readers on the host and the
thumbnails made straight from a file's bytes.  ``api`` re-exports every public name here but ``deflate_matching`` (a setting, not
a codec: the package exports it itself); this module does not import ``api``.
Every operation takes one path through the helpers below.  ``_ffi.call`` and ``_ffi.load`` are looked up on ``_ffi`` at every
call: the CPU tests replace them to see what is asked of the library.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _ffi
from .thumbplan import jpeg_draft_scale, thumbnail_plan, thumbnail_size
from .tiffio import TiffError


def _shape(h, w, c):
    """``[H, W]`` for one sample per pixel, ``[H, W, C]`` otherwise: the arrays Pillow gives."""
    return (h, w) if c == 1 else (h, w, c)


def _host_query(fn_name, *args):
    """A host function of the library that answers through its arguments; a refusal is ``ValueError`` with the library's words."""
    lib = _ffi.load()
    if getattr(lib, fn_name)(*args) != 0:
        raise ValueError(lib.lars_last_error().decode("utf-8", "replace"))


def _file_call(name, *args, error=ValueError):
    """``_ffi.call`` of a decoder: LARS_ERR_INVALID there speaks of the file's contents and becomes ``error``."""
    try:
        _ffi.call(name, *args)
    except _ffi.LarsError as e:
        if e.code == -1:
            raise error(str(e)) from None
        raise


def _file_thumbnail(name, arr, plan, c, *lead, error=ValueError):
    """The call every thumbnail from a file's bytes ends in: ``plan`` applied to the decoded file on the device (``lead``: what
    the entry point takes between the file and the plan)."""
    new_w, new_h = plan.size
    out = np.empty(_shape(new_h, new_w, c), dtype=np.uint8)
    _file_call(name, _ffi.ptr(arr), arr.size, *lead, plan.factor[0], plan.factor[1], (C.c_int * 4)(*plan.reduce_box),
               (C.c_float * 4)(*plan.box), new_h, new_w, int(plan.vertical_first), _ffi.ptr(out), error=error)
    return out


def _encode_call(name, nbytes, *args):
    """The call every encoder ends in: a buffer of ``nbytes`` for the file, ``args`` in front of it, the bytes written."""
    out = np.empty(nbytes, dtype=np.uint8)
    n = C.c_int64(0)
    _ffi.call(name, *args, _ffi.ptr(out), out.nbytes, C.byref(n))
    return out[:n.value].tobytes()


@contextlib.contextmanager
def deflate_matching(on=True):
    """``with deflate_matching(): ...`` -- inside the block the Deflate coder of ``encode_png``, ``encode_tiff(...,
    compression="deflate")``, ``encode_tiff_f32(..., compression="deflate")`` and of ``process_image``'s ``want_png`` /
    ``want_tiff="deflate..."`` files searches every 32 KiB segment for repeats (LZ77 length / distance pairs) instead of coding
    literals only: the same pixels and the same bounds, smaller files on masks, class pictures, flat areas and colormap
    pictures, never a larger one (a segment that gains nothing is written as without it).  The tuning knob
    ``deflate_matching``, one per process: do not enter it from threads that encode at the same time with different wishes.
    On leaving, the knob is what it was."""
    with _ffi.tuning(deflate_matching=1 if on else 0):
        yield


# ---------------------------------------------------------------------------
# PNG files built on the device
# ---------------------------------------------------------------------------
_PNG_CHANNELS = (1, 3, 4)


def _uint8_picture(array, who):
    """What ``encode_png`` and ``encode_jpeg`` open with: the array, uint8 or refused, ``[H, W, 1]`` taken as ``[H, W]``."""
    arr = np.asarray(array)
    if arr.dtype != np.uint8:
        raise TypeError(f"{who}: uint8 pictures only, got {arr.dtype}")
    return arr[:, :, 0] if arr.ndim == 3 and arr.shape[2] == 1 else arr


def png_bound(h, w, channels):
    """The largest file ``encode_png`` can return for an ``h x w`` picture of ``channels`` samples (``lars_png_bound``;
    host code, no device needed)."""
    return int(_ffi.load().lars_png_bound(int(h), int(w), int(channels)))


def encode_png(array, palette=None):
    """PNG file (``bytes``) of a uint8 picture, encoded on the GPU: ``[H, W]`` (mode L), ``[H, W, 3]`` (RGB) or ``[H, W, 4]``
    (RGBA); with ``palette`` (``N x 4`` uint8 RGBA, N <= 256) a ``[H, W]`` array is written as mode P with PLTE + tRNS.

    ``Image.open(io.BytesIO(b))`` gives back exactly ``array`` (``.convert("RGBA")`` the palette's colours for P); the
    compressed bytes are not zlib's.  The same input always gives the same bytes.  What ``Image.fromarray(array).save(f,
    "PNG")`` does at the end of every index picture (backend-process.py:70) and ZIP entry (process-images.py:567-617).
    """
    arr = _uint8_picture(array, "encode_png")
    if arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in _PNG_CHANNELS):
        raise ValueError(f"encode_png: shape [H, W], [H, W, 3] or [H, W, 4] expected, got {arr.shape}")
    h, w = arr.shape[:2]
    c = 1 if arr.ndim == 2 else arr.shape[2]
    if not (1 <= h <= 1 << 24 and 1 <= w <= 1 << 24):
        raise ValueError(f"encode_png: {h} x {w} picture (1 to 2^24 on each side)")
    pal, npal = None, 0
    if palette is not None:
        pal = np.ascontiguousarray(np.asarray(palette), dtype=np.uint8)
        if c != 1:
            raise ValueError("encode_png: a palette needs a [H, W] array of entries")
        if pal.ndim != 2 or pal.shape[1] != 4 or not 1 <= pal.shape[0] <= 256:
            raise ValueError(f"encode_png: palette must be N x 4 RGBA with 1 <= N <= 256, got {pal.shape}")
        npal = pal.shape[0]
    arr = np.ascontiguousarray(arr)
    return _encode_call("lars_h_encode_png_u8", png_bound(h, w, c), _ffi.ptr(arr), h, w, c, _ffi.ptr(pal), npal)


# ---------------------------------------------------------------------------
# JPEG files built on the device
# ---------------------------------------------------------------------------
_JPEG_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2, 0: 0, 1: 1, 2: 2}


def jpeg_bound(h, w, channels, subsampling=2):
    """The largest file ``encode_jpeg`` can return for an ``h x w`` picture of ``channels`` samples at any quality
    (``lars_jpeg_bound``; host code, no device needed); 0 for a shape that cannot be encoded."""
    return int(_ffi.load().lars_jpeg_bound(int(h), int(w), int(channels), int(subsampling)))


def encode_jpeg(array, quality=75, subsampling="4:2:0"):
    """Baseline JPEG file (``bytes``) of a uint8 picture, encoded on the GPU: ``[H, W]`` (mode L) or ``[H, W, 3]`` (RGB, stored
    as YCbCr).  ``quality`` 1 to 100; ``subsampling`` ``"4:4:4"``, ``"4:2:2"``, ``"4:2:0"`` or Pillow's 0, 1, 2 (for
    ``[H, W]`` the data do not depend on it; as in Pillow's files, one byte of the frame header does).  1 <= H, W <= 65500 and fewer than 2^31 samples.

    The bytes are exactly those of ``Image.fromarray(array).save(f, "JPEG", quality=quality, subsampling=subsampling)`` with
    Pillow on libjpeg-turbo: what ends the camera path (process-rgn.py:47 with :72-73) and an upload kept in its own format
    (process-images.py:247).  ``optimize``, progressive files, restart intervals and metadata are not covered.
    """
    arr = _uint8_picture(array, "encode_jpeg")
    if arr.ndim == 3 and arr.shape[2] == 4:
        raise TypeError("encode_jpeg: cannot write mode RGBA as JPEG")
    if arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] != 3):
        raise ValueError(f"encode_jpeg: shape [H, W] or [H, W, 3] expected, got {arr.shape}")
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)):
        raise TypeError(f"encode_jpeg: quality must be an int, got {quality!r}")
    if not 1 <= quality <= 100:
        raise ValueError(f"encode_jpeg: quality 1 to 100, got {quality}")
    if isinstance(subsampling, bool) or not isinstance(subsampling, (str, int)) or subsampling not in _JPEG_SUBSAMPLING:
        raise ValueError(f"encode_jpeg: subsampling '4:4:4', '4:2:2', '4:2:0' or 0, 1, 2, got {subsampling!r}")
    h, w = arr.shape[:2]
    c = 1 if arr.ndim == 2 else 3
    if not (1 <= h <= 65500 and 1 <= w <= 65500):
        raise ValueError(f"encode_jpeg: {h} x {w} picture (1 to 65500 on each side)")
    if h * w * c >= 1 << 31:
        raise ValueError(f"encode_jpeg: {h} x {w} x {c} samples (fewer than 2^31)")
    sub = _JPEG_SUBSAMPLING[subsampling]
    arr = np.ascontiguousarray(arr)
    return _encode_call("lars_h_encode_jpeg_u8", jpeg_bound(h, w, c, sub), _ffi.ptr(arr), h, w, c, int(quality), sub)


# ---------------------------------------------------------------------------
# TIFF files built on the device
# ---------------------------------------------------------------------------
# (float32 samples, Deflate) -> (the encoder, its bound); the integer entry points take the sample size after the channels
_TIFF_ENCODERS = {(False, False): ("lars_h_encode_tiff", "lars_tiff_bound"),
                  (False, True): ("lars_h_encode_tiff_deflate", "lars_tiff_deflate_bound"),
                  (True, False): ("lars_h_encode_tiff_f32", "lars_tiff_f32_bound"),
                  (True, True): ("lars_h_encode_tiff_deflate_float32", "lars_tiff_float32_deflate_bound")}


def _tiff_picture(array, rows_per_strip, who, f32=False):
    """What ``encode_tiff`` and ``encode_tiff_f32`` open with, before anything is launched: (C-contiguous ``[H, W, C]`` array, rows
    per strip or 0)."""
    arr = np.asarray(array)
    if f32 and arr.dtype != np.float32:
        raise TypeError(f"{who}: float32 pictures only, got {arr.dtype} (nothing is cast)")
    if not f32 and arr.dtype not in (np.uint8, np.uint16):
        raise TypeError(f"{who}: uint8 or uint16 pictures only, got {arr.dtype}")
    if arr.ndim == 2:
        arr = arr[:, :, None]
    if arr.ndim != 3:
        raise ValueError(f"{who}: shape [H, W] or [H, W, C] expected, got {arr.shape}")
    if arr.size == 0:
        raise ValueError(f"{who}: empty picture of shape {arr.shape}")
    h, w, c = arr.shape
    if not 1 <= c <= 5:
        raise ValueError(f"{who}: 1 to 5 samples per pixel, got {c}")
    if not (h <= 1 << 24 and w <= 1 << 24):
        raise ValueError(f"{who}: {h} x {w} picture (1 to 2^24 on each side)")
    if rows_per_strip is None:
        rps = 0
    else:
        if isinstance(rows_per_strip, bool) or not isinstance(rows_per_strip, (int, np.integer)):
            raise TypeError(f"{who}: rows_per_strip must be an int or None, got {rows_per_strip!r}")
        if rows_per_strip < 1:
            raise ValueError(f"{who}: rows_per_strip must be positive, got {rows_per_strip}")
        rps = min(int(rows_per_strip), h)
    if not arr.dtype.isnative:
        arr = arr.astype(arr.dtype.newbyteorder("="))
    return np.ascontiguousarray(arr), rps


def _tiff_compression(compression, who):
    """``compression`` of the TIFF encoders, checked before anything is launched: True for ``"deflate"``, False for ``"lzw"``."""
    if not isinstance(compression, str) or compression not in ("lzw", "deflate"):
        raise ValueError(f"{who}: compression must be 'lzw' or 'deflate', got {compression!r}")
    return compression == "deflate"


def _tiff_bound(who, h, w, channels, itemsize, rows_per_strip, compression, f32):
    """The library's bound for the file of either TIFF encoder; ``itemsize`` is only passed on for integer samples."""
    name = _TIFF_ENCODERS[f32, _tiff_compression(compression, who)][1]
    size = () if f32 else (int(itemsize),)
    return int(getattr(_ffi.load(), name)(int(h), int(w), int(channels), *size, int(rows_per_strip or 0)))


def _encode_tiff(who, array, rows_per_strip, predictor, compression, f32):
    """``encode_tiff`` (``f32=False``) and ``encode_tiff_f32`` (``f32=True``)."""
    deflate = _tiff_compression(compression, who)
    arr, rps = _tiff_picture(array, rows_per_strip, who, f32)
    h, w, c = arr.shape
    itemsize = arr.dtype.itemsize
    bound = _tiff_bound(who, h, w, c, itemsize, rps, compression, f32)
    if bound == 0:
        raise ValueError(f"{who}: strips of {rps or 'the default number of'} rows of {w * c * itemsize} bytes are too long (2^30 bytes at most)")
    nbytes = min(bound, 1 << 32)
    size = () if f32 else (itemsize,)
    try:
        return _encode_call(_TIFF_ENCODERS[f32, deflate][0], nbytes, _ffi.ptr(arr), h, w, c, *size, rps, int(bool(predictor)))
    except _ffi.LarsError as e:
        if e.code == -6 or (e.code == -1 and bound > nbytes):
            raise TiffError("image too large for a classic TIFF (4 GiB)") from None
        raise


def tiff_bound(h, w, channels, itemsize, rows_per_strip=None, compression="lzw"):
    """The largest file ``encode_tiff`` can return for an ``h x w`` picture of ``channels`` samples of ``itemsize`` bytes
    (``lars_tiff_bound``; host code, no device needed); 0 for a shape that cannot be encoded.

    The derivation, strip by strip: the stream opens with a Clear and ends with EndOfInformation; every other code but the
    Clears that follow a full table stands for at least one input byte, so a strip of n bytes gives at most n of them; the
    table is full after 3836 codes, so at most n // 3836 Clears follow; no code is wider than 12 bits.  That is
    ``ceil(12 * (n + n // 3836 + 2) / 8)`` bytes, plus one where that is odd (strips start on even offsets).  Around the
    strips: 8 bytes of header, a directory of at most 13 entries (2 + 12 * 13 + 4 bytes), BitsPerSample and SampleFormat
    (``2 * channels`` bytes each), and 8 bytes of offset and byte count per strip.  ``rows_per_strip=None``: the rows the
    knob ``tiff_strip_bytes`` gives, as in ``encode_tiff``.

    ``compression="deflate"`` (``lars_tiff_deflate_bound``): per strip of n bytes in ``p = ceil(n / 32768)`` parts, 2 bytes of
    zlib header, the n bytes, 5 bytes per part (a stored block's header; a dynamic block with its flush is only written where it
    is no longer than the stored form), 4 bytes of Adler-32 -- ``n + 5 * p + 6`` -- plus one where that is odd; around the strips
    the same."""
    return _tiff_bound("tiff_bound", h, w, channels, itemsize, rows_per_strip, compression, False)


def encode_tiff(array, rows_per_strip=None, predictor=False, compression="lzw"):
    """LZW or Deflate TIFF file (``bytes``) of a picture, encoded on the GPU: ``[H, W]`` or ``[H, W, C]`` with C = 1..5, uint8 or uint16.

    A classic little-endian TIFF with strips, chunky samples and Compression 5; ``predictor=True`` writes Predictor 2
    (horizontal differencing per sample modulo 2^bits, every row on its own).  The directory holds the tags and values of
    ``tiffio.write_tiff`` for the same array and ``rows_per_strip`` (RGB for C >= 3, BlackIsZero otherwise, samples past the
    third as unspecified extra samples), strip data first, every strip on an even offset.  ``rows_per_strip=None``: the most
    rows whose uncompressed strip stays within the tuning knob ``tiff_strip_bytes`` (65536, libtiff's and Pillow's strip
    size), at least one.  Every strip is the greedy encoder's stream with a Clear code when the table holds 4094 codes: the
    bytes libtiff writes for that strip.  What ``Image.fromarray(corrected).save(".../<name>_wb.tif")`` does for the batch
    job's primary output (backend-process.py:57), compressed.

    ``compression="deflate"`` writes Compression 8 instead, the same strips, directory (``tiffio.write_tiff(..., deflate=True)``'s)
    and predictor: every strip is a zlib stream whose 32768-byte parts are coded in parallel, each as a dynamic Huffman block over
    literals only (zlib's ``Z_HUFFMAN_ONLY``) or a stored block where that is not shorter, with an empty stored block between
    parts.  No string matching: on predicted data that gives up little, on flat pictures a great deal (LZW is the smaller file
    there).  Any inflate reads it; ``decode_tiff(..., deflate=True)`` does on the device.

    ``TypeError`` / ``ValueError`` for other dtypes, shapes, empty arrays, C > 5 or another ``compression`` before anything is launched;
    ``tiffio.TiffError`` for a file that would reach 4 GiB.  No CPU fallback.
    """
    return _encode_tiff("encode_tiff", array, rows_per_strip, predictor, compression, False)


def tiff_f32_bound(h, w, channels, rows_per_strip=None, compression="lzw"):
    """The largest file ``encode_tiff_f32`` can return for an ``h x w`` picture of ``channels`` float32 samples
    (``lars_tiff_f32_bound``; host code, no device needed); 0 for a shape that cannot be encoded.  ``tiff_bound``'s derivation
    with rows of ``w * channels * 4`` bytes: per strip of n bytes ``ceil(12 * (n + n // 3836 + 2) / 8)`` bytes, plus one where
    that is odd; 8 bytes of header, 2 + 12 * 13 + 4 of directory, ``4 * channels`` of BitsPerSample and SampleFormat, 8 per
    strip.  ``rows_per_strip=None``: the rows the knob ``tiff_strip_bytes`` gives.  ``compression="deflate"``
    (``lars_tiff_float32_deflate_bound``): ``n + 5 * ceil(n / 32768) + 6`` bytes per strip, plus one where that is odd, as in
    ``tiff_bound``."""
    return _tiff_bound("tiff_f32_bound", h, w, channels, 4, rows_per_strip, compression, True)


def encode_tiff_f32(array, rows_per_strip=None, predictor=False, compression="lzw"):
    """LZW or Deflate TIFF file (``bytes``) of float32 samples, encoded on the GPU: ``[H, W]`` or ``[H, W, C]`` with C = 1..5 -- an index plane
    (``calculate_index``) kept bit for bit, in the file GDAL, rasterio and QGIS exchange such rasters in.

    ``encode_tiff``'s file (classic, little-endian, strips, chunky, Compression 5, the same strip rule and knob) with
    BitsPerSample 32 and SampleFormat 3; the directory is ``tiffio.write_float_tiff``'s.  ``predictor=True`` writes Predictor 3,
    the floating-point predictor (libtiff's fpDiff: every row as four byte planes, most significant first, differenced across
    the plane borders), computed from the picture as the encoder reads it.  Every strip is libtiff's stream for those bytes.
    ``compression="deflate"``: Compression 8 with ``encode_tiff``'s Deflate streams, the directory of
    ``tiffio.write_float_tiff(..., deflate=True)`` -- with ``predictor=True`` what GDAL writes for COMPRESS=DEFLATE PREDICTOR=3.

    ``TypeError`` for any dtype but float32 (float64 is not cast), ``TypeError`` / ``ValueError`` for shapes, empty arrays,
    C > 5 or another ``compression``, all before anything is launched; ``tiffio.TiffError`` for a file that would reach 4 GiB.  No CPU fallback.
    """
    return _encode_tiff("encode_tiff_f32", array, rows_per_strip, predictor, compression, True)


# ---------------------------------------------------------------------------
# PNG files decoded on the device
# ---------------------------------------------------------------------------
# Pillow's PngImagePlugin._MODES: (bit depth, colour type) -> mode
_PNG_MODES = {(1, 0): "1", (2, 0): "L", (4, 0): "L", (8, 0): "L", (16, 0): "I;16", (8, 2): "RGB", (16, 2): "RGB",
              (1, 3): "P", (2, 3): "P", (4, 3): "P", (8, 3): "P", (8, 4): "LA", (16, 4): "RGBA", (8, 6): "RGBA",
              (16, 6): "RGBA"}


def _file_bytes(data, who, fmt):
    """The bytes of a whole ``fmt`` ("PNG", "JPEG", "TIFF") file as a contiguous 1-D uint8 array."""
    if isinstance(data, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(data, dtype=np.uint8)
    elif isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1:
        arr = data
    else:
        raise TypeError(f"{who}: a whole {fmt} file as bytes, bytearray, memoryview or 1-D uint8 array expected, got {type(data).__name__}")
    return np.ascontiguousarray(arr)


def _png_info(arr):
    info = _ffi.PngInfo.array()
    _host_query("lars_png_info", _ffi.ptr(arr), arr.size, info, None, 0)
    return _ffi.PngInfo(*info)


def _png_out_format(i):
    """``(dtype, shape)`` of the array the extended decoder gives for the IHDR numbers ``i`` (``lars_png_out_format``, pure
    host code): Pillow's ``np.asarray`` of the file."""
    channels, itemsize = C.c_int(0), C.c_int(0)
    _host_query("lars_png_out_format", i.bit_depth, i.color_type, C.byref(channels), C.byref(itemsize))
    dtype = np.dtype(np.uint16) if itemsize.value == 2 else np.dtype(bool) if (i.bit_depth, i.color_type) == (1, 0) else np.dtype(np.uint8)
    return dtype, _shape(i.height, i.width, channels.value)


def _png_need(i):
    """Filtered bytes of all passes (``lars_png_layout``, pure host code)."""
    passes = (C.c_int64 * 70)()
    npass, need = C.c_int64(0), C.c_int64(0)
    _host_query("lars_png_layout", i.width, i.height, i.bit_depth, i.color_type, i.interlace, passes, C.byref(npass), C.byref(need))
    return need.value


def png_info(data, extended=False):
    """The chunk layout of a PNG file, validated on the host (``lars_png_info``; no device needed).

    Returns ``width``, ``height``, ``bit_depth``, ``color_type``, ``interlace``, ``mode`` (Pillow's name for it),
    ``channels``, ``idat_bytes`` and ``supported`` (what ``decode_png`` decodes: bit depth 8, no interlace, not APNG).
    ``extended=True``: ``supported`` is what ``decode_png(data, extended=True)`` decodes -- every valid IHDR combination
    that is not APNG -- and the dict gains ``dtype`` and ``shape`` of the array that call returns.
    Raises ``ValueError`` for structural damage: bad signature, missing or misplaced IHDR / IDAT / IEND, a chunk running
    past the end of the file, a bad CRC in a chunk other than IDAT (IDAT CRCs are checked where they are gathered).
    """
    i = _png_info(_file_bytes(data, "png_info", "PNG"))
    out = {"width": i.width, "height": i.height, "bit_depth": i.bit_depth, "color_type": i.color_type, "interlace": i.interlace,
           "mode": _PNG_MODES[(i.bit_depth, i.color_type)], "channels": i.channels, "idat_bytes": i.idat_bytes,
           "supported": bool(i.supported)}
    if extended:
        out["supported"] = not i.apng
        out["dtype"], out["shape"] = _png_out_format(i)
    return out


def _png_check(arr, who, extended=False):
    """The ``PngInfo`` of a file the plain or the extended decoder takes; refused otherwise: unsupported, then too large."""
    i = _png_info(arr)
    w, h, channels = i.width, i.height, i.channels
    sides = 1 <= h <= 1 << 24 and 1 <= w <= 1 << 24
    if extended:
        if i.apng:
            raise NotImplementedError(f"{who}: APNG PNG files are not supported")
        if not sides or _png_need(i) > (1 << 31) - 1:
            raise ValueError(f"{who}: {w} x {h} picture of {channels} channels at bit depth {i.bit_depth} is too large")
        return i
    if not i.supported:
        what = "APNG" if i.apng else "interlaced" if i.interlace else f"bit depth {i.bit_depth}"
        raise NotImplementedError(f"{who}: {what} PNG files are not supported (8-bit, non-interlaced only)")
    if not sides or h * (1 + w * channels) > (1 << 31) - 1:
        raise ValueError(f"{who}: {w} x {h} picture of {channels} channels is too large")
    return i


def decode_png(data, extended=False):
    """``np.asarray(Image.open(io.BytesIO(data)))`` of a PNG file, decoded on the GPU (process-images.py:181-193).

    ``data``: the whole file as ``bytes``, ``bytearray``, ``memoryview`` or a 1-D uint8 array.  Bit depth 8, no interlace,
    colour types 0 (L, ``[H, W]``), 2 (RGB, ``[H, W, 3]``), 3 (P: the palette indices, ``[H, W]``), 4 (LA, ``[H, W, 2]``) and
    6 (RGBA, ``[H, W, 4]``); ancillary chunks are skipped.  Other variants raise ``NotImplementedError``; damaged files
    raise ``ValueError`` saying what is wrong.  Stricter than Pillow on purpose: the CRC of every IDAT chunk and the
    zlib stream's Adler-32 trailer are always checked.  One exception: a stream that decodes to more bytes than the image
    needs (Pillow ignores the extra data) has the extra bytes dropped, not stored -- they could be up to 1032 times the
    compressed size -- so the Adler-32 over the whole stream cannot be formed, and that trailer is not checked.  Limits: 1 <= h, w <= 2^24 and
    ``h * (1 + w * channels) < 2^31``.  No CPU fallback.

    ``extended=True`` also decodes bit depths 1, 2, 4 and 16 and Adam7-interlaced files, every valid IHDR combination that
    is not APNG, to the array Pillow gives: ``bool`` for 1-bit gray, ``uint8`` samples times 85 / 17 for 2- / 4-bit gray,
    native-endian ``uint16`` for 16-bit gray (mode ``I;16``), the unscaled indices for palettes of any depth, the high
    byte of every sample for 16-bit RGB / RGBA, and ``[H, W, 4]`` = L, L, L, A of the high bytes for 16-bit LA (Pillow
    opens it as RGBA).  Interlace changes nothing in the result.  The limit is then on the filtered bytes of all passes,
    which must stay below 2^31; a bad filter byte is reported with its pass.
    """
    arr = _file_bytes(data, "decode_png", "PNG")
    i = _png_check(arr, "decode_png", extended)
    dtype, shape = _png_out_format(i) if extended else (np.dtype(np.uint8), _shape(i.height, i.width, i.channels))
    out = np.empty(shape, dtype=np.uint8 if dtype == np.dtype(bool) else dtype)
    _file_call("lars_h_decode_png_ex" if extended else "lars_h_decode_png_u8", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes)
    return out.view(dtype) if extended else out


def thumbnail_png(data, size=(400, 400), reducing_gap=2.0, extended=False):
    """``np.asarray`` of ``Image.open(io.BytesIO(data))`` after ``.thumbnail(size, LANCZOS, reducing_gap)``, bit for bit
    (process-images.py:186-189), from the file's bytes: the decoded pixels stay on the GPU and go straight into the
    thumbnail kernels, only the thumbnail comes back.  Modes L, RGB and RGBA; others raise ``TypeError`` as ``thumbnail``
    does.  ``draft`` does nothing for PNG, so ``thumbnail_plan(..., draft_box=None)`` is the whole plan; a file that
    already fits comes back as ``decode_png`` gives it.  Errors of the file as ``decode_png``.

    ``extended=True`` takes every file ``decode_png(data, extended=True)`` decodes whose Pillow mode is L, RGB or RGBA: 2- and
    4-bit gray, 16-bit RGB / LA / RGBA, and the interlaced ones.  Modes ``1``, ``I;16``, ``P`` and ``LA`` raise ``TypeError``."""
    arr = _file_bytes(data, "thumbnail_png", "PNG")
    i = _png_check(arr, "thumbnail_png", extended)
    mode = _PNG_MODES[(i.bit_depth, i.color_type)]
    if mode not in ("L", "RGB", "RGBA"):
        raise TypeError(f"thumbnail_png: PNG files in mode L, RGB or RGBA (got mode {mode!r})")
    c = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
    plan = thumbnail_plan((i.width, i.height), size, reducing_gap, None, None, rgba=c == 4)
    if plan is None:
        return decode_png(arr, extended=True) if extended else decode_png(arr)
    return _file_thumbnail("lars_h_thumbnail_png_ex" if extended else "lars_h_thumbnail_png_u8", arr, plan, c)


# ---------------------------------------------------------------------------
# JPEG files decoded on the device
# ---------------------------------------------------------------------------
# why a file is not decoded, by the header's LARS_JPEG_REASON_* names, in the order of their values (tests/test_abi_cpu.py)
_JPEG_REASONS = {"NONE": None, "PROGRESSIVE": "progressive (SOF2)", "FRAME": "lossless, arithmetic-coded or hierarchical frame",
                 "PRECISION": "precision other than 8 bit", "SCANS": "more than one scan", "COMPONENTS": "2 or 4 components (CMYK / YCCK)",
                 "COLORSPACE": "RGB stored as such (no YCbCr transform)", "SAMPLING": "sampling other than 4:4:4, 4:2:2 or 4:2:0",
                 "DNL": "DNL marker", "SIZE": "h * w * channels >= 2^31"}
_JPEG_REASON_TEXT = dict(enumerate(_JPEG_REASONS.values()))
_JPEG_FRAMES = {0xC0: "baseline", 0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless"}


def _jpeg_info(arr):
    info = _ffi.JpegInfo.array()
    _host_query("lars_jpeg_info", _ffi.ptr(arr), arr.size, info)
    return _ffi.JpegInfo(*info)


def jpeg_info(data):
    """The marker segments of a JPEG file, validated on the host (``lars_jpeg_info``; no device needed).

    Returns ``size`` (w, h), ``width``, ``height``, ``components``, ``mode`` (Pillow's: L, RGB or CMYK), ``frame`` (baseline,
    extended sequential, progressive, ...), ``precision``, ``sampling`` ((h, v) per component), ``restart_interval``,
    ``entropy_offset``, ``entropy_bytes``, ``supported`` (what ``decode_jpeg`` decodes) and ``reason`` (``None``, or why not).
    Raises ``ValueError`` for structural damage: no SOI, a segment length that leaves the file, no SOS, SOS before the frame
    header, a missing quantisation or Huffman table, an oversubscribed Huffman table.
    """
    i = _jpeg_info(_file_bytes(data, "jpeg_info", "JPEG"))
    w, h, nc = i.width, i.height, i.components
    return {"size": (w, h), "width": w, "height": h, "components": nc, "mode": {1: "L", 3: "RGB", 4: "CMYK"}.get(nc),
            "frame": _JPEG_FRAMES.get(i.frame, f"SOF{i.frame - 0xC0}"), "precision": i.precision,
            "sampling": i.sampling[:min(nc, 3)], "restart_interval": i.restart_interval, "entropy_offset": i.entropy_offset,
            "entropy_bytes": i.entropy_bytes, "supported": bool(i.supported), "reason": _JPEG_REASON_TEXT.get(i.reason, str(i.reason))}


def _jpeg_check(arr, who):
    i = _jpeg_info(arr)
    if not i.supported:
        raise NotImplementedError(f"{who}: JPEG files with {_JPEG_REASON_TEXT.get(i.reason, i.reason)} are not supported "
                                  "(baseline / extended sequential, 8 bit, one scan, L or YCbCr at 4:4:4, 4:2:2, 4:2:0)")
    return i.height, i.width, i.components


def decode_jpeg(data, scale=1):
    """``np.asarray(Image.open(io.BytesIO(data)))`` of a JPEG file, decoded on the GPU (process-images.py:181-193).

    ``data``: the whole file as ``bytes``, ``bytearray``, ``memoryview`` or a 1-D uint8 array.  Baseline and extended
    sequential Huffman files of 8 bits with one scan: one component (L, ``[H, W]``) or YCbCr at 4:4:4, 4:2:2 or 4:2:0
    (RGB, ``[H, W, 3]``), with or without restart markers; the arithmetic is libjpeg's (``JDCT_ISLOW``, fancy upsampling),
    so the array is Pillow's bit for bit.  EXIF orientation is not applied (``Image.open`` does not either).  Other
    variants (``jpeg_info(data)["reason"]``) raise ``NotImplementedError`` before anything is launched; damaged files raise
    ``ValueError`` saying what is wrong.  Stricter than Pillow on purpose: entropy data that ends early, an invalid code, a
    coefficient past 63 and a missing or misnumbered restart marker are errors.  No CPU fallback.

    ``scale``: 1 (the default: exactly the above), or 2, 4, 8 for libjpeg's decoding at 1/2, 1/4, 1/8 scale -- the array
    ``np.asarray(im)`` gives after ``im.draft(...)`` has set ``im.decoderconfig == (scale, 0)``, bit for bit, of shape
    ``(ceil(H / scale), ceil(W / scale)[, 3])``.  The scaling happens at the coefficients (reduced IDCTs), as in libjpeg.
    Any other value raises ``ValueError``.
    """
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale not in (1, 2, 4, 8):
        raise ValueError(f"decode_jpeg: scale 1, 2, 4 or 8, got {scale!r}")
    arr = _file_bytes(data, "decode_jpeg", "JPEG")
    h, w, c = _jpeg_check(arr, "decode_jpeg")
    scale = int(scale)
    out = np.empty(_shape(-(-h // scale), -(-w // scale), c), dtype=np.uint8)
    if scale == 1:
        _file_call("lars_h_decode_jpeg_u8", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes)
    else:
        _file_call("lars_h_decode_jpeg_scaled_u8", _ffi.ptr(arr), arr.size, scale, _ffi.ptr(out), out.nbytes)
    return out


def thumbnail_jpeg(data, size=(400, 400), reducing_gap=2.0, scaled=False):
    """``np.asarray`` of ``Image.open(io.BytesIO(data))`` after ``.thumbnail(size, LANCZOS, reducing_gap)``, bit for bit
    (process-images.py:186-189), from a JPEG file's bytes: the decoded pixels stay on the GPU and go straight into the
    thumbnail kernels, only the thumbnail comes back.  Pillow's ``thumbnail`` first lets ``draft`` switch the decoder to
    1/2, 1/4 or 1/8 scale where both sides of the image are at least twice ``size * reducing_gap`` (``jpeg_draft_scale``
    above 1).

    ``scaled=False`` (the default): the decoder works at full scale only and raises ``NotImplementedError`` where
    ``jpeg_draft_scale`` is above 1.  ``scaled=True``: there the file is decoded at that scale on the device
    (``decode_jpeg(data, scale)``) and the thumbnail kernels get the plan ``thumbnail_plan`` computes for the scaled
    picture and the box ``draft`` returns, ``(0, 0, w / scale, h / scale)`` -- fractional where the size does not divide;
    when the draft already lands on the final size the scaled decode is the answer.  Where the scale is 1 both settings
    run the same code.  A file that already fits comes back as ``decode_jpeg`` gives it.  Errors of the file as
    ``decode_jpeg``."""
    if not isinstance(scaled, (bool, np.bool_)):
        raise TypeError(f"thumbnail_jpeg: scaled must be True or False, got {scaled!r}")
    arr = _file_bytes(data, "thumbnail_jpeg", "JPEG")
    h, w, c = _jpeg_check(arr, "thumbnail_jpeg")
    if reducing_gap is not None and reducing_gap < 1.0 and thumbnail_size((w, h), size) is not None:
        raise ValueError("reducing_gap must be 1.0 or greater")
    scale = jpeg_draft_scale((w, h), size, reducing_gap)
    if scale != 1 and not scaled:
        raise NotImplementedError(f"thumbnail_jpeg: Pillow's draft() decodes this {w} x {h} file at 1/{scale} scale for size {tuple(size)}; "
                                  "scaled decoding is not supported unless scaled=True is given")
    if scale != 1:
        plan = thumbnail_plan((w, h), size, reducing_gap, (0, 0, w / scale, h / scale), (-(-w // scale), -(-h // scale)))
        if plan is None:
            return decode_jpeg(arr, scale)
        return _file_thumbnail("lars_h_thumbnail_jpeg_scaled_u8", arr, plan, c, scale)
    plan = thumbnail_plan((w, h), size, reducing_gap, None, None)
    if plan is None:
        return decode_jpeg(arr)
    return _file_thumbnail("lars_h_thumbnail_jpeg_u8", arr, plan, c)


# ---------------------------------------------------------------------------
# TIFF files decoded on the device
# ---------------------------------------------------------------------------
# why a file is not decoded, by the header's LARS_TIFF_REASON_* names, in the order of their values (tests/test_tiff_decode_cpu.py)
_TIFF_REASONS = {"NONE": None, "BIGTIFF": "BigTIFF (64-bit offsets)", "BITS": "samples that are not all 8, all 16 or all 32 bits wide",
                 "SAMPLE_FORMAT": "signed samples, floats of 8 or 16 bits or integers of 32", "DEFLATE": "Deflate compression (read_tiff reads it on the host)",
                 "PACKBITS": "PackBits compression", "JPEG": "JPEG compression", "CCITT": "CCITT compression",
                 "COMPRESSION": "an unknown compression scheme", "PREDICTOR": "a predictor other than 1 and 2 (3 goes with float32 samples only)",
                 "OLD_LZW": "old-style (LSB-first) LZW", "SIZE": "2^31 or more decoded bytes"}
_TIFF_REASON_TEXT = dict(enumerate(_TIFF_REASONS.values()))
_TIFF_DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}      # bits == 32 means float32: no other 32-bit kind is supported


def _tiff_info(arr, deflate=False):
    info = _ffi.TiffInfo.array()
    _host_query("lars_tiff_info_deflate" if deflate else "lars_tiff_info", _ffi.ptr(arr), arr.size, info, None, 0)
    return _ffi.TiffInfo(*info)


def tiff_info(data, deflate=False):
    """The first directory of a TIFF file, read on the host by ``tiffio.read_tiff``'s rules (``lars_tiff_info``; no device needed).
    ``deflate=True`` answers for ``decode_tiff(data, deflate=True)`` (``lars_tiff_info_deflate``): a Deflate file is supported,
    every other file reads as without the flag.

    Returns ``width``, ``height``, ``samples``, ``bits``, ``compression``, ``predictor``, ``planar``, ``big_endian``,
    ``photometric`` (-1: no such tag), ``extra_samples``, ``tiled``, ``chunk_w``, ``chunk_h``, ``chunks`` (strips / tiles),
    ``dtype`` and ``shape`` of the array ``decode_tiff`` gives (``None`` where the directory does not say), ``supported`` and
    ``reason`` (``None``, or why the device does not decode it: Deflate, PackBits, JPEG, CCITT, old-style LZW, other bit
    depths, signed samples, BigTIFF, 2^31 bytes or more); ``bits == 32`` is float32.  Raises ``ValueError`` for structural damage: no byte-order
    mark, a directory, a tag's values or a strip / tile outside the file, a missing required tag, a wrong number of strips.
    """
    i = _tiff_info(_file_bytes(data, "tiff_info", "TIFF"), bool(deflate))
    out = i._asdict()
    for k in ("big_endian", "tiled", "supported"):
        out[k] = bool(out[k])
    known = i.bits in _TIFF_DTYPES and i.width > 0 and i.height > 0 and i.samples > 0
    out["dtype"] = np.dtype(_TIFF_DTYPES[i.bits]) if known else None
    out["shape"] = _shape(i.height, i.width, i.samples) if known else None
    out["reason"] = _TIFF_REASON_TEXT.get(i.reason, str(i.reason))
    return out


def _tiff_check(arr, who, deflate=False):
    try:
        i = _tiff_info(arr, deflate)
    except ValueError as e:
        raise TiffError(str(e)) from None
    if not i.supported:
        raise NotImplementedError(f"{who}: TIFF files with {_TIFF_REASON_TEXT.get(i.reason, i.reason)} are not decoded on the device "
                                  "(classic TIFF, 8 or 16 bit unsigned or float32 samples, uncompressed or LZW; Deflate with deflate=True)")
    return i


def decode_tiff(data, deflate=False):
    """``tiffio.read_tiff(data)`` of a TIFF file, decoded on the GPU: the same array bit for bit, dtype and shape included
    (the ``Image.open(io.BytesIO(...))`` of process-images.py:183 for the first accepted extension, at the file's full depth).

    ``data``: the whole file as ``bytes``, ``bytearray``, ``memoryview`` or a 1-D uint8 array.  Classic TIFF, first
    directory, either byte order, 8 or 16 bit unsigned samples, uncompressed or LZW, predictor 1 or 2, chunky or planar,
    strips or tiles: ``[H, W, C]`` (``[H, W]`` for one sample) uint8 or native-endian uint16.  Float32 files (BitsPerSample 32,
    SampleFormat 3) in the same layouts, with predictor 1, 2 or 3 (the floating-point predictor): native float32.  Other variants
    (``tiff_info(data)["reason"]``) raise ``NotImplementedError`` before anything is launched; damaged files raise
    ``tiffio.TiffError`` (a ``ValueError``) where ``read_tiff`` does.  No CPU fallback.

    ``deflate=True``: Deflate files (compression 8, what GDAL's ``COMPRESS=DEFLATE``, tifffile and Pillow's
    ``tiff_adobe_deflate`` write, and 32946) are decoded as well, one zlib stream per strip / tile, refused where zlib
    refuses them for ``read_tiff``: "corrupt Deflate data", "inflates past its N bytes", "holds N bytes, M expected", for
    the first such strip / tile of the file.  One lane decodes a strip's symbols, so the gain comes from the number of
    strips / tiles: a file written as one huge strip gains nothing and may lose against zlib on the host.  The default is
    unchanged: without the flag a Deflate file raises ``NotImplementedError``.
    """
    arr = _file_bytes(data, "decode_tiff", "TIFF")
    deflate = bool(deflate)
    i = _tiff_check(arr, "decode_tiff", deflate)
    out = np.empty(_shape(i.height, i.width, i.samples), dtype=_TIFF_DTYPES[i.bits])
    _file_call("lars_h_decode_tiff_deflate" if deflate else "lars_h_decode_tiff", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes,
               error=TiffError)
    return out


def _tiff_is_pillow_u8(i):
    """8-bit files Pillow opens as mode L or RGB with the samples as stored: one BlackIsZero sample, or RGB, no extra samples."""
    return i.bits == 8 and i.extra_samples == 0 and ((i.samples == 1 and i.photometric == 1) or (i.samples == 3 and i.photometric == 2))


def thumbnail_tiff(data, size=(400, 400), reducing_gap=2.0, deflate=False):
    """``np.asarray`` of ``Image.open(io.BytesIO(data))`` after ``.thumbnail(size, LANCZOS, reducing_gap)``, bit for bit
    (process-images.py:186-189), from a TIFF file's bytes: the decoded pixels stay on the GPU and go straight into the
    thumbnail kernels, only the thumbnail comes back.  8-bit files with one sample (BlackIsZero) or three (RGB) and no
    extra samples; others raise ``TypeError``.  ``draft`` does nothing for TIFF, so ``thumbnail_plan(..., draft_box=None)``
    is the whole plan; a file that already fits comes back as ``decode_tiff`` gives it.  Errors of the file as ``decode_tiff``.
    ``deflate=True``: Deflate files too, as in ``decode_tiff``."""
    arr = _file_bytes(data, "thumbnail_tiff", "TIFF")
    deflate = bool(deflate)
    i = _tiff_check(arr, "thumbnail_tiff", deflate)
    if not _tiff_is_pillow_u8(i):
        raise TypeError(f"thumbnail_tiff: 8-bit TIFF files in mode L or RGB (got {i.samples} samples of {i.bits} bits, "
                        f"photometric {i.photometric}, {i.extra_samples} extra samples)")
    plan = thumbnail_plan((i.width, i.height), size, reducing_gap, None, None)
    if plan is None:
        return decode_tiff(arr, deflate=True) if deflate else decode_tiff(arr)
    return _file_thumbnail("lars_h_thumbnail_tiff_deflate_u8" if deflate else "lars_h_thumbnail_tiff_u8", arr, plan, i.samples, error=TiffError)
