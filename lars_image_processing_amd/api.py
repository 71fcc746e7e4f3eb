"""The reference's function signatures, served by the HIP library.

Same names, positional arguments, return types and error behaviour as
lars-uav/lars-image-processing, so its callers (Streamlit front-end, MongoDB
I/O, batch script) keep working unchanged:

==============================  ============================================
this module                     reference
==============================  ============================================
``fix_white_balance(arr)``      process-images.py:424  (ndarray -> uint8 ndarray)
``fix_white_balance(pil)``      backend-process.py:17  (PIL.Image -> PIL.Image)
``fix_white_balance_rgnir``     process-rgn.py:4       (path in, array / file out)
``calculate_index(arr, t)``     process-images.py:449
``calculate_index(r, g, n, t)`` backend-process.py:28
``calculate_ndvi(path, ...)``   process-ndvi.py:5      (float64)
``analyze_index(idx, t)``       process-images.py:492
``analyze_ndvi_statistics``     process-ndvi.py:50
``preprocess_large_image``      process-images.py:398  (Pillow LANCZOS down-scale)
``thumbnail``                   process-images.py:186  (Pillow LANCZOS gallery thumbnail; a new object, not in place)
``encode_png``                  backend-process.py:70, process-images.py:567-617 (``Image.fromarray(x).save(png)``: same pixels)
``decode_png``                  process-images.py:181-193 (``np.array(Image.open(io.BytesIO(img_bytes)))``: same array)
``thumbnail_png``               process-images.py:186-189 from the file's bytes (decode + thumbnail, pixels stay on the GPU)
``encode_jpeg``                 process-rgn.py:47 with :72-73, process-images.py:247 (``img.save(f, "JPEG")``: the same file, byte for byte)
``decode_jpeg``                 process-images.py:181-193, backend-process.py:52 for JPEG files (same array as Pillow's; ``scale=2, 4, 8``: after ``draft``)
``thumbnail_jpeg``              process-images.py:186-189 from a JPEG file's bytes (``scaled=True``: also where ``draft`` decodes at 1/2, 1/4, 1/8)
``align_images``                process-images.py:515  (phase correlation + shift)
``calculate_index_statistics_by_timeframe``  process-images.py:619 (pandas table)
``time_series_points``          process-images.py:814-832 (the numbers ``create_time_series_plot`` draws)
``change_detection``            process-images.py:885-923, :956 (the arrays ``create_change_detection_visualization`` draws)
``download_processed_images``   process-images.py:567  (ZIP of the processed images, per-pixel colormaps)
``generate_ndvi_report``        process-ndvi.py:75     (NDVI image + histogram counts + statistics file; BASELINE configs[0])
==============================  ============================================

Figure rendering (matplotlib: ``create_time_series_plot``, ``create_change_detection_visualization``,
``create_index_visualization``, ``create_comparison_view``, the pictures inside ``calculate_ndvi`` /
``generate_ndvi_report``) is NOT part of this package (out of scope).  The
reference's own figure functions keep working on top of the functions here -- INTEGRATION.md section 1 shows the
import swap -- and this module only hands them their numbers.  Nothing under this package imports matplotlib.

``correct_white_balance`` and ``analyze_index_statistics`` are aliases (the
spellings BASELINE.json uses).  Inputs are never modified; outputs are fresh
host ndarrays owned by the caller.  All arithmetic runs on the GPU through
``liblars_hip.so``; there is no NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple

import numpy as np

from . import _ffi
from ._ffi import INDEX_IDS, INDEX_NAMES, Stats
from .batch import index_mask
from .hostpool import empty as _empty        # large result arrays reuse released buffers (no first-touch page faults)

__all__ = [
    "fix_white_balance", "correct_white_balance", "fix_white_balance_rgnir",
    "calculate_index", "calculate_ndvi", "analyze_index", "analyze_index_statistics",
    "analyze_ndvi_statistics", "index_histogram", "classification_mask", "colorize_index", "process_image",
    "timeseries_row", "colormap_lut", "preprocess_large_image", "thumbnail", "thumbnail_plan", "encode_png", "encode_tiff_f32", "tiff_f32_bound",
    "png_info", "decode_png", "thumbnail_png", "jpeg_info", "decode_jpeg", "encode_jpeg", "thumbnail_jpeg", "jpeg_draft_scale", "align_images", "change_detection",
    "colorize_difference", "calculate_index_statistics_by_timeframe", "time_series_points",
    "calculate_ndvi_array", "generate_ndvi_report", "download_processed_images",
    "create_index_visualization", "create_comparison_view", "create_time_series_plot", "create_change_detection_visualization",
]

_CMAPS = None


def colormap_lut(name):
    """256x4 uint8 table of a matplotlib colormap (RdYlGn, RdYlBu, bwr).

    ``(cmap._lut[:256] * 255).astype(uint8)`` of matplotlib 3.10.8, shipped as
    data so that the compute path does not import matplotlib.
    """
    global _CMAPS
    if _CMAPS is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "colormaps.npz")
        with np.load(path, allow_pickle=False) as z:
            _CMAPS = {k: np.ascontiguousarray(z[k]) for k in z.files}
    return _CMAPS[name]


def _colormap_for(index_type):
    # process-images.py:690-693, backend-process.py:42
    return "RdYlBu" if index_type == "NDWI" else "RdYlGn"


def _is_pil(obj):
    return hasattr(obj, "getbands") and hasattr(obj, "convert")


def _as_image(img_array, what):
    """Validate an [H, W, C>=3] integer image and make it C-contiguous."""
    arr = np.asarray(img_array)
    if arr.ndim != 3:
        # the reference indexes [:, :, i] and fails the same way on 2-D input
        raise IndexError(f"too many indices for array: array is {arr.ndim}-dimensional, but 3 were indexed")
    if arr.shape[2] < 3:
        raise IndexError(f"index 2 is out of bounds for axis 2 with size {arr.shape[2]}")
    return np.ascontiguousarray(arr)


# ---------------------------------------------------------------------------
# down-scale in front of the path
# ---------------------------------------------------------------------------
def preprocess_large_image(img_array, max_dimension=1024):
    """process-images.py:398-422: LANCZOS down-scale to ``max_dimension`` on the long edge.

    ``None``/empty -> ``None``; an image that already fits is returned as is (the same object,
    as upstream); otherwise Pillow's ``resize((new_w, new_h), LANCZOS)``, bit for bit, on the GPU
    (uint8 images with 1, 3 or 4 channels; 4 = RGBA through premultiplied alpha, as Pillow does).
    """
    if img_array is None or np.size(img_array) == 0:
        return None
    h, w = img_array.shape[:2]
    if max(h, w) <= max_dimension:
        return img_array
    if h > w:
        new_h = max_dimension
        new_w = int(w * (max_dimension / h))
    else:
        new_w = max_dimension
        new_h = int(h * (max_dimension / w))
    arr = np.ascontiguousarray(img_array)
    if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in (1, 3, 4)):
        raise TypeError(f"preprocess_large_image: uint8 images with 1, 3 or 4 channels (got {arr.dtype}, shape {arr.shape})")
    c = 1 if arr.ndim == 2 else arr.shape[2]
    out = np.empty((new_h, new_w) if arr.ndim == 2 else (new_h, new_w, c), dtype=np.uint8)
    _ffi.call("lars_h_resize_lanczos_u8", _ffi.ptr(arr), h, w, c, new_h, new_w, _ffi.ptr(out))
    return out


# ---------------------------------------------------------------------------
# gallery thumbnails
# ---------------------------------------------------------------------------
_LANCZOS_SUPPORT = 3.0                      # Image._filters_support[LANCZOS]
_THUMB_MODES = {"L": 1, "RGB": 3, "RGBA": 4}
_THUMB_CHANNELS = {1: "L", 3: "RGB", 4: "RGBA"}


class ThumbnailPlan(NamedTuple):
    """What ``Image.thumbnail(size, LANCZOS, reducing_gap)`` does to the decoded pixels (``thumbnail_plan``)."""
    size: tuple            # (w, h) of the thumbnail
    factor: tuple          # (fx, fy) of Image.reduce; (1, 1) = no reduce
    reduce_box: tuple      # (x0, y0, x1, y1) of the decoded image the reduce reads (_get_safe_box), or the whole image
    box: tuple             # (x0, y0, x1, y1) of the LANCZOS passes in the reduced image, rounded to float32 as Pillow's C code holds it
    vertical_first: bool   # Image.resize's tall-image branch: the vertical pass runs before the horizontal one
    premultiply: bool      # RGBA: resampled as RGBa, without the reduce


def thumbnail_size(src_size, size):
    """``preserve_aspect_ratio`` of ``Image.thumbnail``: the (w, h) a (w, h) source becomes, ``None`` if it already fits."""
    x, y = (math.floor(v) for v in size)
    width, height = src_size
    if x >= width and y >= height:
        return None

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def thumbnail_plan(src_size, size=(400, 400), reducing_gap=2.0, draft_box=None, image_size=None, rgba=False):
    """Pillow 12's ``Image.thumbnail(size, LANCZOS, reducing_gap)`` policy as numbers; no GPU involved.

    ``src_size`` is the (w, h) the caller sees before ``draft``, ``image_size`` the (w, h) of the decoded pixels
    (after ``draft``; default ``src_size``) and ``draft_box`` the box ``draft`` returned (``None``: the whole image).
    Returns ``None`` where Pillow leaves the image alone, else a ``ThumbnailPlan``.  Raises ``ValueError`` for a
    ``reducing_gap`` below 1.0 where Pillow would resize.  The only place these rules live: ``thumbnail`` and the C
    entry point ``lars_h_thumbnail_u8`` take its numbers as they are.
    """
    final = thumbnail_size(src_size, size)
    if final is None:
        return None
    w, h = image_size if image_size is not None else src_size
    if (w, h) == final:                                   # thumbnail: `if self.size != final_size`
        return None
    if reducing_gap is not None and reducing_gap < 1.0:
        raise ValueError("reducing_gap must be 1.0 or greater")
    box = (0, 0, w, h) if draft_box is None else tuple(draft_box)
    factor, reduce_box = (1, 1), (0, 0, w, h)
    # resize(): RGBA converts to RGBa and resizes again without reducing_gap
    if reducing_gap is not None and not rgba:
        fx = int((box[2] - box[0]) / final[0] / reducing_gap) or 1
        fy = int((box[3] - box[1]) / final[1] / reducing_gap) or 1
        if fx > 1 or fy > 1:
            # _get_safe_box
            filter_support = _LANCZOS_SUPPORT - 0.5
            support_x = filter_support * ((box[2] - box[0]) / final[0])
            support_y = filter_support * ((box[3] - box[1]) / final[1])
            reduce_box = (max(0, int(box[0] - support_x)), max(0, int(box[1] - support_y)),
                          min(w, math.ceil(box[2] + support_x)), min(h, math.ceil(box[3] + support_y)))
            factor = (fx, fy)
            box = ((box[0] - reduce_box[0]) / fx, (box[1] - reduce_box[1]) / fy,
                   (box[2] - reduce_box[0]) / fx, (box[3] - reduce_box[1]) / fy)
            w = -(-(reduce_box[2] - reduce_box[0]) // fx)
            h = -(-(reduce_box[3] - reduce_box[1]) // fy)
    return ThumbnailPlan(size=final, factor=factor, reduce_box=reduce_box,
                         box=tuple(float(np.float32(v)) for v in box),
                         vertical_first=h > w * 100 and final[1] < h, premultiply=rgba)


def jpeg_draft_scale(src_size, size=(400, 400), reducing_gap=2.0):
    """The scale (1, 2, 4 or 8) ``Image.thumbnail(size, ..., reducing_gap)`` makes the JPEG *decoder* work at, through
    ``JpegImageFile.draft(None, (int(size[0] * reducing_gap), int(size[1] * reducing_gap)))``: the largest of 8, 4, 2, 1 not
    above ``min(w // requested_w, h // requested_h)``.  1 when the image already fits (``thumbnail`` returns before ``draft``)
    or ``reducing_gap`` is ``None``.  No GPU involved."""
    if reducing_gap is None or thumbnail_size(src_size, size) is None:
        return 1
    req = (int(size[0] * reducing_gap), int(size[1] * reducing_gap))
    scale = min(src_size[0] // req[0], src_size[1] // req[1])
    for s in (8, 4, 2, 1):
        if scale >= s:
            break
    return s


def thumbnail(image, size=(400, 400), reducing_gap=2.0):
    """``img.thumbnail(size, Image.Resampling.LANCZOS, reducing_gap)`` (process-images.py:186-189), bit for bit, on the GPU.

    ``image``: a PIL image in mode L, RGB or RGBA, or a uint8 ndarray [H, W], [H, W, 3] or [H, W, 4] (the same three
    modes).  Returns a NEW object of the same kind -- unlike Pillow, which changes the image in place -- or ``image``
    itself, without touching the GPU, where Pillow would leave the image as it is.  A JPEG-backed PIL image is
    ``draft``-ed first exactly as Pillow does (this changes the caller's image object, as Pillow's call does); decoding
    stays Pillow's.  Other modes raise ``TypeError``: there is no CPU fallback.
    """
    pil = _is_pil(image)
    if pil:
        mode = image.mode
        if mode not in _THUMB_MODES:
            raise TypeError(f"thumbnail: PIL images in mode L, RGB or RGBA (got mode {mode!r})")
        src_size = image.size
    else:
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or not (arr.ndim == 2 or (arr.ndim == 3 and arr.shape[2] in (3, 4))):
            raise TypeError(f"thumbnail: uint8 arrays [H, W], [H, W, 3] or [H, W, 4] (got {arr.dtype}, shape {arr.shape})")
        mode = _THUMB_CHANNELS[1 if arr.ndim == 2 else arr.shape[2]]
        src_size = (arr.shape[1], arr.shape[0])
    if thumbnail_size(src_size, size) is None:
        return image
    draft_box = None
    if pil:
        if reducing_gap is not None:
            res = image.draft(None, (int(size[0] * reducing_gap), int(size[1] * reducing_gap)))
            if res is not None:
                draft_box = res[1]
        arr = np.asarray(image)
        if image.mode != mode:
            raise TypeError(f"thumbnail: the decoder turned mode {mode!r} into {image.mode!r}")
    plan = thumbnail_plan(src_size, size, reducing_gap, draft_box, (arr.shape[1], arr.shape[0]), rgba=mode == "RGBA")
    if plan is None:
        return image
    arr = np.ascontiguousarray(arr)
    h, w = arr.shape[:2]
    c = _THUMB_MODES[mode]
    new_w, new_h = plan.size
    out = np.empty((new_h, new_w) if c == 1 else (new_h, new_w, c), dtype=np.uint8)
    _ffi.call("lars_h_thumbnail_u8", _ffi.ptr(arr), h, w, c, plan.factor[0], plan.factor[1], (C.c_int * 4)(*plan.reduce_box),
              (C.c_float * 4)(*plan.box), new_h, new_w, int(plan.vertical_first), _ffi.ptr(out))
    if pil:
        from PIL import Image
        return Image.fromarray(out)
    return out


# ---------------------------------------------------------------------------
# white balance
# ---------------------------------------------------------------------------
def _wb_array(arr, variant=0, want_percentiles=False):
    code = _ffi.dtype_code(arr.dtype)
    h, w, c = arr.shape
    out = _empty((h, w, c), dtype=np.uint8)
    pcts = np.empty((3, 2), dtype=np.float64) if want_percentiles else None
    if code is None:
        # any other sample type (float, wider or signed integers, bool): the reference's first line is
        # `img_array.astype(np.float32)` (process-images.py:431); everything after that cast runs on the device
        if variant != 0:
            raise TypeError(f"fix_white_balance_rgnir: unsupported sample type {arr.dtype} (image files decode to uint8 / uint16)")
        if arr.dtype.kind not in "fiub":
            raise TypeError(f"fix_white_balance: samples of type {arr.dtype} cannot be cast to float32")
        as_f32 = np.ascontiguousarray(arr.astype(np.float32))
        _ffi.call("lars_h_fix_white_balance_f32", _ffi.ptr(as_f32), h, w, c, _ffi.ptr(out), _ffi.ptr(pcts))
    else:
        _ffi.call("lars_h_fix_white_balance", _ffi.ptr(arr), h, w, c, code, variant, _ffi.ptr(out), _ffi.ptr(pcts))
    return (out, pcts) if want_percentiles else out


def fix_white_balance(img_array):
    """Percentile (2, 98) white balance of an RGNir image.

    ndarray in -> uint8 ndarray out, channels >= 3 zeroed, ``None``/empty ->
    ``None`` (process-images.py:424-447).  PIL.Image in -> PIL.Image out
    (backend-process.py:17-26).
    """
    if _is_pil(img_array):
        from PIL import Image
        return Image.fromarray(fix_white_balance(np.array(img_array)))
    if img_array is None or np.size(img_array) == 0:
        return None
    return _wb_array(_as_image(img_array, "fix_white_balance"))


correct_white_balance = fix_white_balance


def fix_white_balance_rgnir(image_path, save_path=None, jpeg_encoder="pillow"):
    """process-rgn.py:4-49: file in; array out, or file out when ``save_path`` is given.

    ``jpeg_encoder="device"`` writes a ``save_path`` ending in ``.jpg`` / ``.jpeg`` with ``encode_jpeg`` (the GPU): byte
    for byte the file Pillow would have written.  Every other file, and the default, go through Pillow."""
    from PIL import Image
    if jpeg_encoder not in ("pillow", "device"):
        raise ValueError(f"jpeg_encoder must be 'pillow' or 'device', got {jpeg_encoder!r}")
    arr = _as_image(np.array(Image.open(image_path)), "fix_white_balance_rgnir")
    corrected = _wb_array(arr, variant=1)
    corrected = np.ascontiguousarray(corrected[:, :, :3])        # np.dstack of three planes (:41)
    if save_path:
        if jpeg_encoder == "device" and os.fspath(save_path).lower().endswith((".jpg", ".jpeg")):
            with open(save_path, "wb") as f:
                f.write(encode_jpeg(corrected))
        else:
            Image.fromarray(corrected).save(save_path)
        return None
    return corrected


# ---------------------------------------------------------------------------
# indices
# ---------------------------------------------------------------------------
def _index_from_planes(red, green, nir, index_type):
    shape = np.shape(nir)
    planes = [np.ascontiguousarray(p, dtype=np.float32) for p in (red, green, nir)]
    n = planes[2].size
    out = _empty(shape, dtype=np.float32)
    _ffi.call("lars_h_calculate_index_planes", _ffi.ptr(planes[0]), _ffi.ptr(planes[1]), _ffi.ptr(planes[2]),
              n, INDEX_IDS[index_type], _ffi.ptr(out))
    return out


def calculate_index(*args):
    """``calculate_index(img_array, index_type)`` (process-images.py:449-490) or
    ``calculate_index(red, green, nir, index_type)`` (backend-process.py:28-38).

    float32 ``(a-b)/(a+b+1e-10)`` clipped to [-1, 1]; ``None``/empty -> ``None``;
    unknown type -> ``ValueError`` (2-arg) / ``UnboundLocalError`` (4-arg), as upstream.
    """
    if len(args) == 4:
        red, green, nir, index_type = args
        if index_type not in INDEX_IDS:
            raise UnboundLocalError("local variable 'index' referenced before assignment")
        return _index_from_planes(red, green, nir, index_type)
    if len(args) != 2:
        raise TypeError("calculate_index(img_array, index_type) or calculate_index(red, green, nir, index_type)")
    img_array, index_type = args
    if img_array is None or np.size(img_array) == 0:
        return None
    arr = _as_image(img_array, "calculate_index")
    if index_type not in INDEX_IDS:
        raise ValueError(f"Unknown index type: {index_type}")
    code = _ffi.dtype_code(arr.dtype)
    if code is None:
        # any other sample type: the reference casts to float32 first (:456)
        f = arr.astype(np.float32)
        return _index_from_planes(f[:, :, 0], f[:, :, 1], f[:, :, 2], index_type)
    h, w, c = arr.shape
    k = INDEX_IDS[index_type]
    out = _empty((h, w), dtype=np.float32)
    outs = [None, None, None]
    outs[k] = out
    p3 = _ffi.ptr3(outs)
    _ffi.call("lars_h_calculate_index", _ffi.ptr(arr), h, w, c, code, 1 << k, C.byref(p3), None, 0)
    return out


def calculate_ndvi_array(img_array):
    """The arithmetic of process-ndvi.py:18-31 on an array: float64 ``(nir - red) / (nir + red + 1e-10)`` clipped to
    [-1, 1] of an ``[H, W, C >= 3]`` uint8 / uint16 image (``astype(float)`` is exact for both)."""
    arr = _as_image(img_array, "calculate_ndvi")
    code = _ffi.dtype_code(arr.dtype)
    if code is None:
        raise TypeError(f"calculate_ndvi: unsupported sample type {arr.dtype}")
    h, w, c = arr.shape
    ndvi = _empty((h, w), dtype=np.float64)
    _ffi.call("lars_h_ndvi_f64", _ffi.ptr(arr), h, w, c, code, _ffi.ptr(ndvi))
    return ndvi


def calculate_ndvi(image_path, save_path=None, visualize=True):
    """process-ndvi.py:5-48: float64 NDVI of an image file.

    The reference also draws a matplotlib figure (``:33-46``); figure rendering is out of scope here.  With
    ``save_path`` this function writes the per-pixel RdYlGn image of the NDVI instead (the colormap of ``:38`` applied
    pixel by pixel on the GPU, full resolution, no axes or colorbar); ``visualize`` is accepted and ignored (upstream:
    ``plt.show()``).  A caller that wants the reference's figure keeps the reference's ``calculate_ndvi`` and lets it
    call ``calculate_ndvi_array`` for lines 18-31.
    """
    from PIL import Image
    ndvi = calculate_ndvi_array(np.array(Image.open(image_path)))
    if save_path:
        Image.fromarray(colorize_index(ndvi.astype(np.float32), "NDVI"), "RGBA").save(save_path)
    return ndvi


# ---------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------
def _coverage_rule(index_type):
    # process-images.py:498-504
    return ("Water", 0.0) if index_type == "NDWI" else ("Vegetation", 0.2)


def _analyze_array(index_array, threshold, want_hist=False, want_std=False):
    """-> (Stats, median, sumsqdev) of a float32 / float64 array via the library."""
    arr = np.asarray(index_array)
    if arr.dtype == np.float32:
        flat = np.ascontiguousarray(arr).reshape(-1)
        st, med = Stats(), np.empty(2, dtype=np.float32)
        _ffi.call("lars_h_analyze_f32", _ffi.ptr(flat), flat.size, np.float32(threshold), int(want_hist),
                  C.byref(st), _ffi.ptr(med))
        median = float(np.float32(np.float32(med[0] + med[1]) / 2))   # mean of the two middles in float32
        return st, median, None
    flat = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1)
    st, med, ssd = Stats(), np.empty(2, dtype=np.float64), C.c_double(0.0)
    _ffi.call("lars_h_analyze_f64", _ffi.ptr(flat), flat.size, float(threshold), int(want_hist), C.byref(st),
              _ffi.ptr(med), C.byref(ssd) if want_std else None)
    return st, float((med[0] + med[1]) / 2), ssd.value


def _summary(st, median):
    """mean / median / min / max / coverage from a Stats record (NumPy NaN rules)."""
    if st.nans:
        nan = float("nan")
        return nan, nan, nan, nan, st.above / st.count * 100
    return st.sum / st.count, median, st.min, st.max, st.above / st.count * 100


def analyze_index(index_array, index_type):
    """process-images.py:492-513: dict with exactly the upstream keys.

    ``Mean`` is the exact sum of the samples divided by their count (the
    reference's float32 pairwise sum differs from it by ~1e-7 relative);
    median / min / max / coverage are exact.
    """
    if index_array is None or np.size(index_array) == 0:
        return {}
    feature_name, threshold = _coverage_rule(index_type)
    st, median, _ = _analyze_array(index_array, threshold)
    mean, median, mn, mx, cover = _summary(st, median)
    return {
        f"Mean {index_type}": float(mean),
        f"Median {index_type}": float(median),
        f"Min {index_type}": float(mn),
        f"Max {index_type}": float(mx),
        f"{feature_name} Coverage (%)": float(cover),
    }


analyze_index_statistics = analyze_index


def timeseries_row(index_array, index_type, date):
    """process-images.py:646-658: the inlined statistics row of the time-series table."""
    feature_name, threshold = _coverage_rule(index_type)
    st, median, _ = _analyze_array(index_array, threshold)
    mean, median, mn, mx, cover = _summary(st, median)
    return {"Date": date, "Mean": float(mean), "Median": float(median), "Min": float(mn), "Max": float(mx),
            f"{feature_name} Coverage (%)": float(cover)}


def analyze_ndvi_statistics(ndvi_array):
    """process-ndvi.py:50-73 (float64 flavour, with population std)."""
    arr = np.asarray(ndvi_array)
    st, median, ssd = _analyze_array(arr, 0.2, want_std=True)
    mean, median, mn, mx, cover = _summary(st, median)
    if arr.dtype == np.float32:
        # np.std of a float32 array: same two-pass definition
        st64, _, ssd = _analyze_array(arr.astype(np.float64), 0.2, want_std=True)
    std = float("nan") if st.nans else math.sqrt(ssd / st.count)
    return {
        "mean_ndvi": float(mean),
        "median_ndvi": float(median),
        "min_ndvi": float(mn),
        "max_ndvi": float(mx),
        "std_ndvi": float(std),
        "vegetation_coverage": float(cover),
    }


def classification_mask(index_array, index_type):
    """uint8 mask of ``index_array > threshold`` (1 = vegetation, or water for NDWI): the array the reference
    averages for its coverage figures (process-images.py:498-511), compared in float32 like NumPy does."""
    if index_array is None or np.size(index_array) == 0:
        return None
    arr = np.ascontiguousarray(index_array, dtype=np.float32)
    _, threshold = _coverage_rule(index_type)
    out = _empty(arr.shape, dtype=np.uint8)
    _ffi.call("lars_h_threshold_mask_f32", _ffi.ptr(arr.reshape(-1)), arr.size, float(threshold), _ffi.ptr(out))
    return out


def index_histogram(index_array):
    """Counts of ``plt.hist(x.flatten(), bins=50, range=(-1, 1))`` (process-ndvi.py:97)."""
    st, _, _ = _analyze_array(index_array, 0.0, want_hist=True)
    return np.array(list(st.hist), dtype=np.int64)


# ---------------------------------------------------------------------------
# colormap + one-upload pipeline
# ---------------------------------------------------------------------------
def colorize_index(index_array, index_type):
    """Per-pixel RGBA8 of ``imshow(index, cmap, vmin=-1, vmax=1)`` (process-images.py:690-695)."""
    arr = np.ascontiguousarray(index_array, dtype=np.float32)
    lut = colormap_lut(_colormap_for(index_type))
    out = _empty(arr.shape + (4,), dtype=np.uint8)
    _ffi.call("lars_h_colormap_f32", _ffi.ptr(arr.reshape(-1)), arr.size, _ffi.ptr(lut), _ffi.ptr(out))
    return out


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
    out = np.empty(png_bound(h, w, c), dtype=np.uint8)
    n = C.c_int64(0)
    _ffi.call("lars_h_encode_png_u8", _ffi.ptr(arr), h, w, c, _ffi.ptr(pal), npal, _ffi.ptr(out), out.nbytes, C.byref(n))
    return out[:n.value].tobytes()


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
    out = np.empty(jpeg_bound(h, w, c, sub), dtype=np.uint8)
    n = C.c_int64(0)
    _ffi.call("lars_h_encode_jpeg_u8", _ffi.ptr(arr), h, w, c, int(quality), sub, _ffi.ptr(out), out.nbytes, C.byref(n))
    return out[:n.value].tobytes()


# ---------------------------------------------------------------------------
# TIFF files built on the device
# ---------------------------------------------------------------------------
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
    name = "lars_tiff_deflate_bound" if _tiff_compression(compression, "tiff_bound") else "lars_tiff_bound"
    return int(getattr(_ffi.load(), name)(int(h), int(w), int(channels), int(itemsize), int(rows_per_strip or 0)))


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
    from .tiffio import TiffError
    deflate = _tiff_compression(compression, "encode_tiff")
    arr, rps = _tiff_picture(array, rows_per_strip, "encode_tiff")
    h, w, c = arr.shape
    bound = tiff_bound(h, w, c, arr.dtype.itemsize, rps, compression)
    if bound == 0:
        raise ValueError(f"encode_tiff: strips of {rps or 'the default number of'} rows of {w * c * arr.dtype.itemsize} bytes are too long (2^30 bytes at most)")
    out = np.empty(min(bound, 1 << 32), dtype=np.uint8)
    n = C.c_int64(0)
    try:
        _ffi.call("lars_h_encode_tiff_deflate" if deflate else "lars_h_encode_tiff", _ffi.ptr(arr), h, w, c, arr.dtype.itemsize, rps,
                  int(bool(predictor)), _ffi.ptr(out), out.nbytes, C.byref(n))
    except _ffi.LarsError as e:
        if e.code == -6 or (e.code == -1 and bound > out.nbytes):
            raise TiffError("image too large for a classic TIFF (4 GiB)") from None
        raise
    return out[:n.value].tobytes()


def tiff_f32_bound(h, w, channels, rows_per_strip=None, compression="lzw"):
    """The largest file ``encode_tiff_f32`` can return for an ``h x w`` picture of ``channels`` float32 samples
    (``lars_tiff_f32_bound``; host code, no device needed); 0 for a shape that cannot be encoded.  ``tiff_bound``'s derivation
    with rows of ``w * channels * 4`` bytes: per strip of n bytes ``ceil(12 * (n + n // 3836 + 2) / 8)`` bytes, plus one where
    that is odd; 8 bytes of header, 2 + 12 * 13 + 4 of directory, ``4 * channels`` of BitsPerSample and SampleFormat, 8 per
    strip.  ``rows_per_strip=None``: the rows the knob ``tiff_strip_bytes`` gives.  ``compression="deflate"``
    (``lars_tiff_float32_deflate_bound``): ``n + 5 * ceil(n / 32768) + 6`` bytes per strip, plus one where that is odd, as in
    ``tiff_bound``."""
    name = "lars_tiff_float32_deflate_bound" if _tiff_compression(compression, "tiff_f32_bound") else "lars_tiff_f32_bound"
    return int(getattr(_ffi.load(), name)(int(h), int(w), int(channels), int(rows_per_strip or 0)))


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
    from .tiffio import TiffError
    deflate = _tiff_compression(compression, "encode_tiff_f32")
    arr, rps = _tiff_picture(array, rows_per_strip, "encode_tiff_f32", f32=True)
    h, w, c = arr.shape
    bound = tiff_f32_bound(h, w, c, rps, compression)
    if bound == 0:
        raise ValueError(f"encode_tiff_f32: strips of {rps or 'the default number of'} rows of {w * c * 4} bytes are too long (2^30 bytes at most)")
    out = np.empty(min(bound, 1 << 32), dtype=np.uint8)
    n = C.c_int64(0)
    try:
        _ffi.call("lars_h_encode_tiff_deflate_float32" if deflate else "lars_h_encode_tiff_f32", _ffi.ptr(arr), h, w, c, rps, int(bool(predictor)),
                  _ffi.ptr(out), out.nbytes, C.byref(n))
    except _ffi.LarsError as e:
        if e.code == -6 or (e.code == -1 and bound > out.nbytes):
            raise TiffError("image too large for a classic TIFF (4 GiB)") from None
        raise
    return out[:n.value].tobytes()


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


def _file_call(name, *args):
    """``_ffi.call`` of a decoder: LARS_ERR_INVALID there speaks of the file's contents and becomes ``ValueError``."""
    try:
        _ffi.call(name, *args)
    except _ffi.LarsError as e:
        if e.code == -1:
            raise ValueError(str(e)) from None
        raise


def _file_thumbnail(name, arr, plan, c):
    """The call both ``thumbnail_png`` and ``thumbnail_jpeg`` end in: ``plan`` applied to the decoded file on the device."""
    new_w, new_h = plan.size
    out = np.empty((new_h, new_w) if c == 1 else (new_h, new_w, c), dtype=np.uint8)
    _file_call(name, _ffi.ptr(arr), arr.size, plan.factor[0], plan.factor[1], (C.c_int * 4)(*plan.reduce_box),
               (C.c_float * 4)(*plan.box), new_h, new_w, int(plan.vertical_first), _ffi.ptr(out))
    return out


def _png_info(arr):
    lib = _ffi.load()
    info = _ffi.PngInfo.array()
    if lib.lars_png_info(_ffi.ptr(arr), arr.size, info, None, 0) != 0:
        raise ValueError(lib.lars_last_error().decode("utf-8", "replace"))
    return _ffi.PngInfo(*info)


def _png_out_format(i):
    """``(dtype, shape)`` of the array the extended decoder gives for the IHDR numbers ``i`` (``lars_png_out_format``, pure
    host code): Pillow's ``np.asarray`` of the file."""
    channels, itemsize = C.c_int(0), C.c_int(0)
    lib = _ffi.load()
    if lib.lars_png_out_format(i.bit_depth, i.color_type, C.byref(channels), C.byref(itemsize)) != 0:
        raise ValueError(lib.lars_last_error().decode("utf-8", "replace"))
    dtype = np.dtype(np.uint16) if itemsize.value == 2 else np.dtype(bool) if (i.bit_depth, i.color_type) == (1, 0) else np.dtype(np.uint8)
    return dtype, (i.height, i.width) if channels.value == 1 else (i.height, i.width, channels.value)


def _png_need(i):
    """Filtered bytes of all passes (``lars_png_layout``, pure host code)."""
    passes = (C.c_int64 * 70)()
    npass, need = C.c_int64(0), C.c_int64(0)
    lib = _ffi.load()
    if lib.lars_png_layout(i.width, i.height, i.bit_depth, i.color_type, i.interlace, passes, C.byref(npass), C.byref(need)) != 0:
        raise ValueError(lib.lars_last_error().decode("utf-8", "replace"))
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
    i = _png_info(arr)
    w, h, ctype, channels = i.width, i.height, i.color_type, i.channels
    if extended:
        if i.apng:
            raise NotImplementedError(f"{who}: APNG PNG files are not supported")
        if not (1 <= h <= 1 << 24 and 1 <= w <= 1 << 24) or _png_need(i) > (1 << 31) - 1:
            raise ValueError(f"{who}: {w} x {h} picture of {channels} channels at bit depth {i.bit_depth} is too large")
        return i
    if not i.supported:
        what = "APNG" if i.apng else "interlaced" if i.interlace else f"bit depth {i.bit_depth}"
        raise NotImplementedError(f"{who}: {what} PNG files are not supported (8-bit, non-interlaced only)")
    if not (1 <= h <= 1 << 24 and 1 <= w <= 1 << 24) or h * (1 + w * channels) > (1 << 31) - 1:
        raise ValueError(f"{who}: {w} x {h} picture of {channels} channels is too large")
    return h, w, ctype, channels


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
    if extended:
        i = _png_check(arr, "decode_png", True)
        dtype, shape = _png_out_format(i)
        out = np.empty(shape, dtype=np.uint8 if dtype == np.dtype(bool) else dtype)
        _file_call("lars_h_decode_png_ex", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes)
        return out.view(dtype)
    h, w, _ctype, c = _png_check(arr, "decode_png")
    out = np.empty((h, w) if c == 1 else (h, w, c), dtype=np.uint8)
    _file_call("lars_h_decode_png_u8", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes)
    return out


def thumbnail_png(data, size=(400, 400), reducing_gap=2.0, extended=False):
    """``np.asarray`` of ``Image.open(io.BytesIO(data))`` after ``.thumbnail(size, LANCZOS, reducing_gap)``, bit for bit
    (process-images.py:186-189), from the file's bytes: the decoded pixels stay on the GPU and go straight into the
    thumbnail kernels, only the thumbnail comes back.  Modes L, RGB and RGBA; others raise ``TypeError`` as ``thumbnail``
    does.  ``draft`` does nothing for PNG, so ``thumbnail_plan(..., draft_box=None)`` is the whole plan; a file that
    already fits comes back as ``decode_png`` gives it.  Errors of the file as ``decode_png``.

    ``extended=True`` takes every file ``decode_png(data, extended=True)`` decodes whose Pillow mode is L, RGB or RGBA: 2- and
    4-bit gray, 16-bit RGB / LA / RGBA, and the interlaced ones.  Modes ``1``, ``I;16``, ``P`` and ``LA`` raise ``TypeError``."""
    arr = _file_bytes(data, "thumbnail_png", "PNG")
    if extended:
        i = _png_check(arr, "thumbnail_png", True)
        mode = _PNG_MODES[(i.bit_depth, i.color_type)]
        if mode not in ("L", "RGB", "RGBA"):
            raise TypeError(f"thumbnail_png: PNG files in mode L, RGB or RGBA (got mode {mode!r})")
        c = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
        plan = thumbnail_plan((i.width, i.height), size, reducing_gap, None, None, rgba=c == 4)
        if plan is None:
            return decode_png(arr, extended=True)
        return _file_thumbnail("lars_h_thumbnail_png_ex", arr, plan, c)
    h, w, ctype, c = _png_check(arr, "thumbnail_png")
    if ctype not in (0, 2, 6):
        raise TypeError(f"thumbnail_png: PNG files in mode L, RGB or RGBA (got mode {_PNG_MODES[(8, ctype)]!r})")
    plan = thumbnail_plan((w, h), size, reducing_gap, None, None, rgba=c == 4)
    if plan is None:
        return decode_png(arr)
    return _file_thumbnail("lars_h_thumbnail_png_u8", arr, plan, c)


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
    lib = _ffi.load()
    info = _ffi.JpegInfo.array()
    if lib.lars_jpeg_info(_ffi.ptr(arr), arr.size, info) != 0:
        raise ValueError(lib.lars_last_error().decode("utf-8", "replace"))
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
    if scale == 1:
        out = np.empty((h, w) if c == 1 else (h, w, c), dtype=np.uint8)
        _file_call("lars_h_decode_jpeg_u8", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes)
        return out
    h, w = -(-h // scale), -(-w // scale)
    out = np.empty((h, w) if c == 1 else (h, w, c), dtype=np.uint8)
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
        new_w, new_h = plan.size
        out = np.empty((new_h, new_w) if c == 1 else (new_h, new_w, c), dtype=np.uint8)
        _file_call("lars_h_thumbnail_jpeg_scaled_u8", _ffi.ptr(arr), arr.size, scale, plan.factor[0], plan.factor[1],
                   (C.c_int * 4)(*plan.reduce_box), (C.c_float * 4)(*plan.box), new_h, new_w, int(plan.vertical_first), _ffi.ptr(out))
        return out
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
    lib = _ffi.load()
    info = _ffi.TiffInfo.array()
    if (lib.lars_tiff_info_deflate if deflate else lib.lars_tiff_info)(_ffi.ptr(arr), arr.size, info, None, 0) != 0:
        raise ValueError(lib.lars_last_error().decode("utf-8", "replace"))
    return _ffi.TiffInfo(*info)


def _tiff_shape(i):
    return (i.height, i.width) if i.samples == 1 else (i.height, i.width, i.samples)


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
    out["shape"] = _tiff_shape(i) if known else None
    out["reason"] = _TIFF_REASON_TEXT.get(i.reason, str(i.reason))
    return out


def _tiff_check(arr, who, deflate=False):
    from .tiffio import TiffError
    try:
        i = _tiff_info(arr, deflate)
    except ValueError as e:
        raise TiffError(str(e)) from None
    if not i.supported:
        raise NotImplementedError(f"{who}: TIFF files with {_TIFF_REASON_TEXT.get(i.reason, i.reason)} are not decoded on the device "
                                  "(classic TIFF, 8 or 16 bit unsigned or float32 samples, uncompressed or LZW; Deflate with deflate=True)")
    return i


def _tiff_call(name, *args):
    from .tiffio import TiffError
    try:
        _ffi.call(name, *args)
    except _ffi.LarsError as e:
        if e.code == -1:
            raise TiffError(str(e)) from None
        raise


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
    out = np.empty(_tiff_shape(i), dtype=_TIFF_DTYPES[i.bits])
    _tiff_call("lars_h_decode_tiff_deflate" if deflate else "lars_h_decode_tiff", _ffi.ptr(arr), arr.size, _ffi.ptr(out), out.nbytes)
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
    from .tiffio import TiffError
    try:
        return _file_thumbnail("lars_h_thumbnail_tiff_deflate_u8" if deflate else "lars_h_thumbnail_tiff_u8", arr, plan, i.samples)
    except ValueError as e:
        raise TiffError(str(e)) from None


def process_image(img_array, indices=INDEX_NAMES, white_balance=True, want_arrays=True, want_hist=False,
                  want_rgba=False, want_entries=False, want_png=False, want_tiff=False):
    """White balance -> indices -> statistics of one image in ONE upload.

    What the Streamlit comparison path does with three separate calls per index
    (process-images.py:1457, :1522, :1525).  Returns a dict with
    ``corrected`` (uint8), and per index ``index`` (float32), ``stats`` (the
    ``analyze_index`` dict), ``hist`` (50 bins) and ``rgba``.  ``want_entries=True`` (instead of
    ``want_rgba``) returns ``entry``: the colormap entry of every pixel, uint8 ``[h, w]``, computed on the
    device -- ``colormap_lut(name)[entry]`` is the RGBA image, and a palette PNG needs nothing else
    (one byte per pixel crosses PCIe; backend-process.py:40-47 per pixel).
    ``want_png=True`` adds ``png``: the PNG file (``bytes``) of the RGBA colormap picture, encoded on the device
    (``encode_png``); ``want_png="palette"`` a mode-P file of the colormap entries with the colormap as its palette.  Either
    way only the file crosses PCIe.
    ``want_tiff=True`` adds ``tiff``: the float32 LZW TIFF file (``bytes``) of the index plane itself, encoded on the device
    (``encode_tiff_f32``, one strip rule for all); ``want_tiff="predictor"`` writes it with Predictor 3.  The plane then need
    not cross PCIe (``want_arrays=False``).  ``want_tiff="deflate"`` and ``"deflate+predictor"`` write the Deflate file instead
    (``encode_tiff_f32(..., compression="deflate")``).  Not together with ``want_png`` (one kind of file per call).
    """
    tiff_modes = {"predictor": 2, "deflate": 3, "deflate+predictor": 4}
    tiff_mode = 0 if want_tiff is False else 1 if want_tiff is True else tiff_modes.get(want_tiff) if isinstance(want_tiff, str) else None
    if tiff_mode is None:
        raise ValueError(f"process_image: want_tiff must be False, True or 'predictor' ('deflate' or 'deflate+predictor' for Deflate), "
                         f"got {want_tiff!r}")
    if tiff_mode and want_png is not False:
        raise ValueError("process_image: want_tiff or want_png, not both (one kind of file per call)")
    png_mode = 0 if want_png is False else 1 if want_png is True else 2 if isinstance(want_png, str) and want_png == "palette" else None
    if png_mode is None:
        raise ValueError(f"process_image: want_png must be False, True or 'palette', got {want_png!r}")
    if png_mode and (want_rgba or want_entries):
        raise ValueError("process_image: want_png replaces want_rgba / want_entries (the pictures stay on the device)")
    if want_rgba and want_entries:
        raise ValueError("process_image: want_rgba or want_entries, not both (they share the output slot of the C ABI)")
    arr = _as_image(img_array, "process_image")
    code = _ffi.dtype_code(arr.dtype)
    if code is None:
        raise TypeError(f"process_image: unsupported sample type {arr.dtype}")
    for t in indices:
        if t not in INDEX_IDS:
            raise ValueError(f"Unknown index type: {t}")
    h, w, c = arr.shape
    mask = index_mask(indices)
    out_wb = _empty((h, w, c), dtype=np.uint8) if white_balance else None
    outs, rgbas, luts = [None] * 3, [None] * 3, [None] * 3
    for t in indices:
        k = INDEX_IDS[t]
        if want_arrays:
            outs[k] = _empty((h, w), dtype=np.float32)
        if want_rgba:
            rgbas[k] = _empty((h, w, 4), dtype=np.uint8)
            luts[k] = colormap_lut(_colormap_for(t))
        elif want_entries:
            rgbas[k] = _empty((h, w), dtype=np.uint8)          # no table: the entry plane comes back in the RGBA slot
    stats = (Stats * 3)()
    med = np.zeros((3, 2), dtype=np.float32)
    pngs, tiffs = [None] * 3, [None] * 3
    if tiff_mode:
        tiff_deflate = tiff_mode >= 3
        cap = tiff_f32_bound(h, w, 1, compression="deflate" if tiff_deflate else "lzw")
        if cap == 0:
            raise ValueError(f"process_image: a {h} x {w} plane is not encoded as a TIFF file (1 to 2^24 on each side)")
        for t in indices:
            tiffs[INDEX_IDS[t]] = np.empty(cap, dtype=np.uint8)
        lens = np.zeros(3, dtype=np.int64)
        p_out, p_rgba, p_lut, p_tiff = _ffi.ptr3(outs), _ffi.ptr3(rgbas), _ffi.ptr3(luts), _ffi.ptr3(tiffs)
        head = (_ffi.ptr(arr), h, w, c, code, int(bool(white_balance)), mask, int(want_hist), _ffi.ptr(out_wb), C.byref(p_out), C.byref(stats),
                _ffi.ptr(med), C.byref(p_rgba), C.byref(p_lut))
        tail = (int(tiff_mode in (2, 4)), 0, C.byref(p_tiff), cap, _ffi.ptr(lens))
        if tiff_deflate:
            _ffi.call("lars_h_process_image_tiff_float32", *head, 8, *tail)
        else:
            _ffi.call("lars_h_process_image_tiff_f32", *head, *tail)
        tiffs = [None if p is None else p[:lens[k]].tobytes() for k, p in enumerate(tiffs)]
    elif png_mode:
        cap = png_bound(h, w, 4 if png_mode == 1 else 1)
        for t in indices:
            k = INDEX_IDS[t]
            luts[k] = colormap_lut(_colormap_for(t))
            pngs[k] = np.empty(cap, dtype=np.uint8)
        lens = np.zeros(3, dtype=np.int64)
        p_out, p_lut, p_png = _ffi.ptr3(outs), _ffi.ptr3(luts), _ffi.ptr3(pngs)
        _ffi.call("lars_h_process_image_png", _ffi.ptr(arr), h, w, c, code, int(bool(white_balance)), mask, int(want_hist),
                  _ffi.ptr(out_wb), C.byref(p_out), C.byref(stats), _ffi.ptr(med), C.byref(p_lut), png_mode, C.byref(p_png), cap,
                  _ffi.ptr(lens))
        pngs = [None if p is None else p[:lens[k]].tobytes() for k, p in enumerate(pngs)]
    else:
        p_out, p_rgba, p_lut = _ffi.ptr3(outs), _ffi.ptr3(rgbas), _ffi.ptr3(luts)
        _ffi.call("lars_h_process_image", _ffi.ptr(arr), h, w, c, code, int(bool(white_balance)), mask, int(want_hist),
                  _ffi.ptr(out_wb), C.byref(p_out), C.byref(stats), _ffi.ptr(med), C.byref(p_rgba), C.byref(p_lut))
    result = {"corrected": out_wb, "indices": {}}
    for t in indices:
        k = INDEX_IDS[t]
        st = stats[k]
        feature_name, _ = _coverage_rule(t)
        median = float(np.float32(np.float32(med[k, 0] + med[k, 1]) / 2))
        result["indices"][t] = {
            "index": outs[k],
            "rgba": rgbas[k] if want_rgba else None,
            "entry": rgbas[k] if want_entries else None,
            "png": pngs[k],
            "tiff": tiffs[k],
            "hist": np.array(list(st.hist), dtype=np.int64) if want_hist else None,
            "stats": {
                f"Mean {t}": st.sum / st.count,
                f"Median {t}": median,
                f"Min {t}": st.min,
                f"Max {t}": st.max,
                f"{feature_name} Coverage (%)": st.above / st.count * 100,
            },
        }
    return result


# ---------------------------------------------------------------------------
# registration, change detection, time series
# ---------------------------------------------------------------------------
_ALIGN_MAX_DIM = 1024                                      # process-images.py:530


def align_images(fixed_img, moving_img):
    """process-images.py:515-565: register ``moving_img`` onto ``fixed_img`` by phase correlation.

    Returns ``(aligned_img, shift)`` like upstream: ``shift`` is what
    ``skimage.registration.phase_cross_correlation`` returns (``[dy, dx]``, with a trailing 0
    for the channel axis of a colour image) and ``aligned_img`` is
    ``scipy.ndimage.shift(moving_img, shift, order=1, mode='reflect')``.  Images larger than 1024
    on a side are down-scaled first (both, independently, as upstream -- the aligned image then has
    the down-scaled size).  ``None`` in -> ``(moving_img, array([0, 0]))``.
    """
    if fixed_img is None or moving_img is None:
        return moving_img, np.array([0, 0])
    fixed_img, moving_img = np.asarray(fixed_img), np.asarray(moving_img)
    if fixed_img.shape[0] > _ALIGN_MAX_DIM or fixed_img.shape[1] > _ALIGN_MAX_DIM:
        fixed_img = preprocess_large_image(fixed_img, _ALIGN_MAX_DIM)
    if moving_img.shape[0] > _ALIGN_MAX_DIM or moving_img.shape[1] > _ALIGN_MAX_DIM:
        moving_img = preprocess_large_image(moving_img, _ALIGN_MAX_DIM)
    for name, a in (("fixed_img", fixed_img), ("moving_img", moving_img)):
        if a.dtype != np.uint8:
            raise TypeError(f"align_images: {name} must be uint8 (got {a.dtype})")
        if a.ndim == 3 and a.shape[2] != 3:
            # skimage.color.rgb2gray's own complaint
            raise ValueError(f"the input array must have size 3 along `channel_axis`, got {a.shape}")
        if a.ndim not in (2, 3):
            raise ValueError(f"align_images: {name} must be [H, W] or [H, W, 3] (got shape {a.shape})")
    if fixed_img.shape != moving_img.shape:
        raise ValueError("images must be same shape")      # phase_cross_correlation's own complaint
    fixed_c, moving_c = np.ascontiguousarray(fixed_img), np.ascontiguousarray(moving_img)
    h, w = moving_c.shape[:2]
    channels = 1 if moving_c.ndim == 2 else 3
    aligned = _empty(moving_c.shape, moving_c.dtype)
    shift = np.zeros(2, dtype=np.float64)
    _ffi.call("lars_h_align_images", _ffi.ptr(fixed_c), _ffi.ptr(moving_c), h, w, channels, _ffi.ptr(aligned), _ffi.ptr(shift))
    if moving_c.ndim == 3:
        shift = np.append(shift, 0)                         # process-images.py:552-554
    return aligned, shift


def colorize_difference(diff, vmin=-0.5, vmax=0.5, cmap="bwr"):
    """Per-pixel RGBA8 of ``imshow(diff, cmap='bwr', vmin=-0.5, vmax=0.5)`` (process-images.py:956)."""
    arr = np.ascontiguousarray(diff, dtype=np.float32)
    out = _empty(arr.shape + (4,), dtype=np.uint8)
    _ffi.call("lars_h_colormap_norm_f32", _ffi.ptr(arr.reshape(-1)), arr.size, float(vmin), float(vmax),
              _ffi.ptr(colormap_lut(cmap)), _ffi.ptr(out))
    return out


def change_detection(early, late, index_type, early_corrected=None, late_corrected=None, align=True, want_rgba=False):
    """The arithmetic of ``create_change_detection_visualization`` (process-images.py:885-923, :956).

    ``early`` / ``late`` are the raw uint8 images, ``*_corrected`` the cached white-balanced arrays
    the UI keeps (process-images.py:894-902); whichever is missing is computed.  One upload: white
    balance, registration of the late image, both indices, ``diff = late_index - early_index`` and
    (``want_rgba``) the per-pixel ``bwr`` map of the difference.  Returns a dict with
    ``early_index``, ``late_index``, ``diff``, ``aligned_late``, ``shift`` and ``diff_rgba``.
    """
    if index_type not in INDEX_IDS:
        raise ValueError(f"Unknown index type: {index_type}")
    e_src = early_corrected if early_corrected is not None else early
    l_src = late_corrected if late_corrected is not None else late
    if e_src is None or l_src is None:
        return None
    e_arr, l_arr = _as_image(e_src, "change_detection"), _as_image(l_src, "change_detection")
    wb_e, wb_l = early_corrected is None, late_corrected is None
    fused = (e_arr.dtype == np.uint8 and l_arr.dtype == np.uint8 and e_arr.shape == l_arr.shape
             and (not align or (e_arr.shape[2] == 3 and max(e_arr.shape[:2]) <= _ALIGN_MAX_DIM)))
    if not fused:
        # sizes the one-upload entry point does not cover: the same steps, one call each
        e_c = fix_white_balance(e_arr) if wb_e else e_arr
        l_c = fix_white_balance(l_arr) if wb_l else l_arr
        aligned, shift = align_images(e_c, l_c) if align else (l_c, np.zeros(3))
        e_idx, l_idx = calculate_index(e_c, index_type), calculate_index(aligned, index_type)
        diff = l_idx - e_idx                               # raises like upstream when the shapes differ (:923)
        return {"early_index": e_idx, "late_index": l_idx, "diff": diff, "aligned_late": aligned, "shift": shift,
                "diff_rgba": colorize_difference(diff) if want_rgba else None}
    h, w, c = e_arr.shape
    e_idx, l_idx, diff = (_empty((h, w), dtype=np.float32) for _ in range(3))
    aligned = _empty((h, w, c), dtype=np.uint8)
    rgba = _empty((h, w, 4), dtype=np.uint8) if want_rgba else None
    shift = np.zeros(2, dtype=np.float64)
    _ffi.call("lars_h_change_detection", _ffi.ptr(e_arr), _ffi.ptr(l_arr), h, w, c, int(wb_e), int(wb_l), int(bool(align)),
              INDEX_IDS[index_type], _ffi.ptr(e_idx), _ffi.ptr(l_idx), _ffi.ptr(diff), _ffi.ptr(rgba),
              _ffi.ptr(colormap_lut("bwr")) if want_rgba else None, -0.5, 0.5, _ffi.ptr(aligned), _ffi.ptr(shift))
    return {"early_index": e_idx, "late_index": l_idx, "diff": diff, "aligned_late": aligned,
            "shift": np.append(shift, 0), "diff_rgba": rgba}


def corrected_of(img_data):
    """The cached white-balanced array of an ``image_data`` dict, or ``None`` (process-images.py:636-641)."""
    if "corrected_array" in img_data and img_data["corrected_array"] is not None:
        return img_data["corrected_array"]
    return None


def _timeframe_records(image_data_list, index_type, want_median):
    """[(date, Stats, median)] of every image of a series: one upload per image, nothing but the
    statistics comes back."""
    if index_type not in INDEX_IDS:
        raise ValueError(f"Unknown index type: {index_type}")
    k = INDEX_IDS[index_type]
    _, threshold = _coverage_rule(index_type)
    out = []
    for img_data in image_data_list:
        date = img_data["metadata"]["upload_date"]
        corrected = corrected_of(img_data)
        src = corrected if corrected is not None else img_data["array"]
        if src is None or np.size(src) == 0:
            continue                                        # calculate_index -> None -> the row is skipped (:649)
        arr = _as_image(src, "time series")
        code = _ffi.dtype_code(arr.dtype)
        if code is None:
            raise TypeError(f"time series: unsupported sample type {arr.dtype}")
        h, w, c = arr.shape
        stats = (Stats * 3)()
        med = np.zeros((3, 2), dtype=np.float32)
        _ffi.call("lars_h_process_image", _ffi.ptr(arr), h, w, c, code, int(corrected is None), 1 << k, 0, None, None,
                  C.byref(stats), _ffi.ptr(med) if want_median else None, None, None)
        median = float(np.float32(np.float32(med[k, 0] + med[k, 1]) / 2)) if want_median else None
        out.append((date, stats[k], median))
    return out


def calculate_index_statistics_by_timeframe(image_data_list, index_type):
    """process-images.py:619-667: pandas DataFrame, one row per image, the upstream columns."""
    import pandas as pd
    feature_name, _ = _coverage_rule(index_type)
    results = []
    for date, st, median in _timeframe_records(image_data_list, index_type, want_median=True):
        results.append({"Date": date, "Mean": st.sum / st.count, "Median": median, "Min": st.min, "Max": st.max,
                        f"{feature_name} Coverage (%)": st.above / st.count * 100})
    return pd.DataFrame(results)


def time_series_points(image_data_list, index_type):
    """The numbers ``create_time_series_plot`` draws (process-images.py:814-832): dates, means, maxima, minima."""
    recs = _timeframe_records(image_data_list, index_type, want_median=False)
    return ([d for d, _, _ in recs], [st.sum / st.count for _, st, _ in recs], [st.max for _, st, _ in recs],
            [st.min for _, st, _ in recs])


def download_processed_images(image_data, corrected_array, selected_indices):
    """process-images.py:567-617: ZIP bytes with ``white_balanced.png`` and ``<INDEX>_visualization.png`` per index.
    The index pictures are full-resolution per-pixel colormap images from one GPU pass (``driver.export_zip``), not
    the reference's matplotlib figures."""
    from .driver import export_zip
    return export_zip(None if image_data is None else image_data.get("array"), selected_indices,
                      corrected_array=corrected_array)


def generate_ndvi_report(image_path, output_dir):
    """process-ndvi.py:75-110 without its two matplotlib figures: writes ``ndvi_visualization.png`` (per-pixel RdYlGn
    image of the NDVI), ``ndvi_histogram.csv`` (the 50 counts ``plt.hist(ndvi.flatten(), bins=50, range=(-1, 1))``
    would draw, with their bin edges) and ``ndvi_statistics.txt`` (same text as upstream) into ``output_dir``;
    returns ``(ndvi_array, stats)``.  NDVI, statistics and histogram counts come from the GPU."""
    os.makedirs(output_dir, exist_ok=True)
    ndvi_array = calculate_ndvi(image_path, os.path.join(output_dir, "ndvi_visualization.png"), visualize=False)
    stats = analyze_ndvi_statistics(ndvi_array)
    counts = index_histogram(ndvi_array)
    edges = np.linspace(-1.0, 1.0, 51)
    with open(os.path.join(output_dir, "ndvi_histogram.csv"), "w") as f:
        f.write("bin_left,bin_right,pixel_count\n")
        for k in range(50):
            f.write(f"{edges[k]:.2f},{edges[k + 1]:.2f},{int(counts[k])}\n")
    with open(os.path.join(output_dir, "ndvi_statistics.txt"), "w") as f:
        f.write("NDVI Statistics:\n")
        for key, value in stats.items():
            f.write(f"{key}: {value:.4f}\n")
    return ndvi_array, stats


# ---------------------------------------------------------------------------
# the reference's figure functions: out of scope here, and saying so loudly
# ---------------------------------------------------------------------------
def _figure_function(name, lines, instead):
    def stub(*_args, **_kwargs):
        raise NotImplementedError(
            f"{name} (process-images.py:{lines}) draws a matplotlib figure and stays in the reference: this package replaces the "
            f"hot-path functions it calls, not the drawing.  Keep the reference's {name} and swap its imports as INTEGRATION.md "
            f"section 1 shows; the numbers it draws come from {instead}.")
    stub.__name__ = name
    stub.__doc__ = f"Not provided: {name} (process-images.py:{lines}) is figure rendering; see INTEGRATION.md (differs from the reference)."
    return stub


create_index_visualization = _figure_function("create_index_visualization", "669-716", "calculate_index / colorize_index")
create_comparison_view = _figure_function("create_comparison_view", "718-799", "process_image / colorize_index")
create_time_series_plot = _figure_function("create_time_series_plot", "801-883", "time_series_points")
create_change_detection_visualization = _figure_function("create_change_detection_visualization", "885-989", "change_detection")
