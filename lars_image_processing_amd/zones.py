"""Zonal statistics (DESIGN.md "Zonal statistics"): one row per plot from a label raster, in one upload and one pass.

``zones`` is an integer ``[H, W]`` array of labels ``0 .. Z``; 0 is "in no zone".  For zone ``z`` the figures are
``analyze_index``'s on ``index[valid & (zones == z)]``: ``zonal_statistics`` for any float32 plane, ``process_image_zones`` for a
picture, whose white balance stays the whole valid picture's, never the plot's.  ``zonal_rows`` turns either result into the rows a
table or a CSV wants.  The kernels are csrc/zonal.hip; there is no NumPy fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from . import nodata as _nodata
from ._ffi import INDEX_IDS
from .api import _coverage_rule, _picture, _picture_result

ZONES_MAX = 65535
_FIGURES = ("mean", "median", "min", "max", "coverage")


def _labels(zones, shape, n_zones, who):
    """``zones`` -> (C-contiguous uint8 / uint16 / int32 ``[H, W]`` labels, Z): every check that needs no device."""
    z = np.asarray(zones)
    if z.dtype.kind not in "ui":
        raise TypeError(f"{who}: zones must be an integer array of labels 0 .. Z (0 = in no zone), got {z.dtype}")
    if z.shape != tuple(shape):
        raise ValueError(f"{who}: zones has shape {z.shape}, the raster is {tuple(shape)}")
    if z.size == 0:
        raise ValueError(f"{who}: zones is empty")
    if n_zones is not None:
        if isinstance(n_zones, (bool, np.bool_)) or not isinstance(n_zones, (int, np.integer)):
            raise TypeError(f"{who}: n_zones must be an int or None (got {type(n_zones).__name__})")
        if not 1 <= int(n_zones) <= ZONES_MAX:
            raise ValueError(f"{who}: n_zones must be 1 to {ZONES_MAX}, got {int(n_zones)}")
    if z.dtype.kind == "i":
        negative = int(np.count_nonzero(z < 0))
        if negative:
            top = f"0 .. {int(n_zones)}" if n_zones is not None else "0 .. Z"
            raise ValueError(f"{who}: {negative} pixels have a negative label; the labels allowed are {top}")
    if n_zones is None:
        n_zones = int(z.max())
        if not 1 <= n_zones <= ZONES_MAX:
            raise ValueError(f"{who}: the largest label is {n_zones}; without n_zones it must be 1 to {ZONES_MAX}")
    n_zones = int(n_zones)
    if z.dtype not in (np.uint8, np.uint16, np.int32):
        # other widths go as int32 once their labels are known to fit: the device counts what is above Z, so only wrap-around is refused
        above = int(np.count_nonzero(z > n_zones))
        if above:
            raise ValueError(f"{who}: {above} pixels have a label outside 0 .. {n_zones}")
        z = z.astype(np.int32)
    return np.ascontiguousarray(z), n_zones


def _bad_labels(who, bad, n_zones):
    return ValueError(f"{who}: {bad} pixels have a label outside 0 .. {n_zones}")


def _figures(records, medians, want_hist):
    """``lars_stats`` records ``[Z]`` and median pairs ``[Z, 2]`` -> the per-zone arrays, by ``api._summary``'s rules."""
    count = records["count"].astype(np.int64)
    empty, nan_inside = count == 0, records["nans"] != 0
    blank = empty | nan_inside
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        median = ((medians[:, 0] + medians[:, 1]).astype(np.float32) / np.float32(2)).astype(np.float64)   # the two middles' mean in float32
        out = {
            "mean": np.where(blank, np.nan, records["sum"] / count),
            "median": np.where(blank, np.nan, median),
            "min": np.where(blank, np.nan, records["min"]),
            "max": np.where(blank, np.nan, records["max"]),
            "coverage": np.where(empty, np.nan, records["above"] / count * 100),
        }
    if want_hist:
        out["hist"] = records["hist"].astype(np.int64)
    return count, out


def zonal_statistics(index_array, zones, index_type, valid=None, n_zones=None, want_hist=False):
    """``analyze_index`` of every zone of a float32 ``[H, W]`` plane in one pass: a dict of arrays with one entry per zone ``1 .. Z``.

    ``zone`` and ``pixels`` (int64), ``mean``, ``median``, ``min``, ``max``, ``coverage`` (float64) and, with ``want_hist``, ``hist``
    (int64 ``[Z, 50]``).  ``index_type`` picks the coverage threshold (water above 0 for NDWI, vegetation above 0.2 otherwise),
    compared in float32.  ``valid``: an ``[H, W]`` bool or integer mask (nonzero = counts) or None.  ``n_zones=None`` takes the
    largest label.  A zone without pixels has ``pixels`` 0, NaN figures and an empty histogram; a zone that holds a NaN has NaN
    mean / median / min / max.  A label below 0 or above ``n_zones`` raises ``ValueError`` with the number of such pixels.
    Everything but ``mean`` is bit-reproducible; the mean's double sum follows the order the device placed the values in."""
    who = "zonal_statistics"
    if index_type not in INDEX_IDS:
        raise ValueError(f"{who}: Unknown index type: {index_type}")
    x = np.asarray(index_array)
    if x.dtype != np.float32:
        raise TypeError(f"{who}: index_array must be float32 (got {x.dtype})")
    if x.ndim != 2 or x.size == 0:
        raise ValueError(f"{who}: index_array must be a non-empty [H, W] array, got shape {x.shape}")
    h, w = x.shape
    lab, nz = _labels(zones, (h, w), n_zones, who)
    if isinstance(valid, str):
        raise TypeError(f"{who}: valid must be an [H, W] bool or integer array or None: a plane has no alpha channel")
    valid_arr, _ = _nodata.valid_argument(valid, (h, w, 0), who)
    _, threshold = _coverage_rule(index_type)
    x = np.ascontiguousarray(x)
    records = np.zeros(nz, dtype=_ffi.STATS_DTYPE)
    medians = np.zeros((nz, 2), dtype=np.float32)
    bad = C.c_int64(-1)
    try:
        _ffi.call("lars_h_zonal_stats_f32", _ffi.ptr(x), _ffi.ptr(lab), lab.dtype.itemsize, _ffi.ptr(valid_arr), h, w, nz,
                  np.float32(threshold), int(bool(want_hist)), _ffi.ptr(records), _ffi.ptr(medians), C.byref(bad))
    except _ffi.LarsError:
        if bad.value > 0:
            raise _bad_labels(who, bad.value, nz) from None
        raise
    count, out = _figures(records, medians, want_hist)
    return {"zone": np.arange(1, nz + 1, dtype=np.int64), "pixels": count, **out}


def process_image_zones(img_array, zones, valid=None, nodata=None, n_zones=None, indices=_ffi.INDEX_NAMES, white_balance=True,
                        want_arrays=True, want_hist=False, want_rgba=False):
    """``process_image_masked`` plus one row per zone: its dict with ``"zones": {"zone", "pixels", t: {mean, median, min, max,
    coverage[, hist]}}`` added.

    The picture crosses PCIe once, the white balance is taken over the whole valid picture -- zones do not change which pixels its
    percentiles see -- and one pass sorts every valid pixel's index value into its zone.  ``corrected``, the planes, ``rgba``, the
    picture-level statistics and ``valid_pixels`` are exactly ``process_image_masked``'s with the same ``valid`` / ``nodata``; the
    zone figures are ``zonal_statistics``'s of each plane under the derived mask.  At least one index must be asked for."""
    who = "process_image_zones"
    p = _picture(who, who, img_array, list(indices), white_balance, want_arrays, bool(want_hist), want_rgba, False, valid, nodata,
                 need_index="zone statistics need at least one index")
    indices = p.indices
    lab, nz = _labels(zones, (p.h, p.w), n_zones, who)
    records = np.zeros((3, nz), dtype=_ffi.STATS_DTYPE)
    medians = np.zeros((3, nz, 2), dtype=np.float32)
    nvalid, bad = C.c_int64(-1), C.c_int64(-1)
    p_rgba, p_lut = _ffi.ptr3(p.rgbas), _ffi.ptr3(p.luts)
    try:
        _ffi.call("lars_h_process_image_zones", *p.head, C.byref(p_rgba), C.byref(p_lut), _ffi.ptr(p.valid), int(p.use_alpha),
                  int(p.nodata is not None), p.nodata or 0, C.byref(nvalid), _ffi.ptr(lab), lab.dtype.itemsize, nz, _ffi.ptr(records),
                  _ffi.ptr(medians), C.byref(bad))
    except _ffi.LarsError:
        if nvalid.value == 0:
            raise ValueError("process_image: no valid pixel") from None
        if bad.value > 0:
            raise _bad_labels(who, bad.value, nz) from None
        raise
    result = _picture_result(p, want_hist, want_rgba, False, valid_pixels=nvalid.value)
    result["zones"] = {"zone": np.arange(1, nz + 1, dtype=np.int64)}
    for t in indices:
        result["zones"]["pixels"], result["zones"][t] = _figures(records[INDEX_IDS[t]], medians[INDEX_IDS[t]], want_hist)
    return result


def zonal_rows(result_or_stats, index_type):
    """One dict per zone -- ``"Zone"``, ``"Pixels"`` and ``analyze_index``'s five keys for ``index_type`` -- from ``zonal_statistics``'s
    dict, ``process_image_zones``'s result or its ``"zones"`` part: the rows of a per-plot table or CSV."""
    if index_type not in INDEX_IDS:
        raise ValueError(f"zonal_rows: Unknown index type: {index_type}")
    part = result_or_stats.get("zones", result_or_stats)
    figures = part[index_type] if index_type in part else part
    missing = [f for f in _FIGURES if f not in figures]
    if missing or "zone" not in part or "pixels" not in part:
        raise KeyError(f"zonal_rows: no zone figures for {index_type} in this result")
    feature_name, _ = _coverage_rule(index_type)
    keys = (f"Mean {index_type}", f"Median {index_type}", f"Min {index_type}", f"Max {index_type}", f"{feature_name} Coverage (%)")
    return [{"Zone": int(z), "Pixels": int(n), **{key: float(figures[f][i]) for key, f in zip(keys, _FIGURES)}}
            for i, (z, n) in enumerate(zip(part["zone"], part["pixels"]))]
