"""Nodata-aware processing (DESIGN.md "Nodata-aware processing"): ``process_image_masked``, which is ``api.process_image`` with
``valid`` / ``nodata`` saying which pixels are picture, and ``valid_mask``, the public face of the device's derivation
(csrc/masked.hip: ``lars_d_valid_mask``).  ``api.process_image`` itself keeps its signature: tests/golden/codec_surface.json
records it, and a caller that names no mask has nothing to change."""
from __future__ import annotations

import numpy as np

from . import _ffi

NO_PALETTE_WITH_MASK = ("the 256-entry palette has no free entry for 'no data': with valid / nodata ask for want_rgba=True or "
                        "want_png=True (RGBA, transparent outside the mask)")


def nodata_value(nodata, dtype, who):
    """``nodata`` as a Python int inside the sample type's range, or None."""
    if nodata is None:
        return None
    if isinstance(nodata, (bool, np.bool_)) or not isinstance(nodata, (int, np.integer)):
        raise TypeError(f"{who}: nodata must be an int (got {type(nodata).__name__})")
    top = int(np.iinfo(dtype).max)
    if not 0 <= int(nodata) <= top:
        raise ValueError(f"{who}: nodata {int(nodata)} is outside the range of {np.dtype(dtype)} samples (0 to {top})")
    return int(nodata)


def valid_argument(valid, shape, who):
    """``valid`` of ``process_image_masked`` -> (uint8 [H, W] array or None, use_alpha)."""
    h, w, c = shape
    if valid is None:
        return None, False
    if isinstance(valid, str):
        if valid != "alpha":
            raise TypeError(f"{who}: valid must be an [H, W] bool or integer array or the string 'alpha', got {valid!r}")
        if c < 4:
            raise ValueError(f"{who}: valid='alpha' needs an image with 4 or more channels (this one has {c})")
        return None, True
    m = np.asarray(valid)
    if m.dtype.kind not in "bui":
        raise TypeError(f"{who}: valid must be a bool or integer array (nonzero = valid) or 'alpha', got {m.dtype}")
    if m.shape != (h, w):
        raise ValueError(f"{who}: valid has shape {m.shape}, the image is {(h, w)}")
    if m.dtype.itemsize != 1:                          # bool and 8-bit masks go as they are: the device reads nonzero bytes as valid
        m = m != 0
    return np.ascontiguousarray(m).view(np.uint8), False


def valid_mask(img_array, nodata=None, alpha=False):
    """Which pixels of an image are picture, as the device derives it for ``process_image_masked``: uint8 ``[H, W]``, 1 = valid.

    ``alpha=True``: valid where channel 3 is nonzero (4 or more channels).  ``nodata=N``: invalid where R, G and NIR all
    equal ``N``.  Both: their AND.  Neither: all ones."""
    from .api import _as_image
    from .hostpool import empty
    arr = _as_image(img_array, "valid_mask")
    code = _ffi.dtype_code(arr.dtype)
    if code is None:
        raise TypeError(f"valid_mask: unsupported sample type {arr.dtype}")
    h, w, c = arr.shape
    nd = nodata_value(nodata, arr.dtype, "valid_mask")
    if alpha and c < 4:
        raise ValueError(f"valid_mask: alpha=True needs an image with 4 or more channels (this one has {c})")
    out = empty((h, w), dtype=np.uint8)
    _ffi.call("lars_h_valid_mask", _ffi.ptr(arr), h, w, c, code, int(bool(alpha)), int(nd is not None), nd or 0, _ffi.ptr(out), None)
    return out


def process_image_masked(img_array, valid=None, nodata=None, indices=_ffi.INDEX_NAMES, white_balance=True, want_arrays=True,
                         want_hist=False, want_rgba=False, want_entries=False, want_png=False, want_tiff=False):
    """``api.process_image`` on a picture that is not picture everywhere: an orthomosaic's frame, reflected borders, a cut-out plot.

    ``valid`` is an ``[H, W]`` bool or integer array (nonzero = valid) or ``"alpha"`` (valid where channel 3 is nonzero; 4 or
    more channels); ``nodata=N`` makes a pixel invalid where R, G and NIR all equal ``N``; given together they combine with
    AND; with neither the call is ``api.process_image``'s.  Every result is the reference's on the valid pixels alone
    (``img[valid][None, :, :]``) scattered back: percentiles of the white balance, statistics, histogram and median of the valid
    values, coverage relative to their number -- ``valid_pixels`` in the result -- and outside the mask ``corrected`` 0 in every
    channel, ``index`` float32 NaN (``0x7FC00000``), ``rgba`` / ``png`` transparent ``(0, 0, 0, 0)`` (matplotlib's colour for masked
    data), ``tiff`` NaN.  No valid pixel at all raises ``ValueError("process_image: no valid pixel")``.  The other arguments are
    ``api.process_image``'s; ``want_entries=True`` and ``want_png="palette"`` are refused with a mask: the 256-entry palette has
    no free entry for "no data"."""
    from .api import _process_image
    return _process_image(img_array, indices, white_balance, want_arrays, want_hist, want_rgba, want_entries, want_png, want_tiff,
                          valid=valid, nodata=nodata)
