"""Pillow's thumbnail policy as numbers: what ``Image.thumbnail(size, LANCZOS, reducing_gap)`` and ``JpegImageFile.draft`` decide
before a pixel is touched.  Pure Python: no ctypes, no library, no GPU.  ``api.thumbnail`` and the thumbnails from file bytes
(``codecs``) hand these numbers to the library as they are."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

_LANCZOS_SUPPORT = 3.0                      # Image._filters_support[LANCZOS]


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
