"""Zonal statistics (DESIGN.md "Zonal statistics"): one row per plot from a label raster, in one upload and one pass.

``zones`` is an integer ``[H, W]`` array of labels ``0 .. Z``; 0 is "in no zone".  For zone ``z`` the figures are
``analyze_index``'s on ``index[valid & (zones == z)]``: ``zonal_statistics`` for any float32 plane, ``process_image_zones`` for a
picture, whose white balance stays the whole valid picture's, never the plot's.  ``zonal_rows`` turns either result into the rows a
table or a CSV wants.  The kernels are csrc/zonal.hip; there is no NumPy fallback.

Where ``zones`` is wanted, plot outlines serve as well (DESIGN.md "Zones from polygons", csrc/zone_raster.hip): a list of polygons, or
``Polygons(list, transform=, want_labels=)``.  The labels are then made on the device and never cross PCIe; ``rasterize_zones`` returns
them, ``polygons_from_geojson`` reads the outlines from a GeoJSON export and ``to_pixel`` undoes a GDAL geotransform.

And where nobody drew outlines, the picture's own connected regions serve (DESIGN.md "Zones from regions", csrc/regions.hip):
``Regions(mask=...)`` or ``Regions(index=, above= / below=)`` labels the patches of a mask or of a thresholded plane on the device;
``label_regions`` returns such labels with each region's area, box and centroid.

The regions leave as shapes too (DESIGN.md "Region outlines", csrc/outlines.hip): ``region_outlines``, or ``Regions(...,
want_outlines=True)``, traces the ring of pixel borders around every region and every hole on the device, as ``Polygons`` that
``rasterize_zones`` turns back into the same labels; ``polygons_to_geojson`` writes them, ``to_world`` applies a geotransform.

The mixed pixels along a plot's edge stay out with a margin (DESIGN.md "Zone margins", csrc/zone_margin.hip): ``Shrunk(zones,
margin)`` where ``zones`` is wanted shrinks every zone inward by that many pixels on the device before ``zonal_statistics`` and
``process_image_zones`` take their figures, whichever of the three kinds made the labels; ``shrink_zones`` returns such labels.

And the outlines leave with a tolerance (DESIGN.md "Simplified outlines", csrc/outline_simplify.hip): ``region_outlines(...,
simplify=t)`` and ``Regions(..., want_outlines=True, simplify=t)`` run Douglas-Peucker on the traced rings on the device, so that only
the vertices kept cross PCIe; ``simplify_outlines`` does the same to outlines that came down earlier."""
from __future__ import annotations

import ctypes as C
import json
import math
import os

import numpy as np

from . import _ffi
from . import nodata as _nodata
from ._ffi import INDEX_IDS
from .api import _coverage_rule, _picture, _picture_result

ZONES_MAX = 65535
VERTICES_MAX = 1 << 24
COORDINATE_MAX = 1e9
OUTLINE_PIXELS_MAX = 1 << 29
MARGIN_MAX = 254
SIMPLIFY_MAX = 254
SIMPLIFY_SIDE_MAX = 32767
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


def _margin2(margin, who):
    """A margin in pixels -> the integer the device compares squared distances with: the largest ``n`` with float64
    ``sqrt(n) <= margin``.  Every check of a margin, on the host."""
    if isinstance(margin, (bool, np.bool_)) or not isinstance(margin, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: margin must be a number of pixels (got {type(margin).__name__})")
    m = float(margin)
    if not math.isfinite(m):
        raise ValueError(f"{who}: margin must be finite, got {margin!r}")
    if not 0 <= m <= MARGIN_MAX:
        raise ValueError(f"{who}: margin must be 0 to {MARGIN_MAX} pixels, got {margin!r}")
    n = int(math.floor(m * m))
    while n > 0 and math.sqrt(n) > m:                              # m * m rounded up past an integer
        n -= 1
    while math.sqrt(n + 1) <= m:
        n += 1
    return n


def _simplify_tq(tolerance, who):
    """A tolerance in pixels -> the integer the device compares distances with, in sixteenths of a pixel: ``floor(tolerance * 16 +
    0.5)``; None and every tolerance that rounds to 0 give 0, which is no simplification.  Every check of a tolerance, on the host."""
    if tolerance is None:
        return 0
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)):
        raise TypeError(f"{who}: simplify must be a number of pixels or None (got {type(tolerance).__name__})")
    t = float(tolerance)
    if not math.isfinite(t):
        raise ValueError(f"{who}: simplify must be finite, got {tolerance!r}")
    if not 0 <= t <= SIMPLIFY_MAX:
        raise ValueError(f"{who}: simplify must be 0 to {SIMPLIFY_MAX} pixels, got {tolerance!r}")
    return int(math.floor(t * 16 + 0.5))


def _simplify_sides(shape, who):
    if max(int(shape[0]), int(shape[1])) > SIMPLIFY_SIDE_MAX:
        raise ValueError(f"{who}: the raster is {int(shape[0])} x {int(shape[1])}; outlines are simplified on at most {SIMPLIFY_SIDE_MAX} a side "
                         f"(every product of coordinates fits 64 bits)")


class Shrunk:
    """Zones without their edge pixels: ``Shrunk(zones, margin)``, handed to ``zonal_statistics`` or ``process_image_zones`` where
    ``zones`` is wanted (DESIGN.md "Zone margins", csrc/zone_margin.hip).

    ``zones`` is any of the three kinds -- a label raster, polygons / ``Polygons``, ``Regions`` -- and ``margin`` the pixels (0 to 254)
    every zone is shrunk inward by on the device before its figures are taken, as ``shrink_zones`` does it: the figures are those of
    the same call on ``shrink_zones``'s raster, labels that come back are the shrunk ones, the regions' table describes the regions as
    found.  A margin of None or 0 is no margin: the call is the one on ``zones`` itself.  ``Regions(want_outlines=True)`` is refused:
    outlines are traced from regions that are connected.  Every check runs here, on the host."""

    def __init__(self, zones, margin):
        who = "Shrunk"
        if isinstance(zones, Shrunk):
            raise TypeError(f"{who}: these zones are shrunk already: give one margin")
        self.zones, self.margin = zones, margin
        self.margin2 = None
        if margin is None:
            return
        m2 = _margin2(margin, who)
        if margin == 0:
            return
        if isinstance(zones, Regions) and zones.want_outlines:
            raise ValueError(f"{who}: Regions(want_outlines=True) cannot be combined with a margin: outlines are traced from regions that "
                             f"are connected, and a margin may break them apart")
        self.margin2 = m2


def _unshrunk(zones):
    """``zones`` of a call -> (the zones themselves, margin2 or None)."""
    return (zones.zones, zones.margin2) if isinstance(zones, Shrunk) else (zones, None)


def _margin_entry(name, args, margin2):
    """The entry point ``name`` and its arguments, or with a margin its ``_margin`` variant, which takes ``margin2`` last."""
    if margin2 is None:
        return name, args
    return (name[:-4] + "_margin_f32" if name.endswith("_f32") else name + "_margin"), (*args, margin2)


def _geotransform(points, transform, who):
    """``(points as float64 [..., 2], the six numbers, their determinant)``: the checks ``to_pixel`` and ``to_world`` share."""
    try:
        t = np.asarray(transform, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: transform must be six numbers (x0, dx, rx, y0, ry, dy), got {transform!r}") from None
    if t.shape != (6,) or not np.isfinite(t).all():
        raise ValueError(f"{who}: transform must be six finite numbers (x0, dx, rx, y0, ry, dy), got {transform!r}")
    det = t[1] * t[5] - t[2] * t[4]
    if det == 0 or not np.isfinite(det):
        raise ValueError(f"{who}: the transform {tuple(t)} is singular: dx * dy - rx * ry = {det}")
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim < 1 or pts.shape[-1] != 2:
        raise ValueError(f"{who}: points must be [..., 2] (x, y), got shape {pts.shape}")
    return pts, t, det


def to_pixel(points, transform):
    """World coordinates ``[..., 2]`` -> pixel coordinates (x along the columns, y along the rows; pixel (i, j) has its centre at
    (j + 0.5, i + 0.5)) by the inverse of a GDAL geotransform ``(x0, dx, rx, y0, ry, dy)``: X = x0 + x * dx + y * rx, Y = y0 + x * ry +
    y * dy.  Float64 NumPy on the host.  A transform that is not six finite numbers or has no inverse raises ``ValueError``."""
    pts, (x0, dx, rx, y0, ry, dy), det = _geotransform(points, transform, "to_pixel")
    u, v = pts[..., 0] - x0, pts[..., 1] - y0
    return np.stack(((u * dy - v * rx) / det, (v * dx - u * ry) / det), axis=-1)


def to_world(points, transform):
    """Pixel coordinates ``[..., 2]`` (x along the columns, y along the rows) -> world coordinates by a GDAL geotransform
    ``(x0, dx, rx, y0, ry, dy)``: X = x0 + x * dx + y * rx, Y = y0 + x * ry + y * dy; the inverse of ``to_pixel``, with its checks.
    Float64 NumPy on the host."""
    pts, (x0, dx, rx, y0, ry, dy), _ = _geotransform(points, transform, "to_world")
    x, y = pts[..., 0], pts[..., 1]
    return np.stack((x0 + x * dx + y * rx, y0 + x * ry + y * dy), axis=-1)


def _rings_of(item, k, who):
    """The rings of polygon ``k``: an ``[n, 2]`` array-like is one ring, anything else a sequence of rings."""
    if isinstance(item, (str, bytes)) or item is None:
        raise TypeError(f"{who}: polygon {k} must be an [n, 2] array-like or a sequence of such rings, got {type(item).__name__}")
    try:
        a = np.asarray(item, dtype=np.float64)
    except (TypeError, ValueError):
        a = None                                                   # rings of different lengths
    if a is not None and a.ndim == 2:
        return [a]
    if a is not None and a.ndim == 3:
        return list(a)
    try:
        return list(item)
    except TypeError:
        raise TypeError(f"{who}: polygon {k} must be an [n, 2] array-like or a sequence of such rings, got {type(item).__name__}") from None


class Polygons:
    """Plot outlines, checked and packed as the library takes them: ``Polygons(polygons, transform=None, want_labels=False)``.

    ``polygons`` is a sequence; each item is an ``[n, 2]`` array-like of (x, y) vertices (one ring) or a sequence of such rings, whose
    edges are pooled (holes, parts).  Polygon ``k`` (0-based) labels its pixels ``k + 1``; where polygons overlap the later one wins.
    ``transform``: the six numbers of a GDAL geotransform when the vertices are world coordinates (``to_pixel`` is applied here).
    ``want_labels=True`` asks ``process_image_zones`` / ``zonal_statistics`` to return the label raster as well.  Every check runs
    here, on the host: ``TypeError`` / ``ValueError`` name the polygon and the ring."""

    def __init__(self, polygons, transform=None, want_labels=False, who="Polygons"):
        if isinstance(polygons, Polygons):
            if transform is not None:
                raise ValueError(f"{who}: these Polygons are in pixel coordinates already: transform cannot be applied again")
            self.verts, self.ring_starts, self.poly_starts = polygons.verts, polygons.ring_starts, polygons.poly_starts
            self.want_labels = bool(want_labels or polygons.want_labels)
            return
        if isinstance(polygons, (str, bytes, dict)) or polygons is None:
            raise TypeError(f"{who}: polygons must be a sequence of polygons, got {type(polygons).__name__} (polygons_from_geojson reads GeoJSON)")
        try:
            items = list(polygons)
        except TypeError:
            raise TypeError(f"{who}: polygons must be a sequence of polygons, got {type(polygons).__name__}") from None
        if not items:
            raise ValueError(f"{who}: the list of polygons is empty")
        if len(items) > ZONES_MAX:
            raise ValueError(f"{who}: {len(items)} polygons; at most {ZONES_MAX} make one label raster")
        rings, ring_starts, poly_starts, total = [], [0], [0], 0
        try:
            same = np.asarray(polygons if isinstance(polygons, np.ndarray) else items, dtype=np.float64) if len(items) > 1 else None
        except (TypeError, ValueError):
            same = None
        if same is not None and same.ndim == 3 and same.shape[1] >= 3 and same.shape[2] == 2:
            # Z single rings of one length, the usual export of a trial's plots: no step per polygon
            n = same.shape[1]
            ring_starts = list(range(0, len(items) * n + 1, n))
            poly_starts = list(range(len(items) + 1))
            total, items = len(items) * n, []
            rings = [same.reshape(-1, 2)]
        for k, item in enumerate(items):
            mine = _rings_of(item, k, who)
            if not mine:
                raise ValueError(f"{who}: polygon {k} has no ring")
            for r, ring in enumerate(mine):
                try:
                    a = np.asarray(ring, dtype=np.float64)
                except (TypeError, ValueError):
                    raise TypeError(f"{who}: polygon {k} ring {r} must be an [n, 2] array of numbers") from None
                if a.ndim != 2 or a.shape[1] != 2:
                    raise ValueError(f"{who}: polygon {k} ring {r} must have shape [n, 2] (x, y), got {a.shape}")
                if a.shape[0] < 3:
                    raise ValueError(f"{who}: polygon {k} ring {r} has {a.shape[0]} vertices; a ring needs 3 or more")
                total += a.shape[0]
                rings.append(a)
                ring_starts.append(total)
            poly_starts.append(len(rings))
        if total > VERTICES_MAX:
            raise ValueError(f"{who}: {total} vertices in all; at most 2**24 = {VERTICES_MAX}")
        if transform is not None:
            to_pixel(np.zeros((1, 2)), transform)                  # a bad transform is refused whatever the vertices are
        verts = np.concatenate(rings)                              # one pass over all vertices; the ring is looked up for a message only

        def ring_of(bad_rows):
            ring = int(np.searchsorted(ring_starts, int(np.flatnonzero(bad_rows)[0]), side="right")) - 1
            k = int(np.searchsorted(poly_starts, ring, side="right")) - 1
            return f"polygon {k} ring {ring - poly_starts[k]}"
        finite = np.isfinite(verts).all(axis=1)
        if not finite.all():
            raise ValueError(f"{who}: {ring_of(~finite)} has a coordinate that is not finite")
        if transform is not None:
            verts = to_pixel(verts, transform)
        small = (np.abs(verts) <= COORDINATE_MAX).all(axis=1)
        if not small.all():
            raise ValueError(f"{who}: {ring_of(~small)} has a pixel coordinate beyond 1e9 in size")
        self.verts = np.ascontiguousarray(verts)
        self.ring_starts = np.asarray(ring_starts, dtype=np.int32)
        self.poly_starts = np.asarray(poly_starts, dtype=np.int32)
        self.want_labels = bool(want_labels)

    @classmethod
    def _packed(cls, verts, ring_starts, poly_starts):
        """Arrays that are packed already, as the tracer of ``region_outlines`` leaves them: nothing to check."""
        self = object.__new__(cls)
        self.verts, self.ring_starts, self.poly_starts, self.want_labels = verts, ring_starts, poly_starts, False
        return self

    def __len__(self):
        return len(self.poly_starts) - 1

    def rings(self, k):
        """The rings of polygon ``k`` (0-based): a list of ``[n, 2]`` views of ``verts``."""
        return [self.verts[self.ring_starts[r]:self.ring_starts[r + 1]] for r in range(self.poly_starts[k], self.poly_starts[k + 1])]

    def _head(self):
        """The six polygon arguments of the C entry points."""
        return (_ffi.ptr(self.verts), len(self.verts), _ffi.ptr(self.ring_starts), len(self.ring_starts) - 1, _ffi.ptr(self.poly_starts),
                len(self))

    def _label_buffer(self, shape):
        return np.zeros(shape, dtype=np.uint8 if len(self) <= 255 else np.uint16)


def _whole(value, name, lo, hi, who):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{who}: {name} must be an int (got {type(value).__name__})")
    if not lo <= int(value) <= hi:
        raise ValueError(f"{who}: {name} must be {lo} to {hi}, got {int(value)}")
    return int(value)


def _foreground(mask, who):
    """``mask`` -> a C-contiguous uint8 ``[H, W]`` array of 0 / 1 with fewer than 2**31 pixels: every check that needs no device."""
    m = np.asarray(mask)
    if m.dtype.kind not in "uib":
        raise TypeError(f"{who}: mask must be a bool or integer array (nonzero = foreground), got {m.dtype}")
    if m.ndim != 2 or m.size == 0:
        raise ValueError(f"{who}: mask must be a non-empty [H, W] array, got shape {m.shape}")
    if m.size >= 1 << 31:
        raise ValueError(f"{who}: mask has {m.size} pixels; regions are labelled on fewer than 2**31")
    return np.ascontiguousarray(m != 0).view(np.uint8)


def _connectivity(connectivity, who):
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 (edge neighbours) or 8 (edge and corner neighbours), got {connectivity!r}")
    return int(connectivity)


def _region_table(table):
    """``lars_region`` rows -> ``area`` (int64), ``bbox`` (int32 ``[R, 4]``: row0, col0, row1, col1, half-open) and ``centroid``
    (float64 ``[R, 2]``: row, column), the quotient of the exact coordinate sums taken here in float64."""
    area = table["area"].astype(np.int64)
    centroid = np.stack((table["row_sum"].astype(np.float64) / area, table["col_sum"].astype(np.float64) / area), axis=-1)
    return {"area": area, "bbox": np.ascontiguousarray(table["bbox"], dtype=np.int32), "centroid": centroid.reshape(-1, 2)}


def _label_view(buffer, shape, label_bytes):
    """The ``[H, W]`` labels of the width the library chose, out of the int32-sized buffer it was handed."""
    dtype = {1: np.uint8, 2: np.uint16, 4: np.int32}[label_bytes]
    h, w = shape
    flat = buffer.reshape(-1).view(dtype)[:h * w].reshape(h, w)
    return flat if label_bytes == 4 else flat.copy()


def label_regions(mask, connectivity=8, min_pixels=1):
    """The connected regions of a foreground mask, labelled on the device (DESIGN.md "Zones from regions", csrc/regions.hip).

    ``mask``: a bool or integer ``[H, W]`` array, nonzero = foreground.  ``connectivity``: 4 (edge neighbours) or 8 (edge and corner
    neighbours).  A region is a maximal connected set of foreground pixels; regions are numbered ``1 .. R`` in raster order of their
    first pixel -- ``scipy.ndimage.label``'s numbering -- and those of fewer than ``min_pixels`` pixels become 0, the others keeping
    their order.  Returns ``{"labels", "n_regions", "area", "bbox", "centroid"}``: ``labels`` is uint8 for up to 255 regions, uint16
    for up to 65535, otherwise int32; ``area`` int64 ``[R]``; ``bbox`` int32 ``[R, 4]`` (row0, col0, row1, col1, half-open);
    ``centroid`` float64 ``[R, 2]`` (row, column).  No region is a result: ``n_regions`` 0 and empty arrays.  Integer arithmetic on
    the device: the same bytes on every run."""
    return _label_regions(mask, connectivity, min_pixels, "label_regions", False)


class _OutlineRoom:
    """The host arrays the tracer fills and the ``lars_outlines`` that names them: room for ``rings`` rows and ``verts`` vertices."""

    def __init__(self, rings, verts, tq=0):
        self.rings = np.empty(rings, dtype=_ffi.RING_DTYPE)
        self.verts = np.empty((verts, 2), dtype=np.int32)
        self.c = _ffi.Outlines(self.rings.ctypes.data, rings, self.verts.ctypes.data, verts, -1, -1, -1)
        self.tq, self.traced = tq, C.c_int64(-1)                   # with a tolerance: the ``_simplified`` entry points, which report the traced count

    def short(self):
        """Did the call end because the rings or vertices found do not fit?"""
        return self.c.n_rings > len(self.rings) or self.c.n_vertices > len(self.verts)

    def result(self, n_regions):
        """``"outlines"`` (a ``Polygons`` in pixel coordinates, or None where there is no region), ``"ring_area2"``, ``"n_rings"`` and
        ``"n_vertices"``.  The vertices stay in the order the device wrote them: (row, col) int32 becomes (x, y) float64."""
        q, v = self.c.n_rings, self.c.n_vertices
        table = self.rings[:q]
        out = {"outlines": None, "ring_area2": table["area2"].astype(np.int64), "n_rings": q, "n_vertices": v}
        if self.tq:
            out["n_vertices_traced"] = self.traced.value
        if n_regions:
            ring_starts = np.append(table["start"], np.int32(v)).astype(np.int32)
            poly_starts = np.searchsorted(table["label"], np.arange(1, n_regions + 2)).astype(np.int32)
            out["outlines"] = Polygons._packed(np.ascontiguousarray(self.verts[:v, ::-1], dtype=np.float64), ring_starts, poly_starts)
        return out


def _outline_argument(room):
    """The trailing ``lars_outlines *`` of the entry points that trace outlines, with the traced count and ``tq`` behind it for those
    that simplify: none for those that do not trace."""
    if not room:
        return ()
    return (C.byref(room.c), C.byref(room.traced), room.tq) if room.tq else (C.byref(room.c),)


def _outline_entry(name, room):
    """The entry point ``name`` that traces outlines, or its ``_simplified`` variant where the room has a tolerance."""
    if not (room and room.tq):
        return name
    return name[:-4] + "_simplified_f32" if name.endswith("_f32") else name + "_simplified"


def _outline_pixels(shape, who):
    if int(shape[0]) * int(shape[1]) >= OUTLINE_PIXELS_MAX:
        raise ValueError(f"{who}: the raster has {int(shape[0]) * int(shape[1])} pixels; outlines are traced on fewer than 2**29 (an edge id fits int32)")


def region_outlines(mask, connectivity=8, min_pixels=1, simplify=None):
    """``label_regions`` plus the outline of every region, traced on the device from the labels where they stand (DESIGN.md "Region
    outlines", csrc/outlines.hip).

    Returns ``label_regions``'s dict and ``"outlines"``: a ``Polygons`` in pixel coordinates, (x, y) = (column, row) float64 on the
    pixel corners, polygon ``k - 1`` = region ``k``; its first ring is the region's outer ring, clockwise on the screen, the others
    are its holes, counter-clockwise; rows and columns alternate along a ring and no vertex lies inside a straight run.  Under
    connectivity 8 a ring passes twice through a corner where the region touches itself diagonally; under 4 it turns there.
    ``"ring_area2"``: int64, the exact doubled signed area of each ring (positive: outer, negative: hole; a region's rings add up to
    twice its pixels), ``"n_rings"`` and ``"n_vertices"``.  ``rasterize_zones(result["outlines"], mask.shape)`` gives the labels back
    (up to 65535 regions).  No region: empty arrays and ``"outlines": None``.  Fewer than 2**29 pixels.  Integer arithmetic on the
    device: the same bytes on every run.

    ``simplify``: a tolerance in pixels, 0 to 254, quantised to sixteenths; None, 0 or a tolerance below 1/32 is no simplification and
    exactly the call above.  Otherwise every ring goes through Douglas-Peucker on the device before it comes down (DESIGN.md
    "Simplified outlines", csrc/outline_simplify.hip), as the chain from its first vertex back to it, the distance taken to the
    segment and compared in integers.  A ring whose result would have fewer than 3 vertices, no area or the other orientation stays
    as traced: rings, their order and their regions never change, nothing disappears.  ``"n_vertices"`` and ``"ring_area2"`` then
    describe the vertices written and ``"n_vertices_traced"`` is added.  ``rasterize_zones`` of simplified outlines no longer returns
    the labels; what holds in its place: every traced vertex lies within the tolerance of its ring.  The raster is at most 32767 a
    side."""
    return _label_regions(mask, connectivity, min_pixels, "region_outlines", True, simplify)


def _label_regions(mask, connectivity, min_pixels, who, want_outlines, simplify=None):
    """``label_regions``, and ``region_outlines`` where the outlines are wanted: one call, repeated with the room it reported where
    the first guess was short."""
    tq = _simplify_tq(simplify, who)
    if want_outlines and np.ndim(mask) == 2:
        _outline_pixels(np.shape(mask), who)                       # before anything is allocated
        if tq:
            _simplify_sides(np.shape(mask), who)
    m = _foreground(mask, who)
    connectivity = _connectivity(connectivity, who)
    min_pixels = _whole(min_pixels, "min_pixels", 1, (1 << 63) - 1, who)
    h, w = m.shape
    labels = np.empty((h, w), dtype=np.int32)
    # rows of the table: no more than there are foreground pixels, or pixels no two of which touch; a picture with more than 2**20
    # regions is labelled a second time with the room it asked for
    apart = ((h + 1) // 2) * ((w + 1) // 2) if connectivity == 8 else (h * w + 1) // 2
    foreground = int(np.count_nonzero(m))
    capacity = max(1, min(foreground, apart, 1 << 20))
    # a foreground pixel has four edges at most, a ring four at least: room that is never short, in pages nobody touches until they are
    # written, up to 2**22 rings and 2**24 vertices; a call that finds more is repeated with the room it reported
    rings, verts = max(1, min(foreground, 1 << 22)), max(4, min(4 * foreground, 1 << 24))
    while True:
        table = np.zeros(capacity, dtype=_ffi.REGION_DTYPE)
        room = _OutlineRoom(rings, verts, tq) if want_outlines else None
        count, width = C.c_int64(-1), C.c_int(0)
        try:
            _ffi.call(_outline_entry("lars_h_region_outlines", room) if room else "lars_h_label_regions", _ffi.ptr(m), h, w, connectivity, min_pixels, 0, _ffi.ptr(labels),
                      C.byref(width), _ffi.ptr(table), capacity, C.byref(count), *_outline_argument(room))
            break
        except _ffi.LarsError:
            if count.value > capacity:
                capacity = count.value
            elif room and room.short():
                rings, verts = max(rings, room.c.n_rings), max(verts, room.c.n_vertices)
            else:
                raise
    r = count.value
    return {"labels": _label_view(labels, (h, w), width.value), "n_regions": r, **_region_table(table[:r]), **(room.result(r) if room else {})}


class Regions:
    """Zones taken from the picture itself: ``Regions(mask=None, index=None, above=None, below=None, connectivity=8, min_pixels=1,
    max_regions=4096, want_labels=False, want_outlines=False, max_vertices=1 << 22, simplify=None)``, a third kind of ``zones`` beside a
    label raster and ``Polygons``.

    The foreground is a host ``mask`` (bool or integer ``[H, W]``, nonzero = foreground) or a threshold, ``above=t`` or ``below=t``,
    compared in float32 with the plane handed to ``zonal_statistics`` or with the ``index`` plane of ``process_image_zones``
    (required there, and among its ``indices``); exactly one of the three is given.  Pixels outside ``valid`` / nodata are never
    foreground.  The regions are ``label_regions``'s with ``connectivity`` and ``min_pixels``, made on the device; zone ``z`` is region
    ``z``.  ``max_regions`` (1 to 65535) is the room of the result arrays: more regions raise ``ValueError`` with their number.
    ``want_labels=True`` asks for the label raster as well.  ``want_outlines=True`` asks for the regions' outlines as
    ``region_outlines`` returns them (``"outlines"``, ``"ring_area2"``, ``"n_rings"``, ``"n_vertices"``), traced from the labels the
    zone stages used, on a raster of fewer than 2**29 pixels; ``max_vertices`` (4 to 2**31 - 1) is their room: more vertices raise
    ``ValueError`` with their number.  ``simplify``: the tolerance in pixels ``region_outlines`` takes, with what it says there; it needs
    ``want_outlines=True``, ``max_vertices`` is then the room of the vertices written, ``"n_vertices_traced"`` is added, and
    ``rasterize_zones`` of such outlines no longer returns the labels: every traced vertex lies within the tolerance of its ring.  Every
    check runs here, on the host."""

    def __init__(self, mask=None, index=None, above=None, below=None, connectivity=8, min_pixels=1, max_regions=4096, want_labels=False,
                 want_outlines=False, max_vertices=1 << 22, simplify=None):
        who = "Regions"
        given = [name for name, v in (("mask", mask), ("above", above), ("below", below)) if v is not None]
        if len(given) != 1:
            raise ValueError(f"{who}: exactly one of mask, above and below must be given, got {', '.join(given) or 'none of them'}")
        self.mask = _foreground(mask, who) if mask is not None else None
        if index is not None and index not in INDEX_IDS:
            raise ValueError(f"{who}: Unknown index type: {index}")
        if index is not None and mask is not None:
            raise ValueError(f"{who}: index names the plane a threshold is compared with; a mask needs none")
        self.index = index
        self.mode, self.threshold = 0, np.float32(0)
        if mask is None:
            t = above if above is not None else below
            if isinstance(t, (bool, np.bool_, str, bytes)) or not isinstance(t, (int, float, np.integer, np.floating)):
                raise TypeError(f"{who}: {given[0]} must be a number (got {type(t).__name__})")
            with np.errstate(over="ignore"):
                finite = bool(np.isfinite(np.float32(t)))
            if not finite:
                raise ValueError(f"{who}: {given[0]} must be finite in float32, got {t!r}")
            self.mode, self.threshold = (1 if above is not None else 2), np.float32(t)                # compared as the coverage count compares
        self.connectivity = _connectivity(connectivity, who)
        self.min_pixels = _whole(min_pixels, "min_pixels", 1, (1 << 63) - 1, who)
        self.max_regions = _whole(max_regions, "max_regions", 1, ZONES_MAX, who)
        self.want_labels = bool(want_labels)
        self.want_outlines = bool(want_outlines)
        self.max_vertices = _whole(max_vertices, "max_vertices", 4, (1 << 31) - 1, who)
        self.simplify_tq = _simplify_tq(simplify, who)
        if simplify is not None and not self.want_outlines:
            raise ValueError(f"{who}: simplify is the tolerance of the outlines: it needs want_outlines=True")

    def _check(self, shape, picture_indices, who):
        """What only the call knows: the mask's shape, and the plane of a threshold.  Returns the id of that plane."""
        if self.mask is not None and self.mask.shape != tuple(shape):
            raise ValueError(f"{who}: the Regions mask has shape {self.mask.shape}, the raster is {tuple(shape)}")
        if int(shape[0]) * int(shape[1]) >= 1 << 31:
            raise ValueError(f"{who}: the raster has {int(shape[0]) * int(shape[1])} pixels; regions are labelled on fewer than 2**31")
        if self.want_outlines:
            _outline_pixels(shape, who)
            if self.simplify_tq:
                _simplify_sides(shape, who)
        if picture_indices is None:
            if self.index is not None:
                raise ValueError(f"{who}: Regions(index={self.index!r}) names a plane of a picture; the threshold is compared with index_array here")
            return 0
        if self.mask is not None:
            return 0
        if self.index is None:
            raise ValueError(f"{who}: Regions needs index=, the plane above / below is compared with")
        if self.index not in picture_indices:
            raise ValueError(f"{who}: Regions(index={self.index!r}) is not among indices {list(picture_indices)}")
        return INDEX_IDS[self.index]

    def _outline_room(self):
        """Room for the outlines where they are wanted: a ring has four vertices or more, a simplified one three."""
        return _OutlineRoom(self.max_vertices // (3 if self.simplify_tq else 4), self.max_vertices, self.simplify_tq) if self.want_outlines else None


def _zone_source(zones, n_zones, who):
    """The split between the kinds of ``zones``.  None for what ``_labels`` has always taken -- an integer ndarray of two
    dimensions is a label raster -- and for everything it refuses; ``Polygons`` for outlines: a ``Polygons``, a list or tuple of
    polygons, or a float ``[Z, n, 2]`` array of single-ring polygons; a ``Regions`` as it stands."""
    if isinstance(zones, Regions):
        if n_zones is not None:
            raise ValueError(f"{who}: n_zones cannot be given with Regions: Z is the number of regions found")
        return zones
    if isinstance(zones, Polygons):
        polys = zones
    elif isinstance(zones, np.ndarray) and zones.dtype.kind == "f" and zones.ndim == 3 and zones.shape[2] == 2:
        polys = Polygons(zones, who=who)
    elif isinstance(zones, (list, tuple)):
        first = zones[0] if len(zones) else None
        nested = False
        rows_of_integers = (isinstance(first, (list, tuple)) and first and isinstance(first[0], (int, np.integer, bool, np.bool_))) or \
            (isinstance(first, np.ndarray) and first.ndim == 1 and first.dtype.kind in "uib")
        if rows_of_integers:
            try:
                as_array = np.asarray(zones)
                nested = as_array.ndim == 2 and as_array.dtype.kind in "uib"
            except ValueError:
                pass
        if nested:
            return None                                            # a label raster written as nested lists
        polys = Polygons(zones, who=who)
    else:
        return None
    if n_zones is not None:
        raise ValueError(f"{who}: n_zones cannot be given with polygons: Z = len(polygons) = {len(polys)}")
    return polys


def _raster_shape(shape, who):
    try:
        h, w = (int(v) for v in shape)
        ok = len(tuple(shape)) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in shape)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (1 <= h <= 1 << 24 and 1 <= w <= 1 << 24):
        raise ValueError(f"{who}: shape must be (H, W), two ints of 1 to 2**24, got {shape!r}")
    return h, w


def rasterize_zones(polygons, shape, transform=None):
    """The ``[H, W]`` label raster of plot outlines, made on the device: uint8 for up to 255 polygons, otherwise uint16.

    Pixel (row i, column j) has its centre at (j + 0.5, i + 0.5); it is inside a polygon iff a ray to its left crosses the polygon's
    pooled edges an odd number of times (even-odd, half-open: of two plots that share an edge exactly one takes each pixel).
    Polygon ``k`` writes ``k + 1``, the largest label wins, 0 is "in no polygon"; a polygon that covers no pixel centre is an empty
    zone.  ``polygons`` and ``transform``: see ``Polygons``.  The result is the definition bit for bit on every run, and equals what
    ``process_image_zones`` / ``zonal_statistics`` use when they are handed the same polygons."""
    who = "rasterize_zones"
    polys = polygons if isinstance(polygons, Polygons) and transform is None else Polygons(polygons, transform, who=who)
    h, w = _raster_shape(shape, who)
    labels = polys._label_buffer((h, w))
    _ffi.call("lars_h_rasterize_zones", *polys._head(), h, w, labels.dtype.itemsize, _ffi.ptr(labels))
    return labels


def shrink_zones(zones, margin, shape=None, transform=None, n_zones=None):
    """The ``[H, W]`` label raster of ``zones`` with every zone shrunk inward by ``margin`` pixels, made on the device (DESIGN.md "Zone
    margins", csrc/zone_margin.hip): what ``zonal_statistics`` / ``process_image_zones`` take their figures from when they are handed
    ``Shrunk(zones, margin)``.

    A pixel keeps its label iff every pixel of the raster with another label -- background, another zone -- is further than
    ``margin`` from it, centre to centre; otherwise it becomes 0.  Outside the raster there are no pixels: the raster's edge shrinks
    nothing.  ``margin`` is a number of pixels, 0 to 254: below 1 nothing goes, 1 takes the 4-connected border layer, ``sqrt(2)`` the
    8-connected one.  A zone may vanish or fall into pieces that keep its label; Z does not change.  ``zones``: a label raster as
    ``zonal_statistics`` takes it (``shape`` must not be given; the result has its dtype; ``n_zones`` as there), or polygons as
    ``rasterize_zones`` takes them with ``shape`` and ``transform`` (the result has its dtype; the labels never cross PCIe before
    they are shrunk).  Integer arithmetic on the device: the same bytes on every run."""
    who = "shrink_zones"
    m2 = _margin2(margin, who)
    if isinstance(zones, (Regions, Shrunk)):
        raise TypeError(f"{who}: zones must be a label raster or polygons, got {type(zones).__name__}")
    raster_like = isinstance(zones, np.ndarray) and zones.dtype.kind in "uib"
    if transform is not None and not raster_like:
        if n_zones is not None:
            raise ValueError(f"{who}: n_zones cannot be given with polygons: Z = len(polygons)")
        source = Polygons(zones, transform, who=who)
    else:
        source = _zone_source(zones, n_zones, who)
    if source is None:
        if shape is not None or transform is not None:
            raise ValueError(f"{who}: shape and transform belong to polygons; a label raster has its own shape")
        given = np.asarray(zones)
        if given.ndim != 2:
            raise ValueError(f"{who}: zones must be an [H, W] array of labels, got shape {given.shape}")
        lab, rows = _labels(given, given.shape, n_zones, who)
        out, bad = np.empty_like(lab), C.c_int64(-1)
        h, w = lab.shape
        try:
            _ffi.call("lars_h_shrink_zones", _ffi.ptr(lab), lab.dtype.itemsize, h, w, rows, m2, _ffi.ptr(out), C.byref(bad))
        except _ffi.LarsError:
            if bad.value > 0:
                raise ValueError(f"{who}: {bad.value} pixels have a label outside 0 .. {rows}") from None
            raise
        return out if out.dtype == given.dtype else out.astype(given.dtype)
    if shape is None:
        raise ValueError(f"{who}: shape is required with polygons: (H, W) of the raster")
    h, w = _raster_shape(shape, who)
    labels = source._label_buffer((h, w))
    _ffi.call("lars_h_rasterize_zones_margin", *source._head(), h, w, labels.dtype.itemsize, _ffi.ptr(labels), m2)
    return labels


def simplify_outlines(result, tolerance):
    """The outlines of an earlier call with fewer vertices: ``region_outlines(..., simplify=tolerance)``'s rings from the rings of
    ``region_outlines(...)``, on the device (DESIGN.md "Simplified outlines", csrc/outline_simplify.hip).

    ``result``: the dict of ``region_outlines``, of ``zonal_statistics`` or of ``process_image_zones`` with outlines (there the
    ``"zones"`` part is the one that changes).  A copy comes back whose ``"outlines"``, ``"ring_area2"`` and ``"n_vertices"`` describe
    the vertices written, with ``"n_vertices_traced"`` added; everything else is shared.  The vertices must be whole numbers of 0 to
    32767.  A tolerance of None, 0 or below 1/32 changes nothing: the copy has the keys and arrays it was given.  ``rasterize_zones`` of
    simplified outlines no longer returns the labels; every vertex given lies within the tolerance of its ring."""
    who = "simplify_outlines"
    if not isinstance(result, dict):
        raise TypeError(f"{who}: result must be the dict of region_outlines or of a zone call with outlines, got {type(result).__name__}")
    if "zones" in result and isinstance(result["zones"], dict) and "outlines" in result["zones"]:
        return {**result, "zones": simplify_outlines(result["zones"], tolerance)}
    if "outlines" not in result or "ring_area2" not in result:
        raise ValueError(f"{who}: this result holds no outlines (region_outlines, or Regions(want_outlines=True), returns them)")
    tq = _simplify_tq(tolerance, who)
    polys = result["outlines"]
    if tq == 0 or polys is None:
        return dict(result)
    if not isinstance(polys, Polygons):
        raise TypeError(f"{who}: result['outlines'] must be a Polygons, got {type(polys).__name__}")
    xy = polys.verts
    if not (np.isfinite(xy).all() and (xy == np.floor(xy)).all() and (xy >= 0).all() and (xy <= SIMPLIFY_SIDE_MAX).all()):
        raise ValueError(f"{who}: the vertices must be whole numbers of 0 to {SIMPLIFY_SIDE_MAX}: pixel corners, as region_outlines writes them")
    q, v = len(polys.ring_starts) - 1, len(xy)
    area2 = np.asarray(result["ring_area2"])
    if area2.shape != (q,):
        raise ValueError(f"{who}: ring_area2 has shape {area2.shape} for {q} rings")
    rings = np.zeros(q, dtype=_ffi.RING_DTYPE)
    rings["label"] = np.repeat(np.arange(1, len(polys) + 1, dtype=np.int32), np.diff(polys.poly_starts))
    rings["start"], rings["count"], rings["area2"] = polys.ring_starts[:-1], np.diff(polys.ring_starts), area2
    verts = np.ascontiguousarray(xy[:, ::-1], dtype=np.int32)
    rings_out, verts_out = np.empty(q, dtype=_ffi.RING_DTYPE), np.empty((v, 2), dtype=np.int32)
    counts = (C.c_int64 * 3)(-1, -1, -1)
    _ffi.call("lars_h_outline_simplify", _ffi.ptr(rings), q, _ffi.ptr(verts), v, tq, SIMPLIFY_SIDE_MAX, SIMPLIFY_SIDE_MAX, _ffi.ptr(rings_out),
              _ffi.ptr(verts_out), v, C.byref(counts), None)
    written = counts[1]
    ring_starts = np.append(rings_out["start"], np.int32(written)).astype(np.int32)
    outlines = Polygons._packed(np.ascontiguousarray(verts_out[:written, ::-1], dtype=np.float64), ring_starts, polys.poly_starts)
    return {**result, "outlines": outlines, "ring_area2": rings_out["area2"].astype(np.int64), "n_vertices": written, "n_vertices_traced": v}


def _geometry_rings(geom, where):
    kind = geom.get("type") if isinstance(geom, dict) else None
    if kind == "Polygon":
        parts = [geom.get("coordinates")]
    elif kind == "MultiPolygon":
        parts = geom.get("coordinates")
    else:
        raise ValueError(f"polygons_from_geojson: {where}: geometry type {kind!r} is no Polygon or MultiPolygon")
    rings = []
    for part in parts or []:
        for ring in part or []:
            a = np.asarray(ring, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] < 2:
                raise ValueError(f"polygons_from_geojson: {where}: a ring must be a list of [x, y] positions, got shape {a.shape}")
            rings.append(np.ascontiguousarray(a[:, :2]))
    if not rings:
        raise ValueError(f"polygons_from_geojson: {where}: the {kind} has no ring")
    return rings


def _collect(obj, where, out):
    kind = obj.get("type") if isinstance(obj, dict) else None
    if kind == "FeatureCollection":
        for i, feature in enumerate(obj.get("features") or []):
            _collect(feature, f"feature {i}", out)
    elif kind == "Feature":
        if obj.get("geometry") is None:
            raise ValueError(f"polygons_from_geojson: {where}: the feature has no geometry")
        _collect(obj["geometry"], where, out)
    elif kind == "GeometryCollection":
        for i, geom in enumerate(obj.get("geometries") or []):
            _collect(geom, f"{where}, geometry {i}" if where else f"geometry {i}", out)
    else:
        out.append(_geometry_rings(obj, where or "the object"))


def polygons_from_geojson(obj_or_path):
    """The polygons of a GeoJSON object (a dict) or file (a path): ``Polygon``, ``MultiPolygon``, ``Feature``, ``FeatureCollection``
    and ``GeometryCollection``.  One polygon per geometry, in file order -- so label ``k + 1`` is the ``k``-th of them -- as a list of
    lists of ``[n, 2]`` float64 rings; the parts of a ``MultiPolygon`` are pooled into one polygon, a third coordinate is dropped.
    Any other geometry type raises ``ValueError`` with the feature's position.  Host JSON only: the coordinates are returned as they
    stand (``transform=`` maps world coordinates to pixels)."""
    if isinstance(obj_or_path, dict):
        obj = obj_or_path
    elif isinstance(obj_or_path, (str, os.PathLike)):
        with open(obj_or_path, encoding="utf-8") as f:
            obj = json.load(f)
    else:
        raise TypeError(f"polygons_from_geojson: a GeoJSON dict or a path is needed, got {type(obj_or_path).__name__}")
    out = []
    _collect(obj, "", out)
    if not out:
        raise ValueError("polygons_from_geojson: no geometry in this object")
    return out


def polygons_to_geojson(polygons, transform=None, properties=None):
    """A GeoJSON ``FeatureCollection`` dict of polygons: one ``Polygon`` feature per polygon, its rings in the order held, each closed
    by repeating its first vertex.

    ``polygons``: a ``Polygons`` (``region_outlines``'s ``"outlines"``) or anything ``Polygons`` takes, in pixel coordinates.
    ``transform``: the six numbers of a GDAL geotransform; the coordinates then go through ``to_world``.  ``properties``: a list of
    one dict per polygon, or None for empty ones.  ``polygons_from_geojson`` reads the result back ring for ring, the closing vertex
    included (it returns rings as they stand, and a repeated vertex changes no label of ``rasterize_zones``).

    Rings are not reversed.  ``region_outlines`` writes outer rings clockwise as the eye sees them on the screen and holes
    counter-clockwise, and a north-up transform (``dy < 0``) shows the same picture: on the map they still run clockwise, their
    shoelace sum with Y upwards is negative.  RFC 7946 recommends the other order (outer rings counter-clockwise) and asks readers not
    to reject this one; a reader that insists wants every ring reversed.  Under connectivity 8 an outer ring may touch itself at a
    corner: some readers call such a ring invalid; connectivity 4 never writes one."""
    who = "polygons_to_geojson"
    polys = polygons if isinstance(polygons, Polygons) else Polygons(polygons, who=who)
    if properties is not None:
        properties = list(properties)
        if len(properties) != len(polys) or not all(isinstance(p, dict) for p in properties):
            raise ValueError(f"{who}: properties must be a list of {len(polys)} dicts, one per polygon")
    verts = polys.verts if transform is None else to_world(polys.verts, transform)
    features = []
    for k in range(len(polys)):
        rings = []
        for r in range(polys.poly_starts[k], polys.poly_starts[k + 1]):
            ring = verts[polys.ring_starts[r]:polys.ring_starts[r + 1]]
            rings.append(ring.tolist() + [ring[0].tolist()])
        features.append({"type": "Feature", "properties": dict(properties[k]) if properties is not None else {},
                         "geometry": {"type": "Polygon", "coordinates": rings}})
    return {"type": "FeatureCollection", "features": features}


class _RasterZones:
    """The zones of one call, of the three kinds below: ``rows`` to allocate for each index, the entry point of a ``plane`` and of a
    ``picture``, the kind's arguments in the layout of either (``plane_args``, and ``picture_args`` behind the picture's own),
    ``explain()`` -- the ``ValueError`` of this kind for a call that failed, or None -- and ``finish()`` -> (Z, the extra keys).

    This one: a label raster, checked (``_labels``)."""
    plane, picture = "lars_h_zonal_stats_f32", "lars_h_process_image_zones"

    def __init__(self, zones, shape, n_zones, who):
        self.who, self.bad = who, C.c_int64(-1)
        self.lab, self.rows = _labels(zones, shape, n_zones, who)

    def plane_args(self, x, valid, h, w, threshold, want_hist, records, medians):
        return (x, _ffi.ptr(self.lab), self.lab.dtype.itemsize, valid, h, w, self.rows, threshold, want_hist, records, medians, C.byref(self.bad))

    def picture_args(self, records, medians):
        return (_ffi.ptr(self.lab), self.lab.dtype.itemsize, self.rows, records, medians, C.byref(self.bad))

    def explain(self):
        if self.bad.value > 0:
            return ValueError(f"{self.who}: {self.bad.value} pixels have a label outside 0 .. {self.rows}")

    def finish(self):
        return self.rows, {}


class _PolygonZones:
    """... ``Polygons``: the labels are made on the device and come back where they are wanted."""
    plane, picture = "lars_h_zonal_stats_polygons_f32", "lars_h_process_image_zones_polygons"

    def __init__(self, polys, shape):
        self.polys, self.rows = polys, len(polys)
        self.made = polys._label_buffer(shape) if polys.want_labels else None
        self.tail = (_ffi.ptr(self.made), self.made.dtype.itemsize if polys.want_labels else 0)

    def plane_args(self, x, valid, h, w, threshold, want_hist, records, medians):
        return (x, *self.polys._head(), valid, h, w, threshold, want_hist, records, medians, *self.tail)

    def picture_args(self, records, medians):
        return (*self.polys._head(), records, medians, *self.tail)

    def explain(self):
        return None

    def finish(self):
        return self.rows, ({"labels": self.made} if self.made is not None else {})


class _RegionZones:
    """... ``Regions``: Z is known once the labels exist, ``max_regions`` rows are allocated; the table, the labels and the outlines
    come back with it.  ``picture_indices``: None for a plane."""

    def __init__(self, regions, shape, picture_indices, who):
        self.regions, self.shape, self.who, self.rows = regions, shape, who, regions.max_regions
        self.source = regions._check(shape, picture_indices, who)
        self.table = np.zeros(self.rows, dtype=_ffi.REGION_DTYPE)
        self.made = np.empty(shape, dtype=np.int32) if regions.want_labels else None
        self.found, self.width = C.c_int64(-1), C.c_int(0)
        self.room = regions._outline_room()
        self.plane = _outline_entry("lars_h_zonal_stats_regions_outlines_f32", self.room) if self.room else "lars_h_zonal_stats_regions_f32"
        self.picture = _outline_entry("lars_h_process_image_regions_outlines", self.room) if self.room else "lars_h_process_image_regions"
        self.foreground = (_ffi.ptr(regions.mask), regions.mode, regions.threshold, regions.connectivity, regions.min_pixels)

    def _tail(self, records, medians):
        return (self.rows, records, medians, _ffi.ptr(self.table), C.byref(self.found), _ffi.ptr(self.made), 0, C.byref(self.width),
                *_outline_argument(self.room))

    def plane_args(self, x, valid, h, w, threshold, want_hist, records, medians):
        return (x, *self.foreground, valid, h, w, threshold, want_hist, *self._tail(records, medians))

    def picture_args(self, records, medians):
        return (self.foreground[0], self.source, *self.foreground[1:], *self._tail(records, medians))

    def explain(self):
        r = self.regions
        if self.found.value > self.rows:
            return ValueError(f"{self.who}: {self.found.value} regions, more than max_regions = {r.max_regions}: raise min_pixels to drop the small "
                              f"ones, or max_regions (at most {ZONES_MAX} regions make one label raster)")
        if self.room and self.room.short():
            return ValueError(f"{self.who}: the outlines have {self.room.c.n_vertices} vertices, more than max_vertices = {r.max_vertices}: raise "
                              f"min_pixels to drop the small regions, or max_vertices")

    def finish(self):
        nz = self.found.value
        extra = {"regions": _region_table(self.table[:nz]), **(self.room.result(nz) if self.room else {})}
        if self.made is not None:
            extra["labels"] = _label_view(self.made, self.shape, self.width.value)
        return nz, extra


def _zones_of_call(zones, n_zones, shape, picture_indices, who):
    source = _zone_source(zones, n_zones, who)
    if isinstance(source, Regions):
        return _RegionZones(source, shape, picture_indices, who)
    return _PolygonZones(source, shape) if source is not None else _RasterZones(zones, shape, n_zones, who)


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
    ``zones`` may be ``Shrunk(zones, margin)``: every zone is then shrunk inward by ``margin`` pixels before its figures are taken.
    Everything but ``mean`` is bit-reproducible; the mean's double sum follows the order the device placed the values in."""
    who = "zonal_statistics"
    if index_type not in INDEX_IDS:
        raise ValueError(f"{who}: Unknown index type: {index_type}")
    zones, margin2 = _unshrunk(zones)
    x = np.asarray(index_array)
    if x.dtype != np.float32:
        raise TypeError(f"{who}: index_array must be float32 (got {x.dtype})")
    if x.ndim != 2 or x.size == 0:
        raise ValueError(f"{who}: index_array must be a non-empty [H, W] array, got shape {x.shape}")
    h, w = x.shape
    z = _zones_of_call(zones, n_zones, (h, w), None, who)
    if isinstance(valid, str):
        raise TypeError(f"{who}: valid must be an [H, W] bool or integer array or None: a plane has no alpha channel")
    valid_arr, _ = _nodata.valid_argument(valid, (h, w, 0), who)
    _, threshold = _coverage_rule(index_type)
    x = np.ascontiguousarray(x)
    records = np.zeros(z.rows, dtype=_ffi.STATS_DTYPE)
    medians = np.zeros((z.rows, 2), dtype=np.float32)
    try:
        name, args = _margin_entry(z.plane, z.plane_args(_ffi.ptr(x), _ffi.ptr(valid_arr), h, w, np.float32(threshold), int(bool(want_hist)),
                                                         _ffi.ptr(records), _ffi.ptr(medians)), margin2)
        _ffi.call(name, *args)
    except _ffi.LarsError:
        explained = z.explain()
        if explained is None:
            raise
        raise explained from None
    nz, extra = z.finish()
    count, out = _figures(records[:nz], medians[:nz], want_hist)
    return {"zone": np.arange(1, nz + 1, dtype=np.int64), "pixels": count, **out, **extra}


def process_image_zones(img_array, zones, valid=None, nodata=None, n_zones=None, indices=_ffi.INDEX_NAMES, white_balance=True,
                        want_arrays=True, want_hist=False, want_rgba=False):
    """``process_image_masked`` plus one row per zone: its dict with ``"zones": {"zone", "pixels", t: {mean, median, min, max,
    coverage[, hist]}}`` added.

    The picture crosses PCIe once, the white balance is taken over the whole valid picture -- zones do not change which pixels its
    percentiles see -- and one pass sorts every valid pixel's index value into its zone.  ``corrected``, the planes, ``rgba``, the
    picture-level statistics and ``valid_pixels`` are exactly ``process_image_masked``'s with the same ``valid`` / ``nodata``; the
    zone figures are ``zonal_statistics``'s of each plane under the derived mask, ``Shrunk(zones, margin)`` as there.  At least one
    index must be asked for."""
    who = "process_image_zones"
    zones, margin2 = _unshrunk(zones)
    p = _picture(who, who, img_array, list(indices), white_balance, want_arrays, bool(want_hist), want_rgba, False, valid, nodata,
                 need_index="zone statistics need at least one index")
    indices = p.indices
    z = _zones_of_call(zones, n_zones, (p.h, p.w), indices, who)
    records = np.zeros((3, z.rows), dtype=_ffi.STATS_DTYPE)
    medians = np.zeros((3, z.rows, 2), dtype=np.float32)
    nvalid = C.c_int64(-1)
    p_rgba, p_lut = _ffi.ptr3(p.rgbas), _ffi.ptr3(p.luts)
    try:
        name, args = _margin_entry(z.picture, (*p.head, C.byref(p_rgba), C.byref(p_lut), _ffi.ptr(p.valid), int(p.use_alpha), int(p.nodata is not None),
                                               p.nodata or 0, C.byref(nvalid), *z.picture_args(_ffi.ptr(records), _ffi.ptr(medians))), margin2)
        _ffi.call(name, *args)
    except _ffi.LarsError:
        explained = ValueError("process_image: no valid pixel") if nvalid.value == 0 else z.explain()
        if explained is None:
            raise
        raise explained from None
    result = _picture_result(p, want_hist, want_rgba, False, valid_pixels=nvalid.value)
    nz, extra = z.finish()
    result["zones"] = {"zone": np.arange(1, nz + 1, dtype=np.int64), **extra}
    for t in indices:
        result["zones"]["pixels"], result["zones"][t] = _figures(records[INDEX_IDS[t], :nz], medians[INDEX_IDS[t], :nz], want_hist)
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
