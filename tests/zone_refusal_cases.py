"""What the zone entry points refuse, as a table: for each kind of zones (a label raster, polygons, regions with or without outlines)
the good arguments of a 4 x 5 raster and one row per fault -- (the arguments changed, the exact message) -- in the order the library
checks them.  test_zone_refusals_cpu.py takes the rows through the picture entry points, which answer before they touch a device;
test_gpu_zone_refusals.py through the plane entry points, which open the device first.

Arguments carry the same name wherever they mean the same: ``zone_stats`` / ``zone_medians`` are a plane call's ``stats`` /
``medians``, ``labels_out`` / ``label_bytes`` are ``lars_h_rasterize_zones``'s ``labels`` / ``zone_bytes``.  A refused call reads no
element of an array: a row may name a length with a tiny array behind it where its check fires before any element is read (the
order is the library's, csrc/host_zones.cpp)."""
import ctypes as C

import numpy as np

from lars_image_processing_amd import _ffi

H, W = 4, 5
KEPT = 7                                 # what every out-parameter holds before a call: a refusal that leaves it alone leaves 7
ZONES_MAX, VERTS_MAX = 65535, 1 << 24


class Off:
    """The address ``n`` bytes into ``arr``: a pointer that is not aligned, never followed."""

    def __init__(self, arr, n):
        self.arr, self.n = arr, n


class Ptr3:
    """``void *[3]`` of three optional arrays."""

    def __init__(self, *arrs):
        self.arrs = arrs


def outlines(rings=8, verts=64,ring_ptr=True, vert_ptr=True, ring_off=0, vert_off=0):
    """A ``lars_outlines`` with room for ``rings`` rows and ``verts`` vertices and KEPT in its three counts; the arrays hang on it."""
    o = _ffi.Outlines()
    o.ring_rows, o.vert_rows = np.zeros(max(rings, 1) + 1, dtype=_ffi.RING_DTYPE), np.zeros((max(verts, 1) + 1, 2), dtype=np.int32)
    o.rings = o.ring_rows.ctypes.data + ring_off if ring_ptr else None
    o.verts = o.vert_rows.ctypes.data + vert_off if vert_ptr else None
    o.ring_capacity, o.vert_capacity = rings, verts
    o.n_rings = o.n_vertices = o.n_edges = KEPT
    return o


def counts_of(o):
    return (o.n_rings, o.n_vertices, o.n_edges)


# ---- the good arguments ----
ZONES = np.array([[0, 1, 1, 0, 2], [1, 1, 0, 2, 2], [0, 0, 0, 2, 2], [1, 1, 0, 0, 0]], dtype=np.uint8)
SQUARES = [np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]]), np.array([[3.0, 1.0], [5.0, 1.0], [5.0, 4.0], [3.0, 4.0]])]
MASK = (ZONES != 0).astype(np.uint8)


def plane():
    return np.linspace(-1, 1, H * W, dtype=np.float32).reshape(H, W)


def raster_arguments():
    return {"zones": ZONES.copy(), "zone_bytes": 1, "nzones": 2, "zone_stats": np.zeros((3, 2), dtype=_ffi.STATS_DTYPE),
            "zone_medians": np.zeros((3, 2, 2), dtype=np.float32), "bad_labels": C.c_int64(KEPT)}


def polygon_arguments():
    return {"verts": np.concatenate(SQUARES), "nverts": 8, "ring_starts": np.array([0, 4, 8], dtype=np.int32), "nrings": 2,
            "poly_starts": np.array([0, 1, 2], dtype=np.int32), "npolys": 2, "zone_stats": np.zeros((3, 2), dtype=_ffi.STATS_DTYPE),
            "zone_medians": np.zeros((3, 2, 2), dtype=np.float32), "labels_out": np.zeros((H, W), dtype=np.uint8), "label_bytes": 1}


def region_arguments(with_outlines):
    a = {"mask": MASK.copy(), "source_index": 0, "mode": 0, "t": 0.0, "connectivity": 8, "min_pixels": 1, "capacity": 8,
         "zone_stats": np.zeros((3, 8), dtype=_ffi.STATS_DTYPE), "zone_medians": np.zeros((3, 8, 2), dtype=np.float32),
         "table": np.zeros(8, dtype=_ffi.REGION_DTYPE), "n_regions": C.c_int64(KEPT), "labels_out": np.zeros((H, W), dtype=np.int32),
         "label_bytes": 0, "label_bytes_out": C.c_int(KEPT)}
    if with_outlines:
        a["outlines"] = outlines()
    return a


# ---- the faults: name -> (the arguments changed, the message behind "<entry point>: "), in the order of the checks ----
RASTER_FAULTS = {
    "zones_null": ({"zones": None}, "zones, their records and their medians are required"),
    "records_null": ({"zone_stats": None}, "zones, their records and their medians are required"),
    "medians_null": ({"zone_medians": None}, "zones, their records and their medians are required"),
    "zone_bytes_3": ({"zone_bytes": 3}, "labels are 1, 2 or 4 bytes wide, got 3"),
    "zone_bytes_0": ({"zone_bytes": 0}, "labels are 1, 2 or 4 bytes wide, got 0"),
    "nzones_0": ({"nzones": 0}, "1 to 65535 zones, got 0"),
    "nzones_65536": ({"nzones": 65536}, "1 to 65535 zones, got 65536"),
    # two faults: the earlier check answers
    "zones_null_and_zone_bytes_3": ({"zones": None, "zone_bytes": 3}, "zones, their records and their medians are required"),
    "zone_bytes_3_and_nzones_0": ({"zone_bytes": 3, "nzones": 0}, "labels are 1, 2 or 4 bytes wide, got 3"),
}

_STARTS = "poly_starts must run from 0 to nrings and ring_starts from 0 to nverts"
_RINGS = "{} polygons need as many rings or more (got {}) of three vertices or more each (got {} in all, at most 16777216)"
_I32 = lambda *v: np.array(v, dtype=np.int32)                                               # noqa: E731
POLYGON_FAULTS = {
    "verts_null": ({"verts": None}, "verts, ring_starts and poly_starts are required"),
    "ring_starts_null": ({"ring_starts": None}, "verts, ring_starts and poly_starts are required"),
    "poly_starts_null": ({"poly_starts": None}, "verts, ring_starts and poly_starts are required"),
    "npolys_0": ({"npolys": 0}, "1 to 65535 polygons, got 0"),
    "npolys_65536": ({"npolys": 65536}, "1 to 65535 polygons, got 65536"),
    "fewer_rings_than_polygons": ({"nrings": 1}, _RINGS.format(2, 1, 8)),
    "fewer_than_three_vertices_a_ring": ({"nverts": 5}, _RINGS.format(2, 2, 5)),
    "vertices_above_the_ceiling": ({"nverts": VERTS_MAX + 1}, _RINGS.format(2, 2, VERTS_MAX + 1)),     # fires before any element is read
    "label_bytes_3": ({"label_bytes": 3}, "labels come back 1, 2 or 4 bytes wide, got 3"),
    "labels_misaligned": ({"labels_out": Off(np.zeros(H * W + 2, dtype=np.uint16), 1), "label_bytes": 2},
                          "2 labels do not fit 2-byte labels, or the labels are not aligned"),
    # 256 polygons in one byte: refused before poly_starts[256] is read
    "one_byte_for_256_polygons": ({"npolys": 256, "nrings": 256, "nverts": 768}, "256 labels do not fit 1-byte labels, or the labels are not aligned"),
    "poly_starts_from_1": ({"poly_starts": _I32(1, 1, 2)}, _STARTS),
    "poly_starts_end_short": ({"poly_starts": _I32(0, 1, 1)}, _STARTS),
    "ring_starts_from_1": ({"ring_starts": _I32(1, 4, 8)}, _STARTS),
    "ring_starts_end_short": ({"ring_starts": _I32(0, 4, 7)}, _STARTS),
    "polygon_0_without_ring": ({"poly_starts": _I32(0, 0, 2)}, "polygon 0 has no ring (poly_starts must rise)"),
    "polygon_1_without_ring": ({"poly_starts": _I32(0, 2, 2)}, "polygon 1 has no ring (poly_starts must rise)"),
    "polygon_0_beyond_the_rings": ({"poly_starts": _I32(0, 3, 2)}, "polygon 0 has no ring (poly_starts must rise)"),
    "ring_0_of_two_vertices": ({"ring_starts": _I32(0, 2, 8)}, "ring 0 has fewer than three vertices (ring_starts must rise by three or more)"),
    "ring_1_of_two_vertices": ({"ring_starts": _I32(0, 6, 8)}, "ring 1 has fewer than three vertices (ring_starts must rise by three or more)"),
    # two faults
    "npolys_0_and_label_bytes_3": ({"npolys": 0, "label_bytes": 3}, "1 to 65535 polygons, got 0"),
    "label_bytes_3_and_poly_starts_from_1": ({"label_bytes": 3, "poly_starts": _I32(1, 1, 2)}, "labels come back 1, 2 or 4 bytes wide, got 3"),
}


def _with(verts, at, value):
    out = np.array(verts, dtype=np.float64)
    out[at] = value
    return out


_COORD = "vertex {} has a coordinate that is not finite or beyond 1e9 in size"
POLYGON_FAULTS["vertex_5_nan"] = ({"verts": _with(np.concatenate(SQUARES), (5, 1), np.nan)}, _COORD.format(5))
POLYGON_FAULTS["vertex_0_inf"] = ({"verts": _with(np.concatenate(SQUARES), (0, 0), -np.inf)}, _COORD.format(0))
POLYGON_FAULTS["vertex_7_beyond_1e9"] = ({"verts": _with(np.concatenate(SQUARES), (7, 0), 1.5e9)}, _COORD.format(7))
POLYGON_FAULTS["ring_of_two_vertices_and_vertex_nan"] = ({"ring_starts": _I32(0, 2, 8), "verts": _with(np.concatenate(SQUARES), (5, 1), np.nan)},
                                                         "ring 0 has fewer than three vertices (ring_starts must rise by three or more)")
# the raster's own limit, for the calls that take h and w beside the polygons: nothing of h x w is read
POLYGON_RASTER = "the raster is 1 to 2^24 on each side"

_TABLE = "a table of capacity 1 to {most} and n_regions are required, got {}"
_ROOM = "the outlines need a ring table and a vertex array of capacity >= 0, 8- and 4-byte aligned"
REGION_FAULTS = {
    "connectivity_5": ({"connectivity": 5}, "connectivity must be 4 or 8, got 5"),
    "connectivity_0": ({"connectivity": 0}, "connectivity must be 4 or 8, got 0"),
    "min_pixels_0": ({"min_pixels": 0}, "min_pixels must be 1 or more, got 0"),
    "capacity_0": ({"capacity": 0}, _TABLE.format(0, most="{most}")),
    "capacity_above_the_most": ({"capacity": "most + 1"}, _TABLE.format("{over}", most="{most}")),
    "table_null": ({"table": None}, _TABLE.format(8, most="{most}")),
    "n_regions_null": ({"n_regions": None}, _TABLE.format(8, most="{most}")),
    "label_bytes_3": ({"label_bytes": 3}, "labels come back 1, 2 or 4 bytes wide (0: the narrowest), got 3"),
    "labels_misaligned": ({"labels_out": Off(np.zeros(H * W + 1, dtype=np.int32), 2)}, "the labels are not aligned"),
    # two faults
    "label_bytes_3_and_connectivity_5": ({"label_bytes": 3, "connectivity": 5}, "connectivity must be 4 or 8, got 5"),
    "min_pixels_0_and_capacity_0": ({"min_pixels": 0, "capacity": 0}, "min_pixels must be 1 or more, got 0"),
    "capacity_0_and_labels_misaligned": ({"capacity": 0, "labels_out": Off(np.zeros(H * W + 1, dtype=np.int32), 2)}, _TABLE.format(0, most="{most}")),
}
# with a plane to threshold instead of a mask (not lars_h_label_regions / lars_h_region_outlines, which need the mask)
REGION_MODE_FAULTS = {
    "no_mask_and_mode_0": ({"mask": None, "mode": 0}, "a mask, or mode 1 (above t) or 2 (below t), is required"),
    "no_mask_and_mode_3": ({"mask": None, "mode": 3}, "a mask, or mode 1 (above t) or 2 (below t), is required"),
    "no_mask_mode_3_and_connectivity_5": ({"mask": None, "mode": 3, "connectivity": 5}, "a mask, or mode 1 (above t) or 2 (below t), is required"),
}
# the checks of the outline room come last and set the three counts to -1 first: after these rows the counts are -1, after the rows
# above they are what they were
OUTLINE_FAULTS = {
    "ring_capacity_below_0": (lambda: {"outlines": outlines(rings=-1)}, _ROOM),
    "vert_capacity_below_0": (lambda: {"outlines": outlines(verts=-1)}, _ROOM),
    "rings_null_with_room": (lambda: {"outlines": outlines(ring_ptr=False)}, _ROOM),
    "verts_null_with_room": (lambda: {"outlines": outlines(vert_ptr=False)}, _ROOM),
    "rings_misaligned": (lambda: {"outlines": outlines(ring_off=4)}, _ROOM),
    "verts_misaligned": (lambda: {"outlines": outlines(vert_off=2)}, _ROOM),
    "label_bytes_3_and_rings_null": (lambda: {"outlines": outlines(ring_ptr=False), "label_bytes": 3},
                                     "labels come back 1, 2 or 4 bytes wide (0: the narrowest), got 3"),
}
REGION_RASTER = "the raster is 1 or more on each side and has fewer than 2^31 pixels"
OUTLINE_RASTER = "outlines are traced on fewer than 2^29 pixels (an edge id fits int32), got {} x {}"


def region_faults(with_outlines, most, needs_mask=False):
    """name -> (changes, message, the outline counts afterwards or None) for an entry point whose table holds ``most`` rows at most."""
    rows = dict(REGION_FAULTS)
    if not needs_mask:
        rows.update(REGION_MODE_FAULTS)
    out = {}
    for name, (change, text) in rows.items():
        change = {k: (most + 1 if isinstance(v, str) else v) for k, v in change.items()}
        out[name] = (change, text.format(most=most, over=most + 1), (KEPT,) * 3 if with_outlines else None)
    if with_outlines:
        for name, (change, text) in OUTLINE_FAULTS.items():
            out["outline_" + name] = (change(), text, (-1,) * 3 if text is _ROOM else (KEPT,) * 3)
    return out


def convert(value, keep):
    """An argument as ctypes takes it; what must outlive the call goes to ``keep``."""
    if isinstance(value, np.ndarray):
        keep.append(value)
        return _ffi.ptr(value)
    if isinstance(value, Off):
        keep.append(value.arr)
        return C.c_void_p(value.arr.ctypes.data + value.n)
    if isinstance(value, Ptr3):
        keep.extend(value.arrs)
        p = _ffi.ptr3(value.arrs)
        keep.append(p)
        return C.byref(p)
    if isinstance(value, (C.c_int64, C.c_int, _ffi.Outlines)):
        return C.byref(value)
    return value


def invoke(entry, order, arguments):
    """-> (status, message) of ``entry`` called with ``arguments[name] for name in order``."""
    lib = _ffi.load()
    keep = []
    status = getattr(lib, entry)(*[convert(arguments[name], keep) for name in order])
    message = lib.lars_last_error()
    return status, message.decode() if message else ""
