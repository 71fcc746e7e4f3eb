"""lars_d_region_outline and lars_d_region_label at their device entries, on what the host routes never hand them (include/lars_hip.h
"region outlines", "zones from regions"): label rasters no labeller writes (outline_label_cases.py), edge room above and below the
count, ring and vertex room that is short on the device, an n_labels below the labels.  Every expectation is the model's
(outlines_model.trace, regions_model.label), every comparison of integers and bit for bit; what lies beyond a capacity is watched with
64 rows of a sentinel byte behind each table and array.  Every call is within the contract: the scratch has the size the library asks
for, the buffers are the library's own allocations, and the refused calls launch nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import outline_label_cases as lc
import outlines_model as om
import regions_cases as gc
import regions_model as gm
from lars_image_processing_amd import _ffi

pytestmark = pytest.mark.gpu

TAIL = 64                               # rows behind every capacity that nothing may touch
SENTINEL = 0xA5
RING_FIELDS = (("label", "ring_label"), ("key", "ring_key"), ("start", "ring_start"), ("count", "ring_count"), ("area2", "ring_area2"))
CASES = sorted(lc.cases())


def untouched(rows):
    return bool((np.ascontiguousarray(rows).view(np.uint8) == SENTINEL).all())


class Room:
    """``capacity`` rows of ``dtype`` (``cols`` of them a row) on the device and TAIL more, all of them sentinel bytes; capacity 0 with
    ``null``: no buffer at all, the pointer is NULL."""

    def __init__(self, capacity, dtype, null=False, cols=None):
        self.capacity, self.dtype, self.cols = capacity, np.dtype(dtype), cols
        self.row_bytes = self.dtype.itemsize * (cols or 1)
        self.buf = None if null else _ffi.DeviceBuffer((capacity + TAIL) * self.row_bytes)
        if self.buf:
            self.buf.upload(np.full(self.buf.nbytes, SENTINEL, dtype=np.uint8))

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr) if self.buf else None

    def fetch(self):
        """-> (rows[:capacity], the tail)"""
        shape = (-1, self.cols) if self.cols else (-1,)
        if not self.buf:
            return np.zeros(0, dtype=self.dtype).reshape(shape), np.zeros(0, dtype=self.dtype).reshape(shape)
        rows = self.buf.download(np.uint8, ((self.capacity + TAIL) * self.row_bytes,)).view(self.dtype).reshape(shape)
        return rows[:self.capacity], rows[self.capacity:]

    def free(self):
        if self.buf:
            self.buf.free()


def upload(arr):
    arr = np.ascontiguousarray(arr)
    buf = _ffi.DeviceBuffer(max(arr.nbytes, 4))
    buf.upload(arr)
    return buf


def device_trace(labels, connectivity, n_labels, edge_capacity, ring_capacity, vert_capacity, shape=None):
    """One lars_d_region_outline on the library stream.  ``labels``: an int32 raster, or a DeviceBuffer that holds one of ``shape``.
    ring_capacity / vert_capacity 0: rings / verts NULL.  -> {"counts": (edges, rings, vertices), "rings", "verts": the rows below the
    capacities, "ring_tail", "vert_tail": the TAIL rows behind them}"""
    lib = _ffi.load()
    own = not isinstance(labels, _ffi.DeviceBuffer)
    h, w = labels.shape if own else shape
    d_labels = upload(labels.astype(np.int32, copy=False)) if own else labels
    need = int(lib.lars_region_outline_scratch_bytes(h, w, edge_capacity))
    assert need > 0 or edge_capacity == 0
    scratch = _ffi.DeviceBuffer(need or 256)
    rings, verts = Room(ring_capacity, _ffi.RING_DTYPE, null=ring_capacity == 0), Room(vert_capacity, np.int32, null=vert_capacity == 0, cols=2)
    counts = Room(3, np.int64)
    try:
        _ffi.call("lars_d_region_outline", C.c_void_p(d_labels.ptr), h, w, connectivity, n_labels, edge_capacity, rings.ptr, ring_capacity, verts.ptr,
                  vert_capacity, counts.ptr, C.c_void_p(scratch.ptr), None)
        _ffi.call("lars_synchronize", None)
        got_counts, counts_tail = counts.fetch()
        assert untouched(counts_tail)
        out = {"counts": tuple(int(v) for v in got_counts)}
        out["rings"], out["ring_tail"] = rings.fetch()
        out["verts"], out["vert_tail"] = verts.fetch()
        return out
    finally:
        for b in (rings, verts, counts, scratch) + ((d_labels,) if own else ()):
            b.free()


def device_edge_count(labels):
    d_labels, d_count = upload(labels.astype(np.int32, copy=False)), Room(1, np.int64)
    try:
        _ffi.call("lars_d_region_outline_count", C.c_void_p(d_labels.ptr), labels.shape[0], labels.shape[1], d_count.ptr, None)
        _ffi.call("lars_synchronize", None)
        count, tail = d_count.fetch()
        assert untouched(tail)
        return int(count[0])
    finally:
        d_labels.free()
        d_count.free()


def same_rows(rings, want, rows=None):
    """The first ``rows`` rows (all of them: None) of the ring table are the expectation's, field by field."""
    rows = len(rings) if rows is None else rows
    assert rings.dtype == _ffi.RING_DTYPE and len(rings) >= rows
    for field, key in RING_FIELDS:
        bad = np.flatnonzero(rings[field][:rows] != want[key][:rows])
        assert bad.size == 0, (field, len(bad), bad[:5].tolist(), rings[field][bad[:5]].tolist(), want[key][bad[:5]].tolist())


def same_verts(verts, want, rows=None):
    rows = len(verts) if rows is None else rows
    bad = np.flatnonzero((verts[:rows] != want["verts"][:rows]).any(axis=1))
    assert bad.size == 0, (len(bad), bad[:5].tolist(), verts[bad[:5]].tolist(), want["verts"][bad[:5]].tolist())


def counts_of(want):
    return want["n_edges"], want["n_rings"], want["n_vertices"]


def same_trace(got, want):
    """Exact room: the counts, the whole table and every vertex are the expectation's, and both tails are as they were."""
    assert got["counts"] == counts_of(want), (got["counts"], counts_of(want))
    assert len(got["rings"]) == want["n_rings"] and len(got["verts"]) == want["n_vertices"]
    same_rows(got["rings"], want)
    same_verts(got["verts"], want)
    assert untouched(got["ring_tail"]) and untouched(got["vert_tail"])


@functools.lru_cache(maxsize=None)
def exact(name, connectivity):
    """The named case traced with exactly the room it needs; shared by the tests that compare other rooms with it."""
    c, want = lc.find(name), lc.expected(name, connectivity)
    return device_trace(c["labels"], connectivity, c["n_labels"], *counts_of(want))


# ===========================================================================
# every case, both connectivities, ample room
# ===========================================================================
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", CASES)
def test_every_case_with_ample_room(name, connectivity):
    c, want = lc.cases()[name], lc.expected(name, connectivity)
    same_trace(exact(name, connectivity), want)
    assert device_edge_count(c["labels"]) == want["n_edges"]


# ===========================================================================
# edge room above the count
# ===========================================================================
def rooms_above(edges, pixels):
    above = 1 << edges.bit_length()                                   # the next power of two above E: one more round of doubling
    rooms = (edges + 1, above, above + 1, 4 * pixels)
    assert all(edges < r <= 4 * pixels for r in rooms)
    return rooms


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["scattered", "stripes_1_2", "strip_4096_0_descending"])
def test_edge_room_above_the_count_changes_nothing(name, connectivity):
    c, want = lc.cases()[name], lc.expected(name, connectivity)
    base = exact(name, connectivity)
    same_trace(base, want)
    for room in rooms_above(want["n_edges"], c["labels"].size):
        got = device_trace(c["labels"], connectivity, c["n_labels"], room, want["n_rings"], want["n_vertices"])
        same_trace(got, want)
        assert got["rings"].tobytes() == base["rings"].tobytes() and got["verts"].tobytes() == base["verts"].tobytes(), room
    if name == "scattered":                                           # room for h * w + 1 rings: five sort chunks, a histogram of 1280 entries
        assert 256 * -(-(c["labels"].size + 1) // lc.CHUNK) > 1024 and want["n_rings"] > 2 * lc.CHUNK


# ===========================================================================
# edge room below the count
# ===========================================================================
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["scattered", "stripes_1_2", "strip_2049_0_repeated", "blocks_23x89"])
def test_edge_room_below_the_count_traces_nothing(name, connectivity):
    c, want = lc.cases()[name], lc.expected(name, connectivity)
    edges = want["n_edges"]
    for room in (edges - 1, edges // 2, 0):
        got = device_trace(c["labels"], connectivity, c["n_labels"], room, want["n_rings"], want["n_vertices"])
        assert got["counts"] == (edges, 0, 0), (room, got["counts"])
        assert untouched(got["rings"]) and untouched(got["verts"]) and untouched(got["ring_tail"]) and untouched(got["vert_tail"]), room


# ===========================================================================
# short ring room, short vertex room
# ===========================================================================
def short_ring_rooms(rings):
    boundary = (rings - 1) // lc.CHUNK * lc.CHUNK - 1                 # one short of the last chunk boundary below the count
    return sorted({0, 1, rings - 1, boundary} - {-1})


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["scattered", "stripes_1_16777217", "strip_2049_0_descending", "strip_4097_0_low_byte"])
def test_short_ring_room_cuts_the_table_and_nothing_else(name, connectivity):
    c, want = lc.cases()[name], lc.expected(name, connectivity)
    rooms = short_ring_rooms(want["n_rings"])
    assert name.startswith("stripes") or {lc.CHUNK - 1, 2 * lc.CHUNK - 1} & set(rooms)
    for room in rooms:
        got = device_trace(c["labels"], connectivity, c["n_labels"], want["n_edges"], room, want["n_vertices"])
        assert got["counts"] == counts_of(want), (room, got["counts"])
        assert len(got["rings"]) == room
        same_rows(got["rings"], want, room)                           # area2, start and count of the rows that are there
        assert untouched(got["ring_tail"]) and untouched(got["vert_tail"]), room
        same_verts(got["verts"], want)                                # all V of them


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["scattered", "stripes_1_2", "strip_2049_0_descending", "blocks_3x683"])
def test_short_vertex_room_cuts_the_vertices_and_nothing_else(name, connectivity):
    c, want = lc.cases()[name], lc.expected(name, connectivity)
    for room in (0, 4, want["n_vertices"] - 1):
        got = device_trace(c["labels"], connectivity, c["n_labels"], want["n_edges"], want["n_rings"], room)
        assert got["counts"] == counts_of(want), (room, got["counts"])
        same_rows(got["rings"], want)                                 # start and count do not depend on the room
        assert len(got["verts"]) == room
        same_verts(got["verts"], want, room)
        assert untouched(got["ring_tail"]) and untouched(got["vert_tail"]), room


def test_short_ring_and_vertex_room_together():
    c, want = lc.cases()["scattered"], lc.expected("scattered", 8)
    ring_room, vert_room = lc.CHUNK + 1, 2 * lc.CHUNK - 1
    got = device_trace(c["labels"], 8, c["n_labels"], want["n_edges"] + 3, ring_room, vert_room)
    assert got["counts"] == counts_of(want)
    same_rows(got["rings"], want, ring_room)
    same_verts(got["verts"], want, vert_room)
    assert untouched(got["ring_tail"]) and untouched(got["vert_tail"])


# ===========================================================================
# understated n_labels
# ===========================================================================
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(lc.understated_cases()))
def test_understated_n_labels_sort_by_the_low_bytes(name, connectivity):
    c, want = lc.understated_cases()[name], lc.expected(name, connectivity)
    assert c["passes"] < 4 and not np.array_equal(want["ring_label"], lc.model_trace("scattered", connectivity)["ring_label"])
    same_trace(exact(name, connectivity), want)


# ===========================================================================
# background only; the same call twice
# ===========================================================================
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("edge_capacity", [0, 16])
def test_background_only_writes_nothing(edge_capacity, connectivity):
    c = lc.background()
    got = device_trace(c["labels"], connectivity, c["n_labels"], edge_capacity, 8, 8)
    assert got["counts"] == (0, 0, 0)
    assert untouched(got["rings"]) and untouched(got["verts"]) and untouched(got["ring_tail"]) and untouched(got["vert_tail"])
    nothing = device_trace(c["labels"], connectivity, c["n_labels"], edge_capacity, 0, 0)
    assert nothing["counts"] == (0, 0, 0)
    assert device_edge_count(c["labels"]) == 0


@pytest.mark.parametrize("connectivity", [4, 8])
def test_twice_the_same_call_gives_the_same_bytes(connectivity):
    c, want = lc.cases()["scattered"], lc.expected("scattered", connectivity)
    one = exact("scattered", connectivity)
    two = device_trace(c["labels"], connectivity, c["n_labels"], *counts_of(want))
    assert two["counts"] == one["counts"] == counts_of(want)
    assert two["rings"].tobytes() == one["rings"].tobytes() and two["verts"].tobytes() == one["verts"].tobytes()


# ===========================================================================
# refusals that launch nothing
# ===========================================================================
BAD_RASTER = r"lars_d_region_outline: the raster is 1 or more on each side and has fewer than 2^29 pixels (an edge id fits int32), got 32768 x 16384"
BAD_ARGUMENTS = ("lars_d_region_outline: bad arguments (connectivity 4 or 8, n_labels 0 to 2^31 - 1, edge_capacity 0 to 4 * h * w, "
                 "a ring table and a vertex array of capacity >= 0)")
H, W = 6, 9
GOOD = {"labels": 0, "h": H, "w": W, "connectivity": 8, "n_labels": 3, "edge_capacity": 4 * H * W, "rings": 1024, "ring_capacity": 4,
        "verts": 2048, "vert_capacity": 4, "counts": 3072, "scratch": 4096}
REFUSALS = {
    "connectivity_5": ({"connectivity": 5}, BAD_ARGUMENTS),
    "n_labels_below_0": ({"n_labels": -1}, BAD_ARGUMENTS),
    "n_labels_2_to_31": ({"n_labels": 1 << 31}, BAD_ARGUMENTS),
    "edge_capacity_below_0": ({"edge_capacity": -1}, BAD_ARGUMENTS),
    "edge_capacity_above_4hw": ({"edge_capacity": 4 * H * W + 1}, BAD_ARGUMENTS),
    "rings_null_with_room": ({"rings": None}, BAD_ARGUMENTS),
    "verts_null_with_room": ({"verts": None}, BAD_ARGUMENTS),
    "counts_null": ({"counts": None}, BAD_ARGUMENTS),
    "scratch_null": ({"scratch": None}, BAD_ARGUMENTS),
    "raster_of_2_to_29_pixels": ({"h": 1 << 15, "w": 1 << 14, "edge_capacity": 8}, BAD_RASTER),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_launch_nothing(name):
    """Bad arguments are answered with -1 and their text before any launch: the pointers are small and valid (offsets into one
    allocation that is as large as the good call needs), or NULL where NULL is the case, and nothing behind them changes."""
    lib = _ffi.load()
    change, text = REFUSALS[name]
    arena = Room((4096 + int(lib.lars_region_outline_scratch_bytes(H, W, 4 * H * W))) // 8, np.int64)
    try:
        a = dict(GOOD, **change)
        at = {k: (None if a[k] is None else C.c_void_p(arena.buf.ptr + a[k])) for k in ("labels", "rings", "verts", "counts", "scratch")}
        status = lib.lars_d_region_outline(at["labels"], a["h"], a["w"], a["connectivity"], a["n_labels"], a["edge_capacity"], at["rings"], a["ring_capacity"],
                                           at["verts"], a["vert_capacity"], at["counts"], at["scratch"], None)
        assert status == -1 and lib.lars_last_error().decode() == text
        _ffi.call("lars_synchronize", None)
        rows, tail = arena.fetch()
        assert untouched(rows) and untouched(tail)
        if name == "raster_of_2_to_29_pixels":
            d_count = C.c_void_p(arena.buf.ptr + GOOD["counts"])
            assert lib.lars_d_region_outline_count(at["labels"], a["h"], a["w"], d_count, None) == -1
            assert "fewer than 2^29 pixels" in lib.lars_last_error().decode()
    finally:
        arena.free()


def test_scratch_bytes_is_0_for_the_refused_shapes_and_capacities_only():
    lib = _ffi.load()
    for h, w, room in ((1 << 15, 1 << 14, 8), (H, W, -1), (H, W, 4 * H * W + 1), (0, W, 8), (H, -1, 8)):
        assert lib.lars_region_outline_scratch_bytes(h, w, room) == 0, (h, w, room)
    # edge_capacity 0 is a legal room: 4 bytes a pixel and a little, each array on a multiple of 256
    assert 4 * H * W <= lib.lars_region_outline_scratch_bytes(H, W, 0) < 4 * H * W + 14 * 256
    assert 4 * 70 * 130 <= lib.lars_region_outline_scratch_bytes(70, 130, 0) < 4 * 70 * 130 + 14 * 256


# ===========================================================================
# the labeller's device entry: short room, and its labels straight into the tracer
# ===========================================================================
def same_region_rows(rows, model, count):
    assert rows.dtype == _ffi.REGION_DTYPE and len(rows) >= count
    for field in gm.REGION_FIELDS:
        assert np.array_equal(rows[field][:count], model[field][:count]), field


def label_then_trace(mask, connectivity, capacity, model, want):
    """lars_d_region_label with ``capacity`` rows of table (0: NULL), then lars_d_region_outline of the labels where they stand, with
    n_labels = R: no copy, no wait between the two."""
    lib = _ffi.load()
    h, w = mask.shape
    n = model["n_regions"]
    d_mask = upload(mask.astype(np.uint8))
    d_labels = Room(h * w, np.int32)
    table, count = Room(capacity, _ffi.REGION_DTYPE, null=capacity == 0), Room(1, np.int64)
    need = int(lib.lars_region_label_scratch_bytes(h, w))
    assert need > 0
    scratch = _ffi.DeviceBuffer(need)
    try:
        _ffi.call("lars_d_region_label", C.c_void_p(d_mask.ptr), h, w, connectivity, 1, d_labels.ptr, table.ptr, capacity, count.ptr, C.c_void_p(scratch.ptr), None)
        traced = device_trace(d_labels.buf, connectivity, n, *counts_of(want), shape=(h, w))      # synchronises
        labels, label_tail = d_labels.fetch()
        rows, row_tail = table.fetch()
        got_count, count_tail = count.fetch()
        assert int(got_count[0]) == n and untouched(count_tail) and untouched(label_tail)          # R whatever the capacity is
        assert np.array_equal(labels.reshape(h, w), model["labels"])
        assert len(rows) == capacity
        same_region_rows(rows, model, min(n, capacity))
        assert untouched(rows[min(n, capacity):]) and untouched(row_tail)
        return traced
    finally:
        for b in (d_mask, d_labels, table, count, scratch):
            b.free()


LABELLER_MASKS = {"lattice_300": (lambda: gc.lattice(300), 8), "checkerboard": (lambda: gc.named()["checkerboard"], 4)}


@pytest.mark.parametrize("room", ["none", "one", "one_short", "exact"])
@pytest.mark.parametrize("name", sorted(LABELLER_MASKS))
def test_labeller_short_room_and_its_labels_straight_into_the_tracer(name, room):
    make, connectivity = LABELLER_MASKS[name]
    mask = make()
    model = gm.label(mask, connectivity)
    n = model["n_regions"]
    assert n > 256 and (name != "lattice_300" or n == 300)
    want = om.trace(model["labels"], connectivity)
    capacity = {"none": 0, "one": 1, "one_short": n - 1, "exact": n}[room]
    same_trace(label_then_trace(mask, connectivity, capacity, model, want), want)
