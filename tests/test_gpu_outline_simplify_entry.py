"""lars_h_outline_simplify and lars_d_outline_simplify on rings no tracer writes (outline_simplify_cases.hand_built; include/lars_hip.h
"simplified outlines"): coordinates up to 32767, a near-collinear vertex less than 256 from the threshold on either side, equal maxima,
stretches whose ends coincide, a triangle, a result that flips its sign -- every expectation the model's (outline_simplify_model.py),
every comparison bit for bit -- and damaged rows and counts, which give an error or wrong rings and touch nothing beyond the buffers:
what lies behind a capacity is watched with rows of a sentinel byte.  Every call is within the contract: the scratch has the size the
library asks for and the buffers are the library's own allocations."""
import ctypes as C

import numpy as np
import pytest

import outline_simplify_cases as oc
from lars_image_processing_amd import _ffi
from test_gpu_outline_entry import Room, untouched, upload

pytestmark = pytest.mark.gpu

SIDE = oc.M


def ring_rows(given):
    rows = np.zeros(given["n_rings"], dtype=_ffi.RING_DTYPE)
    for field, key in (("label", "ring_label"), ("key", "ring_key"), ("start", "ring_start"), ("count", "ring_count"), ("area2", "ring_area2")):
        rows[field] = given[key]
    return rows


def host_simplify(rows, verts, tq, room=None, side=SIDE):
    """One lars_h_outline_simplify -> (status, rings_out, verts_out[:written], (rings, written, restored), rounds)"""
    lib = _ffi.load()
    verts = np.ascontiguousarray(verts, dtype=np.int32).reshape(-1, 2)
    room = len(verts) if room is None else room
    rings_out = np.zeros(len(rows), dtype=_ffi.RING_DTYPE)
    for field in rings_out.dtype.names:
        rings_out[field] = -7
    verts_out = np.full((room, 2), -7, dtype=np.int32)
    counts, rounds = (C.c_int64 * 3)(-5, -5, -5), C.c_int64(-5)
    status = lib.lars_h_outline_simplify(_ffi.ptr(rows), len(rows), _ffi.ptr(verts), len(verts), tq, side, side, _ffi.ptr(rings_out), _ffi.ptr(verts_out), room,
                                         C.byref(counts), C.byref(rounds))
    return status, rings_out, verts_out, tuple(counts), rounds.value


def same_as_model(rings_out, verts_out, counts, want):
    assert counts == (want["n_rings"], want["n_vertices"], int(want["restored"].sum())), counts
    for field, key in (("label", "ring_label"), ("key", "ring_key"), ("start", "ring_start"), ("count", "ring_count"), ("area2", "ring_area2")):
        assert np.array_equal(rings_out[field], want[key]), (field, rings_out[field][:8].tolist(), want[key][:8].tolist())
    assert np.array_equal(verts_out[:want["n_vertices"]], want["verts"])
    assert (verts_out[want["n_vertices"]:] == -7).all()


@pytest.mark.parametrize("name", sorted(oc.hand_built()))
def test_hand_built_rings(name):
    given, tq, want = oc.hand_case(name)
    status, rings_out, verts_out, counts, rounds = host_simplify(ring_rows(given), given["verts"], tq)
    assert status == 0, _ffi.load().lars_last_error().decode()
    same_as_model(rings_out, verts_out, counts, want)
    assert rounds == want["rounds"]


def test_the_rounds_of_a_comb_and_of_one_long_ring():
    """Traced rings through the same entry: the comb's depth is several host batches, the serpentine's first stretch spans workgroups."""
    for name, connectivity in (("comb_24", 8), ("serpentine", 4)):
        given, want = oc.labelled(name, connectivity)[2], oc.simplified(name, connectivity, 16)
        status, rings_out, verts_out, counts, rounds = host_simplify(ring_rows(given), given["verts"], 16)
        assert status == 0, _ffi.load().lars_last_error().decode()
        same_as_model(rings_out, verts_out, counts, want)
        assert rounds == want["rounds"] and (name != "comb_24" or rounds > 2 * oc.BATCH)


def test_short_vertex_room_reports_the_count_and_writes_nothing():
    given, tq, want = oc.hand_case("wiggle")
    assert want["n_vertices"] < given["n_vertices"]
    status, rings_out, verts_out, counts, _ = host_simplify(ring_rows(given), given["verts"], tq, room=want["n_vertices"] - 1)
    assert status == -1 and counts[1] == want["n_vertices"] and (verts_out == -7).all() and (rings_out["count"] == -7).all()
    assert "%d vertices; the room is %d" % (want["n_vertices"], want["n_vertices"] - 1) in _ffi.load().lars_last_error().decode()
    status, rings_out, verts_out, counts, _ = host_simplify(ring_rows(given), given["verts"], tq, room=want["n_vertices"])
    assert status == 0
    same_as_model(rings_out, verts_out, counts, want)


def test_refusals_launch_nothing():
    given, tq, _ = oc.hand_case("triangle")
    rows = ring_rows(given)
    for change, text in (({"tq": 0}, "tq must be 1 to 4064"), ({"tq": 4065}, "tq must be 1 to 4064"), ({"side": 32768}, "the raster is 1 to 32767 on each side"),
                         ({"side": 0}, "the raster is 1 to 32767 on each side")):
        status, rings_out, verts_out, counts, _ = host_simplify(rows, given["verts"], change.get("tq", tq), side=change.get("side", SIDE))
        assert status == -1 and text in _ffi.load().lars_last_error().decode(), change
        assert counts == (-1, -1, -1) and (verts_out == -7).all()
    lib = _ffi.load()
    assert lib.lars_outline_simplify_scratch_bytes(-1, 4) == 0 and lib.lars_outline_simplify_scratch_bytes(4, -1) == 0
    assert lib.lars_outline_simplify_scratch_bytes(1 << 31, 4) == 0 and lib.lars_outline_simplify_scratch_bytes(4, 1 << 31) == 0
    assert 0 < lib.lars_outline_simplify_scratch_bytes(0, 0) <= 14 * 256
    assert 29 * 1000 + 58 * 100 <= lib.lars_outline_simplify_scratch_bytes(100, 1000) < 29 * 1000 + 58 * 100 + 14 * 256


# ===========================================================================
# damaged rows and counts
# ===========================================================================
def expect_without(given, tq, damaged):
    """The model on the rings that can be followed: (count, area2) per row, a damaged row being (0, 0), and the vertices written."""
    import outline_simplify_model as sm
    keep = [i for i in range(given["n_rings"]) if i not in damaged]
    part = {k: (v[keep] if isinstance(v, np.ndarray) and k != "verts" else v) for k, v in given.items()}
    part["n_rings"] = len(keep)
    want = sm.simplify(part, tq)
    count, area2 = np.zeros(given["n_rings"], dtype=np.int32), np.zeros(given["n_rings"], dtype=np.int64)
    count[keep], area2[keep] = want["ring_count"], want["ring_area2"]
    return count, area2, want["verts"]


@pytest.mark.parametrize("damage", ["start_below_0", "start_behind_the_end", "count_beyond_the_end", "count_0", "count_below_0", "count_2_to_31"])
def test_a_row_that_leaves_the_vertex_array_is_a_ring_without_vertices(damage):
    given, tq, _ = oc.hand_case("many_small")
    rows = ring_rows(given)
    v = given["n_vertices"]
    hit = {"start_below_0": (7, "start", -1), "start_behind_the_end": (299, "start", v - 3), "count_beyond_the_end": (150, "count", v),
           "count_0": (0, "count", 0), "count_below_0": (42, "count", -4), "count_2_to_31": (42, "count", (1 << 31) - 1)}[damage]
    rows[hit[1]][hit[0]] = hit[2]
    status, rings_out, verts_out, counts, _ = host_simplify(rows, given["verts"], tq)
    assert status == 0, _ffi.load().lars_last_error().decode()
    count, area2, verts = expect_without(given, tq, {hit[0]})
    assert counts[:2] == (given["n_rings"], len(verts))
    assert np.array_equal(rings_out["count"], count) and np.array_equal(rings_out["area2"], area2)
    assert np.array_equal(rings_out["label"], given["ring_label"]) and np.array_equal(rings_out["key"], given["ring_key"])
    live = count > 0
    assert np.array_equal(rings_out["start"][live], (np.cumsum(count) - count)[live])
    assert np.array_equal(verts_out[:len(verts)], verts) and (verts_out[len(verts):] == -7).all()


def device_simplify(rows, verts, counts_in, tq, ring_capacity, vert_capacity, vert_capacity_out):
    """One lars_d_outline_simplify on the library stream, every buffer with a watched tail."""
    lib = _ffi.load()
    d_rows, d_verts, d_counts = upload(rows), upload(np.ascontiguousarray(verts, dtype=np.int32)), upload(np.array(counts_in, dtype=np.int64))
    rings_out, verts_out, counts_out = Room(ring_capacity, _ffi.RING_DTYPE), Room(vert_capacity_out, np.int32, cols=2), Room(3, np.int64)
    need = int(lib.lars_outline_simplify_scratch_bytes(ring_capacity, vert_capacity))
    assert need > 0
    scratch, rounds = _ffi.DeviceBuffer(need), C.c_int64(-5)
    try:
        status = lib.lars_d_outline_simplify(C.c_void_p(d_rows.ptr), ring_capacity, C.c_void_p(d_verts.ptr), vert_capacity, C.c_void_p(d_counts.ptr), tq, SIDE, SIDE,
                                             rings_out.ptr, verts_out.ptr, vert_capacity_out, counts_out.ptr, C.c_void_p(scratch.ptr), C.byref(rounds), None)
        assert status == 0, lib.lars_last_error().decode()
        _ffi.call("lars_synchronize", None)
        got_counts, counts_tail = counts_out.fetch()
        got_rings, ring_tail = rings_out.fetch()
        got_verts, vert_tail = verts_out.fetch()
        assert untouched(counts_tail) and untouched(ring_tail) and untouched(vert_tail)
        return tuple(int(c) for c in got_counts), got_rings, got_verts, rounds.value
    finally:
        for b in (d_rows, d_verts, d_counts, rings_out, verts_out, counts_out, scratch):
            b.free()


def test_the_device_entry_with_exact_and_with_short_room():
    given, tq, want = oc.hand_case("lobes")
    rows = ring_rows(given)
    q, v = given["n_rings"], given["n_vertices"]
    counts, rings_out, verts_out, rounds = device_simplify(rows, given["verts"], (0, q, v), tq, q, v, want["n_vertices"])
    assert counts == (q, want["n_vertices"], 0) and rounds == want["rounds"]
    assert np.array_equal(rings_out["count"], want["ring_count"]) and np.array_equal(rings_out["area2"], want["ring_area2"]) and np.array_equal(verts_out, want["verts"])
    counts, rings_out, verts_out, _ = device_simplify(rows, given["verts"], (0, q, v), tq, q, v, 2)           # the count whatever the room is
    assert counts == (q, want["n_vertices"], 0) and np.array_equal(verts_out, want["verts"][:2])
    assert np.array_equal(rings_out["count"], want["ring_count"]) and np.array_equal(rings_out["start"], want["ring_start"])


def test_counts_above_the_capacities_count_as_nothing():
    given, tq, want = oc.hand_case("square_equal_maxima")
    rows = ring_rows(given)
    q, v = given["n_rings"], given["n_vertices"]
    counts, rings_out, verts_out, _ = device_simplify(rows, given["verts"], (0, q + 1, v), tq, q, v, v)       # more rings than rows: none is read
    assert counts == (0, 0, 0) and untouched(rings_out) and untouched(verts_out)
    counts, rings_out, verts_out, _ = device_simplify(rows, given["verts"], (0, -1, v), tq, q, v, v)
    assert counts == (0, 0, 0) and untouched(rings_out) and untouched(verts_out)
    counts, rings_out, verts_out, _ = device_simplify(rows, given["verts"], (0, q, v + 1), tq, q, v, v)       # more vertices than the array: no row can be followed
    assert counts == (q, 0, 0) and (rings_out["count"] == 0).all() and untouched(verts_out)
    assert np.array_equal(rings_out["label"], given["ring_label"])
    counts, rings_out, verts_out, _ = device_simplify(rows, given["verts"], (0, q, v - 1), tq, q, v, v)       # fewer: the last ring leaves them
    assert counts[:2] == (q, want["ring_count"][0]) and rings_out["count"].tolist() == [want["ring_count"][0], 0]
    assert np.array_equal(verts_out[:counts[1]], want["verts"][:counts[1]])
