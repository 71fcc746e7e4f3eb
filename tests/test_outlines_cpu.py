"""Region outlines without a device: the model of the definition (outlines_model.py) against the invariants the definition promises,
against hand-written rings, and against its own walk through the stages of csrc/outlines.hip; to_world, the GeoJSON writer, and the
refusals that are decided on the host."""
import json

import numpy as np
import pytest

import outlines_model as om
import regions_cases as gc
import regions_model as gm
import zone_raster_model as zm
import lars_image_processing_amd as lars
from lars_image_processing_amd import driver


def invariants(mask, connectivity, min_pixels=1):
    """One ring of positive area per region, keyed by the region's first pixel and first of its rings; the areas of a region's rings add
    up to its pixels; vertices alternate between rows and columns; the rasterised rings are the labels; the staged walk agrees."""
    model = gm.label(mask, connectivity, min_pixels)
    labels, n = model["labels"], model["n_regions"]
    traced = om.trace(labels, connectivity)
    assert om.same(traced, om.trace_staged(labels, connectivity))
    assert np.array_equal(traced["ring_label"], np.sort(traced["ring_label"]))
    first_pixel = {}
    for i, v in enumerate(labels.ravel().tolist()):
        first_pixel.setdefault(v, i)
    for k in range(1, n + 1):
        mine = np.flatnonzero(traced["ring_label"] == k)
        area2 = traced["ring_area2"][mine]
        assert (area2 > 0).sum() == 1 and area2[0] > 0 and (area2[1:] < 0).all()
        assert traced["ring_key"][mine[0]] == 4 * first_pixel[k]
        assert np.array_equal(traced["ring_key"][mine], np.sort(traced["ring_key"][mine]))
        assert area2.sum() == 2 * model["area"][k - 1]
    for start, count in zip(traced["ring_start"], traced["ring_count"]):
        ring = traced["verts"][start:start + count]
        assert count >= 4 and count % 2 == 0
        step = np.roll(ring, -1, axis=0) - ring
        assert ((step != 0).sum(axis=1) == 1).all()                   # one coordinate changes ...
        assert ((step[:, 0] != 0) != np.roll(step[:, 0] != 0, 1)).all()   # ... rows and columns in turn: no vertex inside a straight run
    assert traced["n_vertices"] == traced["ring_count"].sum() and traced["n_edges"] == len(om.edges_of(labels))
    if 0 < n <= 65535:
        assert np.array_equal(zm.labels(om.polygon_list(traced, n), labels.shape), labels)
    return traced


@pytest.mark.parametrize("connectivity", [4, 8])
def test_all_masks_of_three_by_three(connectivity):
    for k in range(512):
        invariants(((k >> np.arange(9).reshape(3, 3)) & 1) != 0, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(gc.named()))
def test_named_masks(name, connectivity):
    invariants(gc.named()[name], connectivity)


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz(chunk):
    for seed in range(chunk * 25, chunk * 25 + 25):
        mask, connectivity, min_pixels = gc.fuzz_case(seed, most=60)
        invariants(mask, connectivity, min_pixels)


HAND = {
    "one pixel": ([[1]], 8, [[(0, 0), (0, 1), (1, 1), (1, 0)]], [2]),
    "a block": ([[1, 1], [1, 1]], 4, [[(0, 0), (0, 2), (2, 2), (2, 0)]], [8]),
    "a ring with its hole": ([[1, 1, 1], [1, 0, 1], [1, 1, 1]], 4, [[(0, 0), (0, 3), (3, 3), (3, 0)], [(1, 2), (1, 1), (2, 1), (2, 2)]], [18, -2]),
    "the diagonal pair under 4": ([[1, 0], [0, 1]], 4, [[(0, 0), (0, 1), (1, 1), (1, 0)], [(1, 1), (1, 2), (2, 2), (2, 1)]], [2, 2]),
    "the diagonal pair under 8": ([[1, 0], [0, 1]], 8, [[(0, 0), (0, 1), (1, 1), (1, 2), (2, 2), (2, 1), (1, 1), (1, 0)]], [4]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_rings(name):
    mask, connectivity, rings, area2 = HAND[name]
    traced = invariants(np.array(mask, dtype=bool), connectivity)
    got = [[tuple(v) for v in traced["verts"][s:s + c].tolist()] for s, c in zip(traced["ring_start"], traced["ring_count"])]
    assert got == rings and traced["ring_area2"].tolist() == area2
    assert traced["ring_label"].tolist() == ([1, 2] if name == "the diagonal pair under 4" else [1] * len(rings))


def test_to_world_is_the_inverse_of_to_pixel():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-50, 4000, size=(7, 11, 2))
    for transform in ((0, 1, 0, 0, 0, 1), (431000.5, 0.02, 0, 5412000.25, 0, -0.02), (10.0, 0.3, 0.1, -7.0, -0.2, 0.4)):
        world = lars.to_world(pts, transform)
        assert world.dtype == np.float64 and world.shape == pts.shape
        x0, dx, rx, y0, ry, dy = transform
        assert np.array_equal(world[..., 0], x0 + pts[..., 0] * dx + pts[..., 1] * rx)
        assert np.array_equal(world[..., 1], y0 + pts[..., 0] * ry + pts[..., 1] * dy)
        # both directions round a few times in float64; the coordinates here are below 2^23 in size
        assert np.abs(lars.to_pixel(world, transform) - pts).max() <= 2.0 ** -20
    corners = np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 2.0]])          # integers and a power-of-two pixel size: exact both ways
    assert np.array_equal(lars.to_pixel(lars.to_world(corners, (100, 0.5, 0, 200, 0, -0.5)), (100, 0.5, 0, 200, 0, -0.5)), corners)
    for bad, message in (((1, 2, 3), "to_world: transform must be six finite numbers"), ((0, 1, 0, 0, 0, 0), "to_world: the transform .* is singular"),
                         ("abc", "to_world: transform must be six")):
        with pytest.raises(ValueError, match=message):
            lars.to_world(pts, bad)
    with pytest.raises(ValueError, match=r"to_world: points must be \[..., 2\]"):
        lars.to_world(np.zeros((3, 3)), (0, 1, 0, 0, 0, 1))


def packed(traced, n):
    return lars.Polygons._packed(*om.polygons(traced, n))


def test_geojson_round_trip(tmp_path):
    mask, connectivity, min_pixels = gc.fuzz_case(9, most=60)
    model = gm.label(mask, connectivity, min_pixels)
    n = model["n_regions"]
    p = packed(om.trace(model["labels"], connectivity), n)
    props = [{"Zone": k + 1, "Area": int(model["area"][k])} for k in range(n)]
    doc = lars.polygons_to_geojson(p, properties=props)
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == n and len(p.ring_starts) - 1 > n          # some region has a hole
    assert [f["properties"] for f in doc["features"]] == props and all(f["geometry"]["type"] == "Polygon" for f in doc["features"])
    path = tmp_path / "regions.geojson"
    path.write_text(json.dumps(doc))
    for source in (doc, path):
        back = lars.polygons_from_geojson(source)
        # a ring is written closed, its first vertex repeated, and read as it stands: without that vertex it is the ring it was
        again = lars.Polygons([[ring[:-1] for ring in rings] for rings in back])
        assert all(np.array_equal(ring[-1], ring[0]) for rings in back for ring in rings)
        assert np.array_equal(again.verts, p.verts) and np.array_equal(again.ring_starts, p.ring_starts) and np.array_equal(again.poly_starts, p.poly_starts)
        assert np.array_equal(zm.labels(back, mask.shape), model["labels"])          # the repeated vertex changes no label
    transform = (431000.5, 0.25, 0, 5412000.25, 0, -0.25)
    world = lars.polygons_to_geojson(p, transform=transform)
    ring = np.array(world["features"][0]["geometry"]["coordinates"][0])
    assert np.array_equal(ring[:-1], lars.to_world(p.rings(0)[0], transform))
    x, y = ring[:-1, 0], ring[:-1, 1]
    # a north-up transform (dy < 0) flips the sign of the shoelace sum, not what the eye sees: the outer ring is clockwise on the map as
    # on the screen, negative with Y upwards (quarters of a unit: exact in float64)
    assert (x * np.roll(y, -1) - np.roll(x, -1) * y).sum() < 0
    again = lars.Polygons(lars.polygons_from_geojson(world), transform=transform)
    assert np.array_equal(zm.labels([again.rings(k) for k in range(n)], mask.shape), model["labels"])
    listed = lars.polygons_to_geojson([[(0, 0), (4, 0), (4, 3)], [[(1, 1), (2, 1), (2, 2)], [(5, 5), (6, 5), (6, 6)]]])
    assert [len(f["geometry"]["coordinates"]) for f in listed["features"]] == [1, 2] and listed["features"][0]["properties"] == {}
    assert listed["features"][0]["geometry"]["coordinates"][0] == [[0.0, 0.0], [4.0, 0.0], [4.0, 3.0], [0.0, 0.0]]
    for bad in ([], [{}] * (n + 1), [1] * n, "x" * n):
        with pytest.raises(ValueError, match=f"polygons_to_geojson: properties must be a list of {n} dicts"):
            lars.polygons_to_geojson(p, properties=bad)


def test_refusals_that_need_no_device(tmp_path):
    huge = np.broadcast_to(np.zeros((1, 1), dtype=bool), (1 << 15, 1 << 14))       # 2^29 pixels that take one byte
    with pytest.raises(ValueError, match=r"region_outlines: the raster has 536870912 pixels; outlines are traced on fewer than 2\*\*29"):
        lars.region_outlines(huge)
    with pytest.raises(ValueError, match="region_outlines: connectivity must be 4"):
        lars.region_outlines(np.ones((3, 3), dtype=bool), connectivity=6)
    with pytest.raises(TypeError, match="region_outlines: mask must be a bool or integer array"):
        lars.region_outlines(np.ones((3, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="region_outlines: min_pixels must be 1 to"):
        lars.region_outlines(np.ones((3, 3), dtype=bool), min_pixels=0)
    for bad, error in ((3, ValueError), (0, ValueError), (-1, ValueError), (1 << 31, ValueError), (4.0, TypeError), (True, TypeError), ("many", TypeError)):
        with pytest.raises(error, match="Regions: max_vertices must be"):
            lars.Regions(above=0.2, want_outlines=True, max_vertices=bad)
    r = lars.Regions(above=0.2)
    assert (r.want_outlines, r.max_vertices) == (False, 1 << 22) and r._outline_room() is None
    asked = lars.Regions(above=0.2, want_outlines=True, max_vertices=4)
    assert asked.want_outlines and asked._outline_room().c.vert_capacity == 4 and asked._outline_room().c.ring_capacity == 1
    with pytest.raises(ValueError, match=r"zonal_statistics: the raster has 536870912 pixels; outlines are traced on fewer than 2\*\*29"):
        asked._check((1 << 15, 1 << 14), None, "zonal_statistics")
    r._check((1 << 15, 1 << 14), None, "zonal_statistics")                          # without outlines the labelling's own limit holds
    with pytest.raises(SystemExit):
        driver.main([str(tmp_path), str(tmp_path / "out"), "--ndvi", "--regions-geojson"])
    with pytest.raises(ValueError, match="regions_geojson writes the outlines of the regions: it goes with regions"):
        driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], regions_geojson=True)
    with pytest.raises(ValueError, match="regions_geojson writes the outlines of the regions: it goes with regions"):
        driver.batch_process(tmp_path, tmp_path / "out", process_ndvi=True, regions_geojson=True)


def test_the_names_are_exported_and_declared():
    from lars_image_processing_amd import _ffi
    for name in ("region_outlines", "to_world", "polygons_to_geojson"):
        assert callable(getattr(lars, name))
    for name in ("lars_region_outline_scratch_bytes", "lars_d_region_outline_count", "lars_d_region_outline", "lars_h_region_outlines",
                 "lars_h_zonal_stats_regions_outlines_f32", "lars_h_process_image_regions_outlines"):
        assert name in _ffi.SIGNATURES
    lib = _ffi.load()
    # 4 bytes a pixel, 35 and a little a byte an edge (DESIGN.md "Region outlines"); nothing for a raster of 2^29 pixels or more
    small, large = lib.lars_region_outline_scratch_bytes(1000, 1000, 100000), lib.lars_region_outline_scratch_bytes(1000, 1000, 1100000)
    assert 4 * 10 ** 6 < small < 4.01 * 10 ** 6 + 36 * 10 ** 5 and 35.0 <= (large - small) / 10 ** 6 <= 35.3
    assert lib.lars_region_outline_scratch_bytes(1 << 15, 1 << 14, 8) == 0 and lib.lars_region_outline_scratch_bytes(0, 5, 8) == 0
    assert lib.lars_region_outline_scratch_bytes((1 << 15) - 1, 1 << 14, 8) > 0
    assert _ffi.RING_DTYPE.itemsize == 24 and _ffi.C.sizeof(_ffi.Outlines) == 56
