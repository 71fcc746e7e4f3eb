"""Zones from polygons without a GPU: the NumPy model of the definition against the model in exact rational arithmetic, the tiling
property, every argument refusal of rasterize_zones (all before any library call), polygons_from_geojson, to_pixel, and the calls
that bring a label raster, which must ask the library for what they asked before."""
import json

import numpy as np
import pytest

import masked_cases as mc
import zonal_cases as zc
import zone_raster_cases as rc
import zone_raster_model as zrm
import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, driver, zones as zones_mod


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
DYADIC = ["vertices_on_centres", "horizontal_edges_on_row_centres", "edges_through_centres", "whole_raster_exactly", "zero_area"]


@pytest.mark.parametrize("name", DYADIC)
def test_model_is_the_exact_rule_on_dyadic_vertices(name):
    polygons, shape = rc.CASES[name]
    shape = (min(shape[0], 33), min(shape[1], 40))
    assert np.array_equal(zrm.labels(polygons, shape), zrm.labels_exact(polygons, shape))


@pytest.mark.parametrize("seed", [0, 2, 4, 6])
def test_model_is_the_exact_rule_on_snapped_random_polygons(seed):
    rng = np.random.default_rng(seed)
    polygons = rc.random_polygons(rng, (24, 28), snap=True)[:8]
    assert np.array_equal(zrm.labels(polygons, (24, 28)), zrm.labels_exact(polygons, (24, 28)))


@pytest.mark.parametrize("name", ["triangle", "comb_200", "far_vertices", "small_and_negative_crossings", "crossing"])
def test_both_evaluation_orders_of_the_model_agree(name):
    polygons, shape = rc.CASES[name]
    assert np.array_equal(zrm.labels(polygons, shape, dense=True), zrm.labels(polygons, shape, dense=False))


def test_ties_fall_as_the_definition_says():
    # a crossing exactly on a pixel centre is left of it (xc <= cx): the pixel is inside what starts there, outside what ends there
    got = zrm.labels([rc.rect(2.5, 2.5, 5.5, 4.5)], (6, 8))
    want = np.zeros((6, 8), dtype=np.uint8)
    want[2:4, 2:5] = 1                                   # rows 2.5 <= cy < 4.5, columns 2.5 <= cx < 5.5
    assert np.array_equal(got, want)
    # even-odd: the overlap of a bow-tie's two halves does not exist, a hole is a hole whichever way it runs
    assert zrm.labels(*rc.CASES["hole"]).tolist() == zrm.labels(*rc.CASES["hole_same_direction"]).tolist()
    assert zrm.labels(*rc.CASES["hole"])[14, 17] == 0 and zrm.labels(*rc.CASES["hole"])[5, 5] == 1


def test_a_grid_of_quads_covers_every_pixel_once():
    shape = (61, 83)
    quads = rc.jittered_grid(6, 7, shape)
    cover = sum(zrm.inside_mask(q, shape).astype(np.int32) for q in quads)
    assert cover.min() == 1 and cover.max() == 1
    lab = zrm.labels(quads, shape)
    assert lab.min() >= 1 and len(np.unique(lab)) > 30


def test_the_later_polygon_wins():
    polygons, shape = rc.CASES["nested"]
    a, b = zrm.labels(polygons, shape), zrm.labels(polygons[::-1], shape)
    assert a[14, 16] == 3 and b[14, 16] == 3 and a[4, 4] == 1 and b[4, 4] == 3 and (a > 0).tolist() == (b > 0).tolist()


# ---------------------------------------------------------------------------
# argument checks: every one of them before any library call
# ---------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def refuse(name, *args):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")
    monkeypatch.setattr(_ffi, "call", refuse)


TRI = [(1.0, 1.0), (8.0, 2.0), (3.0, 7.0)]
MANY = np.broadcast_to(np.zeros((1, 2)), ((1 << 24) + 1, 2))


@pytest.mark.parametrize("polygons, error, words", [
    ([], ValueError, "empty"),
    ([TRI, TRI[:2]], ValueError, "polygon 1 ring 0 has 2 vertices"),
    ([TRI, [TRI, TRI[:1]]], ValueError, "polygon 1 ring 1 has 1 vertices"),
    ([[(1.0, 1.0, 0.0), (8.0, 2.0, 0.0), (3.0, 7.0, 0.0)]], ValueError, r"polygon 0 ring 0 must have shape \[n, 2\]"),
    ([TRI, [1.0, 2.0, 3.0]], ValueError, "polygon 1 ring 0 must have shape"),
    ([TRI, []], ValueError, "polygon 1 has no ring"),
    ([TRI, [(1.0, 1.0), (np.nan, 2.0), (3.0, 7.0)]], ValueError, "polygon 1 ring 0 has a coordinate that is not finite"),
    ([[TRI, [(1.0, 1.0), (np.inf, 2.0), (3.0, 7.0)]]], ValueError, "polygon 0 ring 1 has a coordinate that is not finite"),
    ([[(1.0, 1.0), (1.5e9, 2.0), (3.0, 7.0)]], ValueError, "polygon 0 ring 0 has a pixel coordinate beyond 1e9"),
    ([[(1.0, 1.0), (8.0, -1.0000001e9), (3.0, 7.0)]], ValueError, "beyond 1e9"),
    ([TRI, [("a", "b"), ("c", "d"), ("e", "f")]], TypeError, "polygon 1"),
    ([TRI, 7], TypeError, "polygon 1"),
    ("plots.geojson", TypeError, "polygons_from_geojson"),
    (None, TypeError, "sequence"),
    (rc.one_pixel_squares(65536), ValueError, "65536 polygons; at most 65535"),
    ([MANY], ValueError, r"16777217 vertices in all; at most 2\*\*24"),
])
def test_rasterize_zones_refuses_before_any_launch(no_launch, polygons, error, words):
    with pytest.raises(error, match=words) as e:
        lars.rasterize_zones(polygons, (12, 12))
    assert "rasterize_zones" in str(e.value)


@pytest.mark.parametrize("shape", [(12,), (12, 12, 3), (0, 12), (12, -1), (12.0, 12), "ab", None, (1 << 25, 4)])
def test_rasterize_zones_refuses_a_bad_shape(no_launch, shape):
    with pytest.raises(ValueError, match="shape must be"):
        lars.rasterize_zones([TRI], shape)


def test_the_zone_calls_refuse_polygons_with_n_zones_or_bad_rings(no_launch):
    plane, img = zc.plane(6, 9), mc.image(6, 9, 3)
    for call, who in ((lambda z, **kw: lars.zonal_statistics(plane, z, "NDVI", **kw), "zonal_statistics"),
                      (lambda z, **kw: lars.process_image_zones(img, z, **kw), "process_image_zones")):
        with pytest.raises(ValueError, match=rf"{who}: n_zones cannot be given with polygons: Z = len\(polygons\) = 2"):
            call([TRI, TRI], n_zones=2)
        with pytest.raises(ValueError, match=rf"{who}: polygon 1 ring 0 has 2 vertices"):
            call([TRI, TRI[:2]])
        with pytest.raises(ValueError, match="n_zones cannot be given"):
            call(lars.Polygons([TRI]), n_zones=1)
        with pytest.raises(ValueError, match="empty"):
            call([])


# ---------------------------------------------------------------------------
# transforms and GeoJSON
# ---------------------------------------------------------------------------
GT = (500000.0, 0.25, 0.03, 4100000.0, -0.02, -0.25)


def test_to_pixel_round_trip_and_the_singular_case():
    px = np.array([[0.0, 0.0], [10.5, 3.25], [-7.0, 120.0], [4095.5, 4095.5]])
    x0, dx, rx, y0, ry, dy = GT
    world = np.stack((x0 + px[:, 0] * dx + px[:, 1] * rx, y0 + px[:, 0] * ry + px[:, 1] * dy), axis=1)
    back = lars.to_pixel(world, GT)
    assert back.dtype == np.float64 and np.abs(back - px).max() < 1e-6           # |world| ~ 4e6: a few ulps of it, over dx
    assert np.array_equal(lars.to_pixel(px, (0, 1, 0, 0, 0, 1)), px)
    assert lars.to_pixel(world.reshape(2, 2, 2), GT).shape == (2, 2, 2)
    for bad in ((0, 1, 2, 0, 2, 4), (0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0)):
        with pytest.raises(ValueError, match="singular|six"):
            lars.to_pixel(px, bad)
    with pytest.raises(ValueError, match="six finite"):
        lars.to_pixel(px, (0, 1, 0, np.nan, 0, 1))
    with pytest.raises(ValueError, match=r"\[\.\.\., 2\]"):
        lars.to_pixel(np.zeros((4, 3)), GT)


def test_polygons_apply_the_transform_on_the_host(no_launch):
    world = [[(500001.0, 4099990.0), (500011.0, 4099991.0), (500004.0, 4099980.0)]]
    packed = lars.Polygons(world, transform=GT)
    assert np.array_equal(packed.verts, lars.to_pixel(np.asarray(world[0]), GT)) and len(packed) == 1
    assert packed.ring_starts.tolist() == [0, 3] and packed.poly_starts.tolist() == [0, 1] and packed.ring_starts.dtype == np.int32
    with pytest.raises(ValueError, match="singular"):
        lars.Polygons(world, transform=(0, 1, 2, 0, 2, 4))
    with pytest.raises(ValueError, match="pixel coordinate beyond 1e9"):
        lars.Polygons(world, transform=(0, 1e-6, 0, 0, 0, 1e-6))
    with pytest.raises(ValueError, match="pixel coordinates already"):
        lars.rasterize_zones(lars.Polygons(world, transform=GT, want_labels=True), (4, 4), transform=GT)
    two = lars.Polygons([TRI, [rc.rect(1, 1, 9, 9), rc.rect(3, 3, 5, 5)]])
    assert two.ring_starts.tolist() == [0, 3, 7, 11] and two.poly_starts.tolist() == [0, 1, 3] and two.verts.shape == (11, 2)


RING_A = [[1.0, 1.0], [9.0, 1.0], [9.0, 9.0], [1.0, 9.0], [1.0, 1.0]]
RING_B = [[3.0, 3.0], [5.0, 3.0], [5.0, 5.0], [3.0, 5.0], [3.0, 3.0]]
RING_C = [[20.0, 2.0, 7.5], [30.0, 2.0, 7.5], [25.0, 12.0, 7.5], [20.0, 2.0, 7.5]]


def shapes_of(polygons):
    return [[np.asarray(r).shape for r in p] for p in polygons]


def test_polygons_from_geojson_types(tmp_path):
    polygon = {"type": "Polygon", "coordinates": [RING_A, RING_B]}
    multi = {"type": "MultiPolygon", "coordinates": [[RING_A, RING_B], [RING_C]]}
    got = lars.polygons_from_geojson(polygon)
    assert shapes_of(got) == [[(5, 2), (5, 2)]] and np.array_equal(got[0][1], np.asarray(RING_B))
    got = lars.polygons_from_geojson(multi)
    assert shapes_of(got) == [[(5, 2), (5, 2), (4, 2)]] and np.array_equal(got[0][2], np.asarray(RING_C)[:, :2])     # parts pooled, z dropped
    feature = {"type": "Feature", "properties": {"plot": 7}, "geometry": polygon}
    assert shapes_of(lars.polygons_from_geojson(feature)) == [[(5, 2), (5, 2)]]
    collection = {"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [RING_C]}}, feature,
                                                             {"type": "Feature", "geometry": multi}]}
    assert shapes_of(lars.polygons_from_geojson(collection)) == [[(4, 2)], [(5, 2), (5, 2)], [(5, 2), (5, 2), (4, 2)]]       # file order
    geoms = {"type": "GeometryCollection", "geometries": [polygon, multi]}
    assert shapes_of(lars.polygons_from_geojson(geoms)) == [[(5, 2), (5, 2)], [(5, 2), (5, 2), (4, 2)]]
    path = tmp_path / "plots.geojson"
    path.write_text(json.dumps(collection))
    for p in (path, str(path)):
        assert shapes_of(lars.polygons_from_geojson(p)) == shapes_of(lars.polygons_from_geojson(collection))
    packed = lars.Polygons(lars.polygons_from_geojson(collection))
    assert len(packed) == 3 and packed.poly_starts.tolist() == [0, 1, 3, 6]


def test_polygons_from_geojson_refuses_other_geometries():
    point = {"type": "Feature", "geometry": {"type": "Point", "coordinates": [1.0, 2.0]}}
    good = {"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [RING_A]}}
    with pytest.raises(ValueError, match="feature 2: geometry type 'Point'"):
        lars.polygons_from_geojson({"type": "FeatureCollection", "features": [good, good, point]})
    with pytest.raises(ValueError, match="feature 1, geometry 0: geometry type 'LineString'"):
        lars.polygons_from_geojson({"type": "FeatureCollection", "features": [good, {"type": "Feature", "geometry": {
            "type": "GeometryCollection", "geometries": [{"type": "LineString", "coordinates": RING_A}]}}]})
    with pytest.raises(ValueError, match="feature 0: the feature has no geometry"):
        lars.polygons_from_geojson({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": None}]})
    with pytest.raises(ValueError, match="no geometry"):
        lars.polygons_from_geojson({"type": "FeatureCollection", "features": []})
    with pytest.raises(ValueError, match="geometry type None"):
        lars.polygons_from_geojson({"coordinates": [RING_A]})
    with pytest.raises(TypeError, match="dict or a path"):
        lars.polygons_from_geojson([good])


# ---------------------------------------------------------------------------
# what crosses to the library
# ---------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    calls = []

    def record(name, *args):
        calls.append((name, args))
        if name.startswith("lars_h_process_image"):
            stats = args[10]._obj
            for k in range(3):
                stats[k].count = 1
            if name != "lars_h_process_image":
                args[18]._obj.value = 5
        return 0
    monkeypatch.setattr(_ffi, "call", record)
    return calls


PLANE = zc.plane(6, 9)
ZONES = zc.labels("gaps", 6, 9)[0]
IMG3 = mc.image(6, 9, 3)


def test_calls_with_a_label_raster_are_unchanged(recorded, tmp_path):
    """A label raster binds the entry points, and hands them the arguments, it always did: integer ndarrays of two dimensions, and
    nested lists of integers as well."""
    for zones in (ZONES.astype(np.uint16), ZONES.astype(np.int64), ZONES.tolist()):
        recorded.clear()
        lars.zonal_statistics(PLANE, zones, "NDWI", want_hist=True)
        lars.process_image_zones(IMG3, zones, n_zones=9, indices=["GNDVI"], nodata=7)
        (n1, a1), (n2, a2) = recorded
        assert n1 == "lars_h_zonal_stats_f32" and len(a1) == 12 and a1[4:7] == (6, 9, 5) and a1[8] == 1
        assert n2 == "lars_h_process_image_zones" and len(a2) == 25 and a2[1:8] == (6, 9, 3, _ffi.U8, 1, 2, 0) and a2[21] == 9
        assert a1[2] == a2[20] == (2 if isinstance(zones, np.ndarray) and zones.dtype == np.uint16 else 4)
    from PIL import Image
    recorded.clear()
    Image.fromarray(IMG3).save(tmp_path / "a.png")
    Image.fromarray(ZONES.astype(np.uint16)).save(tmp_path / "z.png")
    driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / "z.png")
    assert [c[0] for c in recorded] == ["lars_h_process_image_zones", "lars_h_process_image"]
    with pytest.raises(ValueError, match=r"z\.png: zones_transform goes with a \.geojson"):
        driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / "z.png", zones_transform=GT)


def test_polygons_bind_their_own_entry_points(recorded):
    polys = [TRI, [rc.rect(1, 1, 8, 5), rc.rect(3, 2, 5, 4)]]
    res = lars.zonal_statistics(PLANE, polys, "NDVI")
    (name, a), = recorded
    assert name == "lars_h_zonal_stats_polygons_f32" and len(a) == 16 and (a[2], a[4], a[6]) == (11, 3, 2) and a[8:10] == (6, 9)
    assert a[14] is None and a[15] == 0 and "labels" not in res and list(res["zone"]) == [1, 2]
    recorded.clear()
    res = lars.zonal_statistics(PLANE, lars.Polygons(polys, want_labels=True), "NDVI")
    a = recorded[0][1]
    assert a[14] is not None and a[15] == 1 and res["labels"].shape == (6, 9) and res["labels"].dtype == np.uint8
    recorded.clear()
    res = lars.process_image_zones(IMG3, lars.Polygons(rc.one_pixel_squares(300, 9), want_labels=True), indices=["NDWI"], nodata=3)
    (name, a), = recorded
    assert name == "lars_h_process_image_zones_polygons" and len(a) == 29 and a[1:8] == (6, 9, 3, _ffi.U8, 1, 4, 0) and a[15:18] == (0, 1, 3)
    assert (a[20], a[22], a[24]) == (1200, 300, 300) and a[28] == 2 and res["zones"]["labels"].dtype == np.uint16
    assert set(res["zones"]) == {"zone", "pixels", "NDWI", "labels"} and len(res["zones"]["zone"]) == 300
    recorded.clear()
    lars.rasterize_zones(polys, (7, 5))
    (name, a), = recorded
    assert name == "lars_h_rasterize_zones" and len(a) == 10 and a[6:9] == (7, 5, 1)


def test_driver_reads_polygons_from_geojson(recorded, tmp_path, monkeypatch):
    from PIL import Image
    Image.fromarray(IMG3).save(tmp_path / "a.png")
    collection = {"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [RING_A]}},
                                                             {"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [RING_B]}}]}
    for name in ("plots.geojson", "plots.JSON"):
        (tmp_path / name).write_text(json.dumps(collection))
        recorded.clear()
        driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / name, nodata=3)
        assert [c[0] for c in recorded] == ["lars_h_process_image_zones_polygons", "lars_h_process_image_masked"]
        a = recorded[0][1]
        assert (a[20], a[22], a[24]) == (10, 2, 2) and a[27] is None
    lines = (tmp_path / "out" / "a_zones.csv").read_text().splitlines()
    assert lines[0] == ",".join(driver.ZONE_CSV_COLUMNS) and len(lines) == 3
    recorded.clear()
    driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / "plots.geojson", zones_transform=(1, 2, 0, 1, 0, 2))
    verts = np.ctypeslib.as_array((__import__("ctypes").c_double * 20).from_address(recorded[0][1][19].value)).reshape(10, 2)
    assert np.array_equal(verts[:5], (np.asarray(RING_A) - 1) / 2)
    seen = {}
    monkeypatch.setattr(driver, "batch_process", lambda *a, **kw: seen.update(kw) or {})
    assert driver.main([str(tmp_path), str(tmp_path), "--zones", "plots.geojson", "--zones-transform", "1,2,0,1,0,-2", "--quiet"]) == 0
    assert seen["zones"] == "plots.geojson" and seen["zones_transform"] == (1.0, 2.0, 0.0, 1.0, 0.0, -2.0)
    seen.clear()
    assert driver.main([str(tmp_path), str(tmp_path), "--zones", "plots.geojson", "--quiet"]) == 0
    assert seen["zones"] == "plots.geojson" and "zones_transform" not in seen
    with pytest.raises(SystemExit):
        driver.main([str(tmp_path), str(tmp_path), "--zones-transform", "1,2,3", "--quiet"])


def test_the_public_names():
    for name in ("rasterize_zones", "polygons_from_geojson", "to_pixel", "Polygons"):
        assert getattr(lars, name) is getattr(zones_mod, name)
    assert zones_mod.VERTICES_MAX == 1 << 24 and zones_mod.ZONES_MAX == 65535
