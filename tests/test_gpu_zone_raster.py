"""Zones from polygons on the device (csrc/zone_raster.hip: rasterize_zones, and process_image_zones / zonal_statistics / the driver
handed polygons) against the NumPy model of the definition (zone_raster_model.py).  Labels are compared for byte equality; the zone
figures of a call that is handed polygons with those of the same call handed the model's raster: everything bit for bit, the mean
within the project's tolerance of 1e-6 of max(|mean|, mean|x|)."""
import csv
import functools
import json

import numpy as np
import pytest

import masked_cases as mc
import zonal_cases as zc
import zone_raster_cases as rc
import zone_raster_model as zrm
import lars_image_processing_amd as lars
from lars_image_processing_amd import driver

pytestmark = pytest.mark.gpu


def check(polygons, shape):
    want = zrm.labels(polygons, shape)
    got = lars.rasterize_zones(polygons, shape)
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return got


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_named_cases(name):
    polygons, shape = rc.CASES[name]
    got = check(polygons, shape)
    present = set(np.unique(got).tolist()) - {0}
    if name in ("sliver", "zero_area", "outside"):
        assert present == {len(polygons) if name != "zero_area" else 2}            # the other zones are empty, and no error
    if name in ("whole_raster", "whole_raster_exactly"):
        assert (got == 1).all()
    if name == "bow_tie":
        assert got[15, 5] == 1 and got[15, 28] == 1 and got[4, 16] == 0 and got[26, 16] == 0  # the two triangles, not what lies between them
    if name == "hole":
        assert got[14, 17] == 0 and got[5, 5] == 1


@pytest.mark.parametrize("name", ["vertices_on_centres", "horizontal_edges_on_row_centres", "edges_through_centres"])
def test_ties_against_the_exact_rule(name):
    polygons, shape = rc.CASES[name]
    assert np.array_equal(lars.rasterize_zones(polygons, shape), zrm.labels_exact(polygons, shape))


@pytest.mark.parametrize("axis", [0, 1], ids=["rows", "columns"])
@pytest.mark.parametrize("n", rc.SIZES)
def test_widths_and_heights(n, axis):
    check(*rc.size_case(n, axis))


def test_a_grid_of_quads_covers_every_pixel_once():
    shape = (61, 83)
    quads = rc.jittered_grid(6, 7, shape)
    got = check(quads, shape)
    assert got.min() >= 1
    alone = sum((lars.rasterize_zones([q], shape) != 0).astype(np.int32) for q in quads)
    assert alone.min() == 1 and alone.max() == 1                                   # of two plots that share an edge exactly one takes each pixel
    snapped = rc.jittered_grid(6, 7, shape, seed=9, snap=8)
    assert np.array_equal(check(snapped, shape), zrm.labels_exact(snapped, shape))


@pytest.mark.parametrize("name", ["nested", "crossing"])
def test_the_later_polygon_wins_in_either_order(name):
    polygons, shape = rc.CASES[name]
    a, b = check(polygons, shape), check(polygons[::-1], shape)
    assert np.array_equal(a != 0, b != 0) and not np.array_equal(a, b)
    if name == "nested":
        assert set(np.unique(a).tolist()) == {0, 1, 2, 3} and set(np.unique(b).tolist()) == {0, 3}   # the outer one, now last, hides the others


@pytest.mark.parametrize("z, dtype", [(255, np.uint8), (256, np.uint16), (257, np.uint16)])
def test_label_width_follows_the_number_of_polygons(z, dtype):
    squares = rc.one_pixel_squares(z, width=20)
    got = check(squares, (14, 20))
    assert got.dtype == dtype and got.reshape(-1)[:z].tolist() == list(range(1, z + 1)) and not got.reshape(-1)[z:].any()


def test_65535_polygons():
    got = lars.rasterize_zones(rc.one_pixel_squares(65535), (256, 256))
    want = np.arange(1, 65537, dtype=np.int64)
    want[-1] = 0
    assert got.dtype == np.uint16 and np.array_equal(got.reshape(-1), want)
    with pytest.raises(ValueError, match="65536 polygons; at most 65535"):
        lars.rasterize_zones(rc.one_pixel_squares(65536), (256, 256))


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz(chunk):
    for seed in range(chunk * 50, chunk * 50 + 50):
        polygons, shape = rc.fuzz_case(seed)
        want, got = zrm.labels(polygons, shape), lars.rasterize_zones(polygons, shape)
        assert np.array_equal(got, want), (seed, shape, len(polygons), np.argwhere(got != want)[:3].tolist())


def test_two_runs_agree():
    polygons = rc.jittered_grid(9, 11, (300, 290), seed=3) + rc.CASES["star_5000"][0] + [rc.rect(20.2, 30.3, 250.5, 260.6)]
    a = lars.rasterize_zones(polygons, (300, 290))
    b = lars.rasterize_zones(polygons, (300, 290))
    assert a.tobytes() == b.tobytes() and np.array_equal(a, zrm.labels(polygons, (300, 290)))


# ---------------------------------------------------------------------------
# the zone calls handed polygons
# ---------------------------------------------------------------------------
FIELD = (96, 131)


@functools.lru_cache(maxsize=None)
def field():
    """Plots that share edges, one that covers nothing, one with a hole, one cut by the border; the model's raster of them."""
    polygons = rc.jittered_grid(4, 5, FIELD, seed=11)[3:15] + [[(1.1, 5.6), (30.3, 5.7), (30.3, 5.75), (1.1, 5.65)],
                                                               [rc.rect(70.3, 50.2, 140.0, 90.6), rc.rect(80.1, 60.7, 100.8, 80.2)]]
    labels = zrm.labels(polygons, FIELD)
    labels.setflags(write=False)
    return polygons, labels


def zone_meanabs(plane, labels, valid, nz):
    lab = labels.astype(np.int64).ravel() if valid is None else np.where(valid.ravel(), labels.astype(np.int64).ravel(), 0)
    x = np.abs(np.nan_to_num(plane.astype(np.float64).ravel()))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.bincount(lab, weights=x, minlength=nz + 1) / np.bincount(lab, minlength=nz + 1))[1:]


def same_figures(a, b, meanabs):
    """Two zone parts ({pixels, mean, median, ...}): everything bit for bit, the mean within 1e-6 of max(|mean|, mean|x|)."""
    for key in ("pixels", "median", "min", "max", "coverage", "hist"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.array_equal(np.isnan(a["mean"]), np.isnan(b["mean"]))
    ok = ~np.isnan(a["mean"])
    assert (np.abs(a["mean"] - b["mean"])[ok] <= 1e-6 * np.maximum(np.abs(b["mean"]), meanabs)[ok]).all()


@pytest.mark.parametrize("masked", [False, True])
def test_zonal_statistics_of_polygons(masked):
    polygons, labels = field()
    plane = zc.plane(*FIELD)
    valid = zc.valid_mask(*FIELD) if masked else None
    want = lars.zonal_statistics(plane, labels, "NDVI", valid=valid, n_zones=len(polygons), want_hist=True)
    got = lars.zonal_statistics(plane, lars.Polygons(polygons, want_labels=True), "NDVI", valid=valid, want_hist=True)
    assert np.array_equal(got["zone"], want["zone"]) and got["pixels"][12] == 0 and got["pixels"].sum() > 4000
    same_figures(got, want, zone_meanabs(plane, labels, valid, len(polygons)))
    assert got["labels"].dtype == np.uint8 and np.array_equal(got["labels"], labels)
    plain = lars.zonal_statistics(plane, polygons, "NDVI", valid=valid, want_hist=True)
    assert "labels" not in plain
    same_figures(plain, want, zone_meanabs(plane, labels, valid, len(polygons)))


@pytest.mark.parametrize("rule", ["none", "valid", "nodata"])
def test_process_image_zones_of_polygons(rule):
    polygons, labels = field()
    img = mc.image(*FIELD, 3).copy()
    img[:9, :, :] = 9
    kwargs = {"none": {}, "valid": dict(valid=zc.valid_mask(*FIELD)), "nodata": dict(nodata=9)}[rule]
    want = lars.process_image_zones(img, labels, n_zones=len(polygons), want_hist=True, **kwargs)
    got = lars.process_image_zones(img, lars.Polygons(polygons, want_labels=True), want_hist=True, **kwargs)
    assert got["valid_pixels"] == want["valid_pixels"] and np.array_equal(got["corrected"], want["corrected"])
    assert np.array_equal(got["zones"]["labels"], labels) and np.array_equal(got["zones"]["pixels"], want["zones"]["pixels"])
    assert set(got["zones"]) == set(want["zones"]) | {"labels"}
    valid = {"none": None, "valid": kwargs.get("valid"), "nodata": ~(img[:, :, :3] == 9).all(axis=2)}[rule]
    for t in ("NDVI", "GNDVI", "NDWI"):
        plane = got["indices"][t]["index"]
        assert np.array_equal(plane.view(np.uint32), want["indices"][t]["index"].view(np.uint32))
        a = {"pixels": got["zones"]["pixels"], **got["zones"][t]}
        b = {"pixels": want["zones"]["pixels"], **want["zones"][t]}
        same_figures(a, b, zone_meanabs(plane, labels, valid, len(polygons)))


def test_transform_equals_transformed_vertices():
    polygons, labels = field()
    gt = (500000.0, 0.25, 0.03, 4100000.0, -0.02, -0.25)
    x0, dx, rx, y0, ry, dy = gt
    world = [[np.stack((x0 + r[:, 0] * dx + r[:, 1] * rx, y0 + r[:, 0] * ry + r[:, 1] * dy), axis=1) for r in zrm.rings_of(p)] for p in polygons]
    pixels = [[lars.to_pixel(r, gt) for r in p] for p in world]
    want = zrm.labels(pixels, FIELD)
    assert np.array_equal(lars.rasterize_zones(world, FIELD, transform=gt), want)
    assert np.array_equal(lars.rasterize_zones(pixels, FIELD), want)
    got = lars.zonal_statistics(zc.plane(*FIELD), lars.Polygons(world, transform=gt, want_labels=True), "NDWI")
    assert np.array_equal(got["labels"], want)


def test_driver_writes_the_rows_of_the_models_raster(tmp_path):
    from PIL import Image
    polygons, labels = field()
    src = tmp_path / "in"
    src.mkdir()
    img = mc.image(*FIELD, 3)
    Image.fromarray(img).save(src / "field.png")
    Image.fromarray(labels.astype(np.uint16)).save(tmp_path / "plots.png")
    features = [{"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [np.vstack((r, r[:1])).tolist() for r in zrm.rings_of(p)]}}
                for p in polygons]
    (tmp_path / "plots.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": features}))
    assert driver.main([str(src), str(tmp_path / "a"), "--ndvi", "--workers", "1", "--quiet", "--zones", str(tmp_path / "plots.geojson")]) == 0
    assert driver.main([str(src), str(tmp_path / "b"), "--ndvi", "--workers", "1", "--quiet", "--zones", str(tmp_path / "plots.png")]) == 0
    rows = []
    for d in ("a", "b"):
        with open(tmp_path / d / "field_zones.csv", newline="") as f:
            rows.append(list(csv.DictReader(f)))
    # the label raster's largest label is the last polygon that covers a pixel; the polygons' file has a row for every polygon
    assert len(rows[0]) == 2 * len(polygons) and len(rows[1]) == 2 * int(labels.max()) == len(rows[0])
    planes = lars.process_image(img, indices=["NDVI", "NDWI"])["indices"]
    meanabs = {t: zone_meanabs(planes[t]["index"], labels, None, len(polygons)) for t in planes}
    for a, b in zip(*rows):
        assert {k: v for k, v in a.items() if k != "Mean"} == {k: v for k, v in b.items() if k != "Mean"}
        bound = 1e-6 * max(abs(float(b["Mean"])), meanabs[b["Index"]][int(b["Zone"]) - 1])
        assert a["Mean"] == b["Mean"] == "nan" or abs(float(a["Mean"]) - float(b["Mean"])) <= bound
