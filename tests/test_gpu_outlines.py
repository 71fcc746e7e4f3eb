"""Region outlines on the device (csrc/outlines.hip: region_outlines, and the zone calls handed a Regions(want_outlines=True)) against
the model of the definition (outlines_model.py) on the model's labels (regions_model.py): vertices, ring starts, polygon starts, doubled
areas, labels and table, all bit for bit."""
import json

import numpy as np
import pytest

import outlines_model as om
import regions_cases as gc
import regions_model as gm
import lars_image_processing_amd as lars
from test_gpu_regions import ROOM, SHAPES, picture, same_regions, width_of
from test_gpu_zone_raster import same_figures, zone_meanabs

pytestmark = pytest.mark.gpu


def same_outlines(part, labels, n, connectivity):
    """``part`` holds the model's outlines of ``labels``; returns the model's trace."""
    want = om.trace(labels, connectivity)
    assert (part["n_rings"], part["n_vertices"]) == (want["n_rings"], want["n_vertices"]), (part["n_rings"], part["n_vertices"], want["n_rings"], want["n_vertices"])
    assert part["ring_area2"].dtype == np.int64 and np.array_equal(part["ring_area2"], want["ring_area2"])
    if n == 0:
        assert part["outlines"] is None and part["ring_area2"].shape == (0,) and part["n_rings"] == 0 and part["n_vertices"] == 0
        return want
    verts, ring_starts, poly_starts = om.polygons(want, n)
    p = part["outlines"]
    assert isinstance(p, lars.Polygons) and len(p) == n
    assert p.verts.dtype == np.float64 and p.verts.flags["C_CONTIGUOUS"] and p.ring_starts.dtype == np.int32 and p.poly_starts.dtype == np.int32
    assert np.array_equal(p.ring_starts, ring_starts), (p.ring_starts[:8], ring_starts[:8])
    assert np.array_equal(p.poly_starts, poly_starts)
    bad = np.flatnonzero((p.verts != verts).any(axis=1))
    assert bad.size == 0, (len(bad), bad[:5].tolist(), p.verts[bad[:5]].tolist(), verts[bad[:5]].tolist())
    return want


def check(mask, connectivity=8, min_pixels=1):
    model = gm.label(mask, connectivity, min_pixels)
    got = lars.region_outlines(mask, connectivity=connectivity, min_pixels=min_pixels)
    n = model["n_regions"]
    assert got["n_regions"] == n, (got["n_regions"], n)
    assert got["labels"].dtype == width_of(n) and np.array_equal(got["labels"], model["labels"])
    same_regions(got, model)
    same_outlines(got, model["labels"], n, connectivity)
    return got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(gc.named()))
def test_named_masks(name, connectivity):
    got = check(gc.named()[name], connectivity)
    if name == "full":
        assert got["outlines"].verts.tolist() == [[0, 0], [gc.T + 3, 0], [gc.T + 3, 2 * gc.T + 1], [0, 2 * gc.T + 1]]
    if name.startswith("diagonal_"):
        assert (got["n_rings"], got["n_vertices"]) == ((2, 8) if connectivity == 4 else (1, 8))


@pytest.mark.parametrize("axis", [0, 1], ids=["heights", "widths"])
def test_every_height_and_width_across_tile_and_wave(axis):
    for n in range(1, 67):
        shape = (n, 37) if axis == 0 else (37, n)
        check(gc.random_mask(*shape, 0.5, 100 * axis + n), 4 if n % 2 else 8)
        check(gc.random_mask(*shape, 0.5, 100 * axis + n), 8 if n % 2 else 4, 1 if n % 3 else 2)


@pytest.mark.parametrize("shape", [(1, 5000), (5000, 1)])
def test_one_row_and_one_column(shape):
    mask = gc.random_mask(*shape, 0.5, 7)
    for connectivity in (4, 8):
        got = check(mask, connectivity)
        assert got["n_rings"] == got["n_regions"] > 1000 and got["n_vertices"] == 4 * got["n_rings"]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_all_masks_of_three_by_three(connectivity):
    raster = np.zeros((3, 4 * 512), dtype=bool)                       # three pixels cannot reach across the background column
    for k in range(512):
        raster[:, 4 * k:4 * k + 3] = ((k >> np.arange(9).reshape(3, 3)) & 1) != 0
    check(raster, connectivity)


def test_a_ring_longer_than_every_block():
    got = check(gc.spiral(260, 260), 8)
    assert got["n_rings"] == 1 and int(got["ring_area2"][0]) == 2 * int(got["area"][0])
    assert 2 * int(got["area"][0]) + 2 > 1 << 16                      # the edges of a one-pixel-wide path: 17 rounds of pointer doubling


def test_checkerboard():
    y, x = np.mgrid[0:64, 0:64]
    board = (x + y) % 2 == 0
    four = check(board, 4)
    assert (four["n_regions"], four["n_rings"], four["n_vertices"]) == (2048, 2048, 8192)
    eight = check(board, 8)
    assert eight["n_regions"] == 1 and eight["n_rings"] > 900 and (eight["ring_area2"][1:] == -2).all()


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz(chunk):
    for seed in range(chunk * 50, chunk * 50 + 50):
        mask, connectivity, min_pixels = gc.fuzz_case(seed, most=96)
        check(mask, connectivity, min_pixels)


def test_min_pixels_above_every_region():
    got = check(gc.random_mask(70, 90, 0.41, 3), 8, min_pixels=10 ** 9)
    assert got["n_regions"] == 0 and got["outlines"] is None and got["ring_area2"].shape == (0,) and not got["labels"].any()


def test_five_runs_give_the_same_bytes():
    mask = gc.random_mask(257, 300, 0.59, 11)
    runs = [lars.region_outlines(mask, connectivity=4, min_pixels=2) for _ in range(5)]
    check(mask, 4, 2)
    for r in runs[1:]:
        for key in ("labels", "area", "bbox", "centroid", "ring_area2"):
            assert r[key].tobytes() == runs[0][key].tobytes(), key
        for key in ("verts", "ring_starts", "poly_starts"):
            assert getattr(r["outlines"], key).tobytes() == getattr(runs[0]["outlines"], key).tobytes(), key


@pytest.mark.parametrize("seed", [3, 9, 17])
def test_rasterising_the_outlines_gives_the_labels_back(seed):
    mask, connectivity, min_pixels = gc.fuzz_case(seed, most=96)
    got = lars.region_outlines(mask, connectivity=connectivity, min_pixels=min_pixels)
    assert got["n_regions"] > 0
    assert np.array_equal(lars.rasterize_zones(got["outlines"], mask.shape), got["labels"])


@pytest.mark.parametrize("shape", SHAPES)
def test_zonal_statistics_with_outlines(shape):
    _, _, masked, _ = picture(shape, "none")
    plane = masked["indices"]["NDVI"]["index"]
    plain = lars.zonal_statistics(plane, lars.Regions(above=0.2, max_regions=ROOM), "NDVI", want_hist=True)
    got = lars.zonal_statistics(plane, lars.Regions(above=0.2, max_regions=ROOM, want_labels=True, want_outlines=True), "NDVI", want_hist=True)
    n = len(got["zone"])
    assert n > 3 and set(got) == set(plain) | {"labels", "outlines", "ring_area2", "n_rings", "n_vertices"}
    assert np.array_equal(got["zone"], plain["zone"])
    same_figures(got, plain, zone_meanabs(plane, got["labels"], None, n))
    assert np.array_equal(got["labels"], gm.label(plane > np.float32(0.2), 8)["labels"])
    same_outlines(got, got["labels"], n, 8)


@pytest.mark.parametrize("shape", SHAPES)
def test_process_image_zones_with_outlines(shape):
    img, kwargs, masked, _ = picture(shape, "none")
    plain = lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, max_regions=ROOM), want_hist=True, **kwargs)
    got = lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, max_regions=ROOM, want_labels=True, want_outlines=True), want_hist=True,
                                   **kwargs)
    n = len(got["zones"]["zone"])
    assert n > 3 and set(got["zones"]) == set(plain["zones"]) | {"labels", "outlines", "ring_area2", "n_rings", "n_vertices"}
    assert np.array_equal(got["zones"]["pixels"], plain["zones"]["pixels"]) and got["corrected"].tobytes() == plain["corrected"].tobytes()
    for t in ("NDVI", "GNDVI", "NDWI"):
        a = {"pixels": got["zones"]["pixels"], **got["zones"][t]}
        b = {"pixels": plain["zones"]["pixels"], **plain["zones"][t]}
        same_figures(a, b, zone_meanabs(got["indices"][t]["index"], got["zones"]["labels"], None, n))
    assert np.array_equal(got["zones"]["labels"], gm.label(masked["indices"]["NDVI"]["index"] > np.float32(0.2), 8)["labels"])
    same_outlines(got["zones"], got["zones"]["labels"], n, 8)


def test_more_vertices_than_room_raise_with_their_number():
    img, kwargs, masked, _ = picture((64, 80), "none")
    plane = masked["indices"]["NDVI"]["index"]
    model = gm.label(plane > np.float32(0.2), 4)
    v = om.trace(model["labels"], 4)["n_vertices"]
    assert v > 16
    with pytest.raises(ValueError, match=rf"zonal_statistics: the outlines have {v} vertices, more than max_vertices = {v - 1}: raise min_pixels .* or max_vertices"):
        lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, want_outlines=True, max_vertices=v - 1), "NDVI")
    assert lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, want_outlines=True, max_vertices=v), "NDVI")["n_vertices"] == v
    with pytest.raises(ValueError, match=rf"process_image_zones: the outlines have {v} vertices, more than max_vertices = 16"):
        lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, connectivity=4, want_outlines=True, max_vertices=16), **kwargs)


def test_driver_writes_the_regions_geojson(tmp_path):
    import masked_cases as mc
    from PIL import Image

    from lars_image_processing_amd import driver
    img = mc.image(64, 80, 3)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(img).save(src / "field.png")
    flags = ["--ndvi", "--gndvi", "--no-ndwi", "--workers", "1", "--quiet", "--regions", "GNDVI:above:0.25:2"]
    assert driver.main([str(src), str(tmp_path / "out"), *flags, "--regions-geojson"]) == 0
    want = lars.process_image_zones(img, lars.Regions(index="GNDVI", above=0.25, min_pixels=2, want_outlines=True), indices=["NDVI", "GNDVI"],
                                    want_arrays=False)
    zones = want["zones"]
    n = len(zones["zone"])
    path = tmp_path / "out" / "field_regions.geojson"
    assert (tmp_path / "out" / "field_zones.csv").exists() and n > 3
    back = lars.polygons_from_geojson(path)
    assert len(back) == n
    for k in range(n):                                                # the same rings, each closed by its first vertex
        rings = zones["outlines"].rings(k)
        assert len(back[k]) == len(rings)
        for mine, theirs in zip(back[k], rings):
            assert np.array_equal(mine[:-1], theirs) and np.array_equal(mine[-1], theirs[0])
    features = json.load(open(path))["features"]
    table = zones["regions"]
    for i in (0, n - 1):
        props = features[i]["properties"]
        assert props["Zone"] == i + 1 and props["Area"] == int(table["area"][i]) and props["Pixels"] == int(zones["pixels"][i])
        assert [props[c] for c in ("Row0", "Col0", "Row1", "Col1")] == table["bbox"][i].tolist()
        assert [props["Centroid Row"], props["Centroid Col"]] == table["centroid"][i].tolist()
        assert props["Mean GNDVI"] == zones["GNDVI"]["mean"][i] and props["Median NDVI"] == zones["NDVI"]["median"][i]
    shifted = tmp_path / "shifted"
    assert driver.main([str(src), str(shifted), *flags, "--regions-geojson", "--zones-transform", "100,0.5,0,200,0,-0.5"]) == 0
    world = lars.Polygons(lars.polygons_from_geojson(shifted / "field_regions.geojson"), transform=(100, 0.5, 0, 200, 0, -0.5))
    assert np.array_equal(lars.rasterize_zones(world, (64, 80)), lars.rasterize_zones(zones["outlines"], (64, 80)))
    assert driver.main([str(src), str(tmp_path / "plain"), *flags]) == 0
    assert not (tmp_path / "plain" / "field_regions.geojson").exists()
