"""Zones from regions on the device (csrc/regions.hip: label_regions, and zonal_statistics / process_image_zones handed a Regions)
against the NumPy model of the definition (regions_model.py).  Labels are compared byte for byte and the table exactly; the zone
figures of a call that is handed a Regions with those of the same call handed the model's raster: everything bit for bit, the mean
within the project's tolerance of 1e-6 of max(|mean|, mean|x|)."""
import functools

import numpy as np
import pytest

import masked_cases as mc
import regions_cases as gc
import regions_model as gm
import lars_image_processing_amd as lars
from test_gpu_zone_raster import same_figures, zone_meanabs      # the comparison of two zone parts, as the polygon tests make it

pytestmark = pytest.mark.gpu

T = gc.T


def width_of(n):
    return np.uint8 if n <= 255 else np.uint16 if n <= 65535 else np.int32


def check(mask, connectivity=8, min_pixels=1):
    want = gm.label(mask, connectivity, min_pixels)
    got = lars.label_regions(mask, connectivity=connectivity, min_pixels=min_pixels)
    n = want["n_regions"]
    assert got["n_regions"] == n, (got["n_regions"], n)
    assert got["labels"].dtype == width_of(n) and got["labels"].shape == want["labels"].shape
    bad = np.argwhere(got["labels"] != want["labels"])
    assert bad.size == 0, (len(bad), bad[:5].tolist(), got["labels"][tuple(bad[0])], want["labels"][tuple(bad[0])])
    assert got["area"].dtype == np.int64 and np.array_equal(got["area"], want["area"])
    assert got["bbox"].dtype == np.int32 and got["bbox"].shape == (n, 4) and np.array_equal(got["bbox"], want["bbox"])
    assert got["centroid"].dtype == np.float64 and got["centroid"].shape == (n, 2)
    assert np.array_equal(got["centroid"], gm.centroid(want))
    return got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(gc.named()))
def test_named_masks(name, connectivity):
    mask = gc.named()[name]
    got = check(mask, connectivity)
    if name == "empty":
        assert got["n_regions"] == 0 and got["area"].shape == (0,) and got["bbox"].shape == (0, 4) and not got["labels"].any()
    if name == "full":
        assert got["n_regions"] == 1 and got["bbox"].tolist() == [[0, 0, *mask.shape]] and got["area"][0] == mask.size
    if name == "checkerboard":
        assert got["n_regions"] == (int(mask.sum()) if connectivity == 4 else 1)
    if name.startswith("diagonal_"):
        assert got["n_regions"] == (2 if connectivity == 4 else 1)
    if name in ("spiral", "serpentine", "comb"):
        assert got["n_regions"] == 1 and got["labels"][0, 0] == 1


@pytest.mark.parametrize("axis", [0, 1], ids=["heights", "widths"])
def test_every_height_and_width_around_the_tile(axis):
    for n in range(1, 2 * T + 2):
        shape = (n, T + 3) if axis == 0 else (T + 3, n)
        mask = gc.random_mask(*shape, 0.5, 100 * axis + n)
        check(mask, 4 if n % 2 else 8, 1 if n % 3 else 2)
        check(mask, 8 if n % 2 else 4)


@pytest.mark.parametrize("shape", [(1, 5000), (5000, 1)])
def test_one_row_and_one_column(shape):
    mask = gc.random_mask(*shape, 0.5, 7)
    for connectivity in (4, 8):
        got = check(mask, connectivity)
        assert got["n_regions"] > 1000
    check(np.ones(shape, dtype=bool), 4)
    check(mask, 8, min_pixels=3)


@pytest.mark.parametrize("chunk", range(4))
def test_fuzz(chunk):
    seen = set()
    for seed in range(chunk * 50, chunk * 50 + 50):
        mask, connectivity, min_pixels = gc.fuzz_case(seed)
        check(mask, connectivity, min_pixels)
        seen.add((gc.DENSITIES[seed % 5], connectivity))
    assert len(seen) == 10                                            # every density under both connectivities in every chunk


@pytest.mark.parametrize("n, dtype", [(255, np.uint8), (256, np.uint16), (65535, np.uint16), (65536, np.int32)])
def test_label_width_follows_the_number_of_regions(n, dtype):
    got = check(gc.lattice(n), 8)
    assert got["n_regions"] == n and got["labels"].dtype == dtype and int(got["labels"].max()) == n
    assert (got["area"] == 1).all()


def test_integer_masks_and_min_pixels_above_every_region():
    mask = gc.random_mask(70, 90, 0.41, 3)
    a = check(mask.astype(np.int64) * 7, 8)
    b = check(mask.astype(np.uint8), 8)
    assert a["labels"].tobytes() == b["labels"].tobytes()
    assert check(mask, 8, min_pixels=10 ** 9)["n_regions"] == 0


def test_five_runs_give_the_same_bytes():
    mask = gc.random_mask(257, 300, 0.59, 11)
    runs = [lars.label_regions(mask, connectivity=4, min_pixels=2) for _ in range(5)]
    check(mask, 4, 2)
    for r in runs[1:]:
        for key in ("labels", "area", "bbox", "centroid"):
            assert r[key].tobytes() == runs[0][key].tobytes(), key


# ---------------------------------------------------------------------------
# the zone calls handed a Regions
# ---------------------------------------------------------------------------
def same_regions(part, want):
    assert np.array_equal(part["area"], want["area"]) and np.array_equal(part["bbox"], want["bbox"])
    assert np.array_equal(part["centroid"], gm.centroid(want))


SHAPES = [(64, 80), (257, 300)]
ROOM = 16384                            # max_regions of these tests: the noisy 257 x 300 picture has some 8000 regions below a threshold


@functools.lru_cache(maxsize=None)
def picture(shape, rule):
    """A picture, its valid / nodata arguments, and process_image_masked's result for them: computed once, never changed."""
    img = mc.image(*shape, 3).copy()
    img[:5, :, :] = 9
    img[shape[0] // 2, 10:40, :] = 9
    kwargs = {"none": {}, "valid": dict(valid=mc.mask("random_99", *shape)), "nodata": dict(nodata=9)}[rule]
    masked = lars.process_image_masked(img, want_hist=True, **kwargs)
    valid = {"none": None, "valid": kwargs.get("valid"), "nodata": ~(img[:, :, :3] == 9).all(axis=2)}[rule]
    img.setflags(write=False)
    return img, kwargs, masked, valid


@pytest.mark.parametrize("rule", ["none", "valid"])
@pytest.mark.parametrize("shape", SHAPES)
def test_zonal_statistics_of_regions(shape, rule):
    _, _, masked, _ = picture(shape, "none")
    plane = masked["indices"]["NDVI"]["index"]
    valid = mc.mask("random_99", *shape) if rule == "valid" else None
    for kwargs, fg in ((dict(above=0.3), plane > np.float32(0.3)), (dict(below=0.25, connectivity=4, min_pixels=3), plane < np.float32(0.25)),
                       (dict(mask=gc.random_mask(*shape, 0.55, 5), connectivity=4, min_pixels=2), gc.random_mask(*shape, 0.55, 5))):
        fg = fg if valid is None else fg & valid
        model = gm.label(fg, kwargs.get("connectivity", 8), kwargs.get("min_pixels", 1))
        n = model["n_regions"]
        assert 3 < n <= ROOM, n
        want = lars.zonal_statistics(plane, model["labels"], "NDVI", valid=valid, n_zones=n, want_hist=True)
        got = lars.zonal_statistics(plane, lars.Regions(want_labels=True, max_regions=ROOM, **kwargs), "NDVI", valid=valid, want_hist=True)
        assert np.array_equal(got["zone"], np.arange(1, n + 1)) and np.array_equal(got["pixels"], model["area"])
        same_figures(got, want, zone_meanabs(plane, model["labels"], valid, n))
        same_regions(got["regions"], model)
        assert got["labels"].dtype == width_of(n) and np.array_equal(got["labels"], model["labels"])
        plain = lars.zonal_statistics(plane, lars.Regions(max_regions=ROOM, **kwargs), "NDVI", valid=valid, want_hist=True)
        assert "labels" not in plain and set(plain) == set(want) | {"regions"}
        same_figures(plain, want, zone_meanabs(plane, model["labels"], valid, n))
        rows = lars.zonal_rows(got, "NDVI")
        assert len(rows) == n and rows[0]["Zone"] == 1 and rows[-1]["Pixels"] == int(model["area"][-1])


@pytest.mark.parametrize("rule", ["none", "valid", "nodata"])
@pytest.mark.parametrize("shape", SHAPES)
def test_process_image_zones_of_regions(shape, rule):
    img, kwargs, masked, valid = picture(shape, rule)
    for index, how in (("NDVI", dict(above=0.3, min_pixels=2)), ("NDWI", dict(below=-0.3, connectivity=4))):
        plane = masked["indices"][index]["index"]
        fg = (plane > np.float32(0.3)) if "above" in how else (plane < np.float32(-0.3))
        fg = fg if valid is None else fg & valid
        model = gm.label(fg, how.get("connectivity", 8), how.get("min_pixels", 1))
        n = model["n_regions"]
        assert 3 < n <= ROOM, n
        want = lars.process_image_zones(img, model["labels"], n_zones=n, want_hist=True, **kwargs)
        got = lars.process_image_zones(img, lars.Regions(index=index, want_labels=True, max_regions=ROOM, **how), want_hist=True, **kwargs)
        assert set(got["zones"]) == set(want["zones"]) | {"labels", "regions"}
        assert np.array_equal(got["zones"]["labels"], model["labels"]) and got["zones"]["labels"].dtype == width_of(n)
        same_regions(got["zones"]["regions"], model)
        assert np.array_equal(got["zones"]["zone"], want["zones"]["zone"]) and np.array_equal(got["zones"]["pixels"], want["zones"]["pixels"])
        # the picture-level results are process_image_masked's, byte for byte
        assert got["valid_pixels"] == masked.get("valid_pixels", shape[0] * shape[1])      # without a rule that call is process_image's
        assert got["corrected"].tobytes() == masked["corrected"].tobytes()
        for t in ("NDVI", "GNDVI", "NDWI"):
            mine, theirs = got["indices"][t], masked["indices"][t]
            assert mine["index"].tobytes() == theirs["index"].tobytes()
            assert mine["stats"] == theirs["stats"] and np.array_equal(mine["hist"], theirs["hist"])
            a = {"pixels": got["zones"]["pixels"], **got["zones"][t]}
            b = {"pixels": want["zones"]["pixels"], **want["zones"][t]}
            same_figures(a, b, zone_meanabs(mine["index"], model["labels"], valid, n))
        assert len(lars.zonal_rows(got, index)) == n


def test_a_host_mask_on_a_picture_and_fewer_indices():
    img, kwargs, masked, valid = picture((64, 80), "nodata")
    mask = gc.random_mask(64, 80, 0.5, 21)
    model = gm.label(mask & valid, 8, 2)
    n = model["n_regions"]
    want = lars.process_image_zones(img, model["labels"], n_zones=n, indices=["GNDVI"], **kwargs)
    got = lars.process_image_zones(img, lars.Regions(mask=mask, min_pixels=2, want_labels=True), indices=["GNDVI"], **kwargs)
    assert np.array_equal(got["zones"]["labels"], model["labels"])
    same_regions(got["zones"]["regions"], model)
    a = {"pixels": got["zones"]["pixels"], **got["zones"]["GNDVI"], "hist": 0}
    b = {"pixels": want["zones"]["pixels"], **want["zones"]["GNDVI"], "hist": 0}
    same_figures(a, b, zone_meanabs(got["indices"]["GNDVI"]["index"], model["labels"], valid, n))


def test_no_region_is_a_result():
    img, kwargs, masked, _ = picture((64, 80), "none")
    plane = masked["indices"]["NDVI"]["index"]
    got = lars.zonal_statistics(plane, lars.Regions(above=2.0, want_labels=True), "NDVI", want_hist=True)
    assert got["zone"].shape == (0,) and got["pixels"].shape == (0,) and got["mean"].shape == (0,) and got["hist"].shape == (0, 50)
    assert got["regions"]["area"].shape == (0,) and got["regions"]["bbox"].shape == (0, 4) and got["regions"]["centroid"].shape == (0, 2)
    assert got["labels"].dtype == np.uint8 and not got["labels"].any()
    assert lars.zonal_rows(got, "NDVI") == []
    pic = lars.process_image_zones(img, lars.Regions(index="NDVI", above=2.0), **kwargs)
    assert pic["zones"]["zone"].shape == (0,) and pic["zones"]["pixels"].shape == (0,) and pic["zones"]["NDVI"]["median"].shape == (0,)
    assert pic["corrected"].tobytes() == masked["corrected"].tobytes()
    few = lars.zonal_statistics(plane, lars.Regions(above=0.3, min_pixels=10 ** 7), "NDVI")
    assert few["zone"].shape == (0,)


def test_more_regions_than_room_raise_with_their_number():
    board = gc.named()["checkerboard"]
    n = int(board.sum())
    plane = np.where(board, np.float32(0.5), np.float32(0.0))
    with pytest.raises(ValueError, match=rf"zonal_statistics: {n} regions, more than max_regions = 100: raise min_pixels .* or max_regions"):
        lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, max_regions=100), "NDVI")
    assert lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, max_regions=n), "NDVI")["zone"].shape == (n,)
    with pytest.raises(ValueError, match=rf"{n} regions, more than max_regions = {n - 1}"):
        lars.zonal_statistics(plane, lars.Regions(mask=board, connectivity=4, max_regions=n - 1), "NDVI")
    lattice = gc.lattice(65536)
    dots = np.where(lattice, np.float32(0.5), np.float32(0.0))
    with pytest.raises(ValueError, match="zonal_statistics: 65536 regions, more than max_regions = 65535.*at most 65535 regions"):
        lars.zonal_statistics(dots, lars.Regions(above=0.2, max_regions=65535), "NDVI")
    img, kwargs, _, _ = picture((64, 80), "none")
    with pytest.raises(ValueError, match=r"process_image_zones: \d+ regions, more than max_regions = 2"):
        lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.3, max_regions=2), **kwargs)


def test_driver_writes_the_regions_csv(tmp_path):
    import csv

    from PIL import Image

    from lars_image_processing_amd import driver
    img = mc.image(64, 80, 3)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(img).save(src / "field.png")
    flags = ["--ndvi", "--gndvi", "--no-ndwi", "--workers", "1", "--quiet"]
    assert driver.main([str(src), str(tmp_path / "out"), *flags, "--regions", "GNDVI:above:0.25:2"]) == 0
    rows = list(csv.reader(open(tmp_path / "out" / "field_zones.csv")))
    want = lars.process_image_zones(img, lars.Regions(index="GNDVI", above=0.25, min_pixels=2), indices=["NDVI", "GNDVI"], want_arrays=False)
    n = len(want["zones"]["zone"])
    assert n > 3 and tuple(rows[0]) == driver.ZONE_CSV_COLUMNS + driver.REGION_CSV_COLUMNS and len(rows) == 1 + 2 * n
    table = want["zones"]["regions"]
    for k, t in enumerate(("NDVI", "GNDVI")):
        for i, row in enumerate(rows[1 + k * n:1 + (k + 1) * n]):
            assert row[:3] == [str(i + 1), t, str(int(want["zones"]["pixels"][i]))]
            assert float(row[3]) == want["zones"][t]["mean"][i] and float(row[4]) == want["zones"][t]["median"][i]
            assert [int(v) for v in row[8:13]] == [int(table["area"][i])] + table["bbox"][i].tolist()
            assert [float(v) for v in row[13:15]] == table["centroid"][i].tolist()
    assert driver.main([str(src), str(tmp_path / "plain"), *flags]) == 0
    assert not (tmp_path / "plain" / "field_zones.csv").exists()
    assert driver.main([str(src), str(tmp_path / "bad"), *flags, "--regions", "NDWI:above:0.0"]) == 1      # NDWI is not asked for
