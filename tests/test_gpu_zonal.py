"""Zonal statistics on the device (csrc/zonal.hip: zonal_statistics, process_image_zones, the driver's zones=) against the NumPy
model of the definition (zonal_model.py): pixel counts, median, min, max, coverage and histogram bit for bit, the mean within the
project's tolerance of 1e-6 of max(|mean|, mean|x|) against the float64 mean."""
import csv
import functools

import numpy as np
import pytest

import masked_cases as mc
import masked_model as mm
import zonal_cases as zc
import zonal_model as zm
import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, driver

pytestmark = pytest.mark.gpu

ALL = list(mm.INDEX_NAMES)
SPLIT_FLOOR = 64


@functools.lru_cache(maxsize=None)
def plane(h, w):
    x = zc.plane(h, w)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def picture(h, w, c=3, dtype="uint8"):
    img = mc.image(h, w, c, np.dtype(dtype))
    img.setflags(write=False)
    return img


def check_plane(x, labels, nz, index_type="NDVI", valid=None, dtype=np.int32, **kw):
    want = zm.zonal_model(x, labels, index_type, valid, nz)
    got = lars.zonal_statistics(x, labels.astype(dtype), index_type, valid=valid, n_zones=nz, want_hist=True, **kw)
    zm.check_zone_figures(got, want, index_type)
    return got, want


def id_of(v):
    return v if isinstance(v, str) else "x".join(map(str, v))


@pytest.mark.parametrize("shape, layout", zc.shape_layout_cases(), ids=id_of)
def test_shapes_and_layouts(shape, layout):
    h, w = shape
    labels, nz = zc.labels(layout, h, w)
    got, _ = check_plane(plane(h, w), labels, nz, "NDVI" if (h + w) % 2 else "NDWI", dtype=np.uint8 if nz < 256 else np.uint16)
    if layout == "all_zero":
        assert not got["pixels"].any() and np.isnan(got["median"]).all() and not got["hist"].any()
    if layout == "gaps":
        assert got["pixels"][2] == 0 and got["pixels"][5] == 0 and np.isnan(got["mean"][[2, 5]]).all() and got["pixels"][[0, 1, 3, 4]].all()
    if layout == "tiny_zones":
        assert list(got["pixels"][:4]) == [1, 2, 3, 4]


@pytest.mark.parametrize("shape", [(1, 65), (33, 65), (255, 257)], ids=id_of)
def test_with_a_valid_mask(shape):
    h, w = shape
    labels, nz = zc.labels("stripes65", h, w)
    valid = zc.valid_mask(h, w)
    got, _ = check_plane(plane(h, w), labels, nz, "GNDVI", valid=valid)
    assert got["pixels"].sum() == valid.sum()
    check_plane(plane(h, w), labels, nz, "GNDVI", valid=valid.astype(np.int16) * 3)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32, np.int64])
def test_label_types(dtype):
    labels, nz = zc.labels("grid8", 33, 65)
    check_plane(plane(33, 65), labels, nz, dtype=dtype)


def test_n_zones_defaults_to_the_largest_label():
    labels, nz = zc.labels("gaps", 33, 65)                     # zone 6 never occurs: the largest label is 5
    got = lars.zonal_statistics(plane(33, 65), labels, "NDVI")
    assert list(got["zone"]) == [1, 2, 3, 4, 5] and "hist" not in got
    zm.check_zone_figures(got, zm.zonal_model(plane(33, 65), labels, "NDVI"), "NDVI", want_hist=False)


def test_random_labels_2000_zones():
    labels = zc.random_labels(512, 512, 2000)
    check_plane(plane(512, 512), labels, 2000, dtype=np.uint16)


def test_65535_zones_mostly_empty():
    labels = zc.sparse_labels(255, 257)
    got, _ = check_plane(plane(255, 257), labels, 65535, "NDWI", dtype=np.uint16)
    assert got["pixels"][0] > 0 and got["pixels"][-1] > 0 and np.count_nonzero(got["pixels"]) < 300


def test_a_nan_spoils_its_zone_only():
    labels, nz = zc.labels("grid8", 33, 65)
    x = plane(33, 65).copy()
    x[12, 23] = np.nan                                         # inside plot (1, 2)
    hit = labels[12, 23]
    assert hit > 0
    got, want = check_plane(x, labels, nz)
    assert np.isnan([got[f][hit - 1] for f in ("mean", "median", "min", "max")]).all() and not np.isnan(got["coverage"][hit - 1])
    assert got["pixels"][hit - 1] == 64 and got["hist"][hit - 1].sum() == 63
    others = np.delete(np.arange(nz), hit - 1)
    assert not np.isnan(got["mean"][others]).any()


def test_bad_labels_are_counted():
    labels, nz = zc.labels("grid8", 33, 65)
    over = labels.astype(np.int32)
    over[5, 5] = over[20, 40] = over[32, 64] = nz + 1
    with pytest.raises(ValueError, match=rf"zonal_statistics: 3 pixels have a label outside 0 \.\. {nz}$"):
        lars.zonal_statistics(plane(33, 65), over, "NDVI", n_zones=nz)
    with pytest.raises(ValueError, match=rf"process_image_zones: 3 pixels have a label outside 0 \.\. {nz}$"):
        lars.process_image_zones(picture(33, 65), over.astype(np.uint16), n_zones=nz)
    under = labels.astype(np.int32)
    under[7, 7] = -1
    with pytest.raises(ValueError, match="zonal_statistics: 1 pixels have a negative label"):
        lars.zonal_statistics(plane(33, 65), under, "NDVI", n_zones=nz)
    # the device's own count of a negative int32 label: through the C entry point, which Python's check stands in front of
    import ctypes as C
    records, medians, bad = np.zeros(nz, dtype=_ffi.STATS_DTYPE), np.zeros((nz, 2), dtype=np.float32), C.c_int64(-1)
    with pytest.raises(_ffi.LarsError, match=rf"2 labels outside 0 \.\. {nz}"):
        under[8, 8] = nz + 7
        _ffi.call("lars_h_zonal_stats_f32", _ffi.ptr(plane(33, 65)), _ffi.ptr(under), 4, None, 33, 65, nz, np.float32(0.2), 0,
                  _ffi.ptr(records), _ffi.ptr(medians), C.byref(bad))
    assert bad.value == 2
    check_plane(plane(33, 65), labels, nz)                    # and the next call is not affected


@pytest.mark.parametrize("shape, layout", [((255, 257), "one_zone"), ((255, 257), "grid8"), ((512, 512), "stripes65"), ((512, 512), "random40")], ids=id_of)
def test_both_routes_for_large_zones(shape, layout):
    """With the knob at 64 every zone of more than 64 values takes the array kernels, with the default none of these does (one
    zone everywhere apart): the records must be the same, the mean within its tolerance."""
    h, w = shape
    labels, nz = (zc.random_labels(h, w, 40), 40) if layout == "random40" else zc.labels(layout, h, w)
    before = _ffi.get_tuning("zone_split_pixels")
    base, want = check_plane(plane(h, w), labels, nz)
    for split in (SPLIT_FLOOR, 2 ** 30):
        with _ffi.tuning(zone_split_pixels=split):
            got = lars.zonal_statistics(plane(h, w), labels.astype(np.int32), "NDVI", n_zones=nz, want_hist=True)
        zm.check_zone_figures(got, want, "NDVI")
        for key in ("pixels", "median", "min", "max", "coverage", "hist"):
            assert np.array_equal(got[key], base[key], equal_nan=True), (split, key)
    assert _ffi.get_tuning("zone_split_pixels") == before


# ---------------------------------------------------------------------------
# pictures
# ---------------------------------------------------------------------------
def check_picture(img, labels, nz, valid_bool, call_kwargs, indices=ALL, white_balance=True, dtype=np.uint16):
    want = zm.zones_model(img, labels, valid_bool, indices=indices, white_balance=white_balance, n_zones=nz)
    res = lars.process_image_zones(img, labels.astype(dtype), n_zones=nz, indices=indices, white_balance=white_balance, want_hist=True,
                                   want_rgba=True, **call_kwargs)
    mm.check_result(res, want, indices)
    masked = lars.process_image_masked(img, indices=indices, white_balance=white_balance, want_hist=True, want_rgba=True, **call_kwargs)
    assert res["valid_pixels"] == masked.get("valid_pixels", labels.size)      # without a mask that call is process_image's: every pixel
    assert (res["corrected"] is None and masked["corrected"] is None) or np.array_equal(res["corrected"], masked["corrected"])
    for t in indices:
        a, b = res["indices"][t], masked["indices"][t]
        assert set(a) == set(b)
        assert np.array_equal(a["index"].view(np.uint32), b["index"].view(np.uint32)) and np.array_equal(a["rgba"], b["rgba"])
        assert np.array_equal(a["hist"], b["hist"])
        assert {k: v for k, v in a["stats"].items() if not k.startswith("Mean")} == {k: v for k, v in b["stats"].items() if not k.startswith("Mean")}
        part = {"zone": res["zones"]["zone"], "pixels": res["zones"]["pixels"], **res["zones"][t]}
        zm.check_zone_figures(part, want["zones"][t], t)
    assert set(res["zones"]) == {"zone", "pixels", *indices}
    return res


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("shape", [(7, 9), (33, 65), (255, 257)], ids=id_of)
def test_pictures_of_both_sample_types(shape, dtype):
    h, w = shape
    labels, nz = zc.labels("gaps" if h < 8 else "grid8", h, w)
    check_picture(picture(h, w, 3, dtype), labels, nz, np.ones((h, w), dtype=bool), {})


@pytest.mark.parametrize("rule", ["valid", "nodata", "alpha", "all"])
def test_pictures_under_a_mask(rule):
    h, w = 33, 65
    labels, nz = zc.labels("grid8", h, w)
    img = picture(h, w, 4).copy()
    img[:4, :, :3] = 9
    img[:, 60:, 3] = 0
    img[:, :60, 3] |= 1
    user = zc.valid_mask(h, w)
    kwargs = {"valid": dict(valid=user), "nodata": dict(nodata=9), "alpha": dict(valid="alpha"), "all": dict(valid=user, nodata=9)}[rule]
    valid_bool = mm.valid_rule(img, user if rule in ("valid", "all") else None, alpha=rule == "alpha", nodata=kwargs.get("nodata"))
    res = check_picture(img, labels, nz, valid_bool, kwargs)
    assert res["zones"]["pixels"].sum() == np.count_nonzero(valid_bool & (labels > 0))


@pytest.mark.parametrize("indices", [["NDWI"], ["NDVI", "NDWI"], ALL], ids=lambda v: "+".join(v))
@pytest.mark.parametrize("white_balance", [True, False])
def test_index_subsets_and_raw_samples(indices, white_balance):
    labels, nz = zc.labels("stripes64", 33, 65)
    check_picture(picture(33, 65), labels, nz, np.ones((33, 65), dtype=bool), {}, indices=indices, white_balance=white_balance, dtype=np.uint8)


def test_the_white_balance_is_the_pictures_not_the_plots():
    img, labels, nz = zc.plots_picture()
    res = lars.process_image_zones(img, labels, indices=["NDVI"])
    own = lars.process_image_masked(img, valid=labels == 5, indices=["NDVI"])["indices"]["NDVI"]["stats"]["Median NDVI"]
    whole = lars.process_image(img, indices=["NDVI"])["indices"]["NDVI"]["index"]
    assert res["zones"]["NDVI"]["median"][4] == float(np.median(whole[labels == 5])) != own


def test_two_runs_agree_in_everything_but_the_mean():
    labels = zc.random_labels(512, 512, 2000)
    img = picture(512, 512)
    a = lars.process_image_zones(img, labels, want_hist=True, want_arrays=False)
    b = lars.process_image_zones(img, labels, want_hist=True, want_arrays=False)
    assert np.array_equal(a["zones"]["pixels"], b["zones"]["pixels"])
    for t in ALL:
        for key in ("median", "min", "max", "coverage", "hist"):
            assert np.array_equal(a["zones"][t][key], b["zones"][t][key], equal_nan=True), (t, key)
        assert np.allclose(a["zones"][t]["mean"], b["zones"][t]["mean"], rtol=1e-12, atol=1e-15, equal_nan=True)


def test_driver_writes_the_rows(tmp_path):
    from PIL import Image
    img, labels, nz = zc.plots_picture()
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(img).save(src / "field.png")
    Image.fromarray(labels.astype(np.uint16)).save(tmp_path / "plots.png")
    res = driver.batch_process(src, tmp_path / "out", process_ndvi=True, process_ndwi=True, workers=1, verbose=False, zones=tmp_path / "plots.png")
    assert sorted(res["field.png"]) == ["NDVI", "NDWI"]
    assert res["field.png"] == driver.batch_process(src, tmp_path / "plain", process_ndvi=True, process_ndwi=True, workers=1, verbose=False)["field.png"]
    assert not list((tmp_path / "plain").glob("*.csv"))
    with open(tmp_path / "out" / "field_zones.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    direct = lars.process_image_zones(img, labels, indices=["NDVI", "NDWI"], want_arrays=False)
    want = [(t, r) for t in ("NDVI", "NDWI") for r in lars.zonal_rows(direct, t)]
    assert len(rows) == len(want) == 2 * nz
    for row, (t, w) in zip(rows, want):
        assert row["Index"] == t and int(row["Zone"]) == w["Zone"] and int(row["Pixels"]) == w["Pixels"] > 0
        figures = [v for k, v in w.items() if k not in ("Zone", "Pixels")]
        for name, value in zip(("Median", "Min", "Max", "Coverage (%)"), figures[1:]):
            assert float(row[name]) == value, (t, w["Zone"], name)
        assert abs(float(row["Mean"]) - figures[0]) <= 1e-12
