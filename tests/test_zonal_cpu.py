"""Zonal statistics without a GPU: the NumPy model (zonal_model.py) against a brute-force loop, every argument refusal of
zonal_statistics / process_image_zones / the driver (all before any library call), the knob zone_split_pixels, zonal_rows, and
the calls that name no zones, which must ask the library for what they asked before."""
import inspect
import json
import os

import numpy as np
import pytest

import masked_cases as mc
import zonal_cases as zc
import zonal_model as zm
import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api, driver, zones as zones_mod
from oracle import index_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def brute_force(plane, labels, index_type, valid, nz):
    """np.median(index[zones == z]) in a loop: Z passes, plain Python where it matters."""
    _, thr = orc.coverage_rule(index_type)
    rows = []
    for z in range(1, nz + 1):
        vals = [plane[i, j] for i in range(plane.shape[0]) for j in range(plane.shape[1])
                if labels[i, j] == z and (valid is None or valid[i, j])]
        if not vals:
            rows.append(None)
            continue
        v = np.array(vals, dtype=np.float32)
        s = np.sort(v)
        n = len(v)
        median = float(np.float32(np.float32(s[(n - 1) // 2] + s[n // 2]) / 2))
        rows.append(dict(pixels=n, median=median, min=float(s[0]), max=float(s[-1]), mean=float(np.mean(v.astype(np.float64))),
                         coverage=sum(1 for x in v if x > np.float32(thr)) / n * 100,
                         hist=np.histogram(v, bins=50, range=(-1, 1))[0]))
    return rows


@pytest.mark.parametrize("shape, layout, index_type, masked", [((7, 9), "gaps", "NDVI", False), ((12, 11), "tiny_zones", "NDWI", True),
                                                               ((9, 23), "grid8", "GNDVI", True)])
def test_model_is_the_brute_force_loop(shape, layout, index_type, masked):
    labels, nz = zc.labels(layout, *shape)
    plane = zc.plane(*shape)
    valid = zc.valid_mask(*shape) if masked else None
    got = zm.zonal_model(plane, labels, index_type, valid, nz)
    want = brute_force(plane, labels, index_type, valid, nz)
    assert len(got) == nz and any(w is None for w in want) == (layout == "gaps")
    for g, w in zip(got, want):
        if w is None:
            assert g["pixels"] == 0 and all(np.isnan(g[f]) for f in zm.FIGURES) and not g["hist"].any()
            continue
        assert g["pixels"] == w["pixels"] and np.array_equal(g["hist"], w["hist"])
        for f in ("median", "min", "max", "coverage"):
            assert g[f] == w[f], f
        assert abs(g["mean"] - w["mean"]) <= 1e-6 * max(abs(w["mean"]), g["meanabs"]) and g["mean64"] == w["mean"]


def test_model_nan_zone_and_bad_labels():
    plane = zc.plane(7, 9)
    labels, nz = zc.labels("stripes65", 7, 9)                       # 9 labels used of 65
    plane[3, 4] = np.nan
    got = zm.zonal_model(plane, labels, "NDVI", None, nz)
    hit = got[labels[3, 4] - 1]
    assert hit["pixels"] == 7 and all(np.isnan(hit[f]) for f in ("mean", "median", "min", "max"))
    assert hit["coverage"] == np.count_nonzero(plane[:, 4] > np.float32(0.2)) / 7 * 100 and hit["hist"].sum() == 6
    assert not any(np.isnan(g["mean"]) for k, g in enumerate(got[:9]) if k != labels[3, 4] - 1)
    labels[0, 0] = nz + 1
    labels[6, 8] = -1
    with pytest.raises(ValueError, match=r"2 pixels have a label outside 0 \.\. 65"):
        zm.zonal_model(plane, labels, "NDVI", None, nz)


def test_zones_model_keeps_the_pictures_white_balance():
    img, labels, nz = zc.plots_picture()
    valid = np.ones(labels.shape, dtype=bool)
    got = zm.zones_model(img, labels, valid, indices=("NDVI",))
    whole = orc.index_app(orc.wb_app(img), "NDVI")
    one_plot = labels == 5
    own = orc.index_app(orc.wb_app(img[one_plot][None, :, :]), "NDVI")[0]        # what one masked call per plot would compute
    assert got["zones"]["NDVI"][4]["median"] == float(np.median(whole[one_plot]))
    assert float(np.median(own)) != float(np.median(whole[one_plot]))


# ---------------------------------------------------------------------------
# argument checks: every one of them before any library call
# ---------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def refuse(name, *args):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")
    monkeypatch.setattr(_ffi, "call", refuse)


PLANE = zc.plane(6, 9)
ZONES = zc.labels("gaps", 6, 9)[0]
IMG3 = mc.image(6, 9, 3)


def negative(dtype):
    z = ZONES.astype(dtype)
    z[1, 1] = z[2, 2] = -4
    return z


@pytest.mark.parametrize("kwargs, error, words", [
    (dict(zones=ZONES.T), ValueError, "shape"),
    (dict(zones=ZONES.reshape(-1)), ValueError, "shape"),
    (dict(zones=ZONES[:, :, None]), ValueError, "shape"),
    (dict(zones=ZONES.astype(np.float32)), TypeError, "integer"),
    (dict(zones=ZONES != 0), TypeError, "integer"),
    (dict(zones=negative(np.int32)), ValueError, "2 pixels have a negative label"),
    (dict(zones=negative(np.int8), n_zones=6), ValueError, r"2 pixels have a negative label; the labels allowed are 0 \.\. 6"),
    (dict(zones=negative(np.int64)), ValueError, "negative"),
    (dict(zones=ZONES, n_zones=0), ValueError, "1 to 65535"),
    (dict(zones=ZONES, n_zones=65536), ValueError, "1 to 65535"),
    (dict(zones=ZONES, n_zones=2.0), TypeError, "n_zones"),
    (dict(zones=ZONES, n_zones=True), TypeError, "n_zones"),
    (dict(zones=np.zeros((6, 9), dtype=np.uint8)), ValueError, "largest label is 0"),
    (dict(zones=np.full((6, 9), 70000, dtype=np.int64)), ValueError, "largest label is 70000"),
    (dict(zones=ZONES, n_zones=4), ValueError, r"pixels have a label outside 0 \.\. 4"),          # int64: counted before the conversion
    (dict(zones=(ZONES + 2 ** 33) * (ZONES > 4), n_zones=5), ValueError, r"outside 0 \.\. 5"),    # would wrap in int32
    (dict(zones=ZONES, valid=np.ones((9, 6), dtype=bool)), ValueError, "valid has shape"),
    (dict(zones=ZONES, valid=np.ones((6, 9), dtype=np.float32)), TypeError, "valid"),
])
def test_both_calls_refuse_before_any_launch(no_launch, kwargs, error, words):
    kwargs = dict(kwargs)
    zones = kwargs.pop("zones")
    with pytest.raises(error, match=words) as e:
        lars.zonal_statistics(PLANE, zones, "NDVI", **kwargs)
    assert "zonal_statistics" in str(e.value)
    with pytest.raises(error, match=words) as e:
        lars.process_image_zones(IMG3, zones, **kwargs)
    assert "process_image_zones" in str(e.value)


@pytest.mark.parametrize("call, error, words", [
    (lambda: lars.zonal_statistics(PLANE.astype(np.float64), ZONES, "NDVI"), TypeError, "float32"),
    (lambda: lars.zonal_statistics(PLANE.reshape(-1), ZONES.reshape(-1), "NDVI"), ValueError, r"\[H, W\]"),
    (lambda: lars.zonal_statistics(PLANE, ZONES, "EVI"), ValueError, "Unknown index type: EVI"),
    (lambda: lars.zonal_statistics(PLANE, ZONES, "NDVI", valid="alpha"), TypeError, "no alpha channel"),
    (lambda: lars.process_image_zones(IMG3, ZONES, valid="alpha"), ValueError, "4 or more channels"),
    (lambda: lars.process_image_zones(IMG3, ZONES, valid="beta"), TypeError, "alpha"),
    (lambda: lars.process_image_zones(IMG3, ZONES, nodata=256), ValueError, "outside the range"),
    (lambda: lars.process_image_zones(IMG3, ZONES, nodata=0.5), TypeError, "nodata"),
    (lambda: lars.process_image_zones(IMG3, ZONES, indices=["EVI"]), ValueError, "Unknown index type: EVI"),
    (lambda: lars.process_image_zones(IMG3, ZONES, indices=[]), ValueError, "at least one index"),
    (lambda: lars.process_image_zones(IMG3.astype(np.float32), ZONES), TypeError, "unsupported sample type"),
    (lambda: lars.process_image_zones(IMG3[:, :, 0], ZONES), IndexError, "dimensional"),
])
def test_each_call_refuses_its_own_arguments(no_launch, call, error, words):
    with pytest.raises(error, match=words):
        call()


def test_files_and_entries_are_no_parameters():
    names = set(inspect.signature(lars.process_image_zones).parameters)
    assert names == {"img_array", "zones", "valid", "nodata", "n_zones", "indices", "white_balance", "want_arrays", "want_hist", "want_rgba"}
    assert list(inspect.signature(lars.zonal_statistics).parameters) == ["index_array", "zones", "index_type", "valid", "n_zones", "want_hist"]


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
            if name in ("lars_h_process_image_masked", "lars_h_process_image_zones"):
                args[18]._obj.value = 5
        return 0
    monkeypatch.setattr(_ffi, "call", record)
    return calls


@pytest.mark.parametrize("dtype, width", [(np.uint8, 1), (np.uint16, 2), (np.int32, 4), (np.int64, 4), (np.int8, 4), (np.uint32, 4), (np.uint64, 4)])
def test_labels_go_as_they_are_or_as_int32(recorded, dtype, width):
    res = lars.zonal_statistics(PLANE, ZONES.astype(dtype), "NDWI", want_hist=True)
    (name, a), = recorded
    assert name == "lars_h_zonal_stats_f32" and len(a) == 12
    assert a[2] == width and a[3] is None and a[4:7] == (6, 9, 5) and a[7] == np.float32(0.0) and a[8] == 1     # Z = the largest label
    assert set(res) == {"zone", "pixels", "mean", "median", "min", "max", "coverage", "hist"}
    assert res["hist"].shape == (5, 50) and np.isnan(res["mean"]).all() and not res["pixels"].any()             # nothing ran: all empty
    recorded.clear()
    lars.process_image_zones(IMG3, ZONES.astype(dtype), n_zones=9, indices=["GNDVI"], valid=np.ones((6, 9), dtype=bool), nodata=7)
    (name, a), = recorded
    assert name == "lars_h_process_image_zones" and len(a) == 25
    assert a[1:8] == (6, 9, 3, _ffi.U8, 1, 2, 0) and a[15:18] == (0, 1, 7) and a[20:22] == (width, 9)


def test_calls_without_zones_are_unchanged(recorded, tmp_path, monkeypatch):
    """api.process_image and process_image_masked bind what they bound; the driver without zones hands _process_image the
    arguments it always did and asks the library for the same call."""
    api.process_image(IMG3, want_rgba=True)
    lars.process_image_masked(IMG3, nodata=0)
    assert [c[0] for c in recorded] == ["lars_h_process_image", "lars_h_process_image_masked"]
    assert len(recorded[0][1]) == 14 and len(recorded[1][1]) == 25
    recorded.clear()
    from PIL import Image
    Image.fromarray(IMG3).save(tmp_path / "a.png")
    stats = driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"])
    assert [c[0] for c in recorded] == ["lars_h_process_image"] and list(stats) == ["NDVI"]
    assert not list((tmp_path / "out").glob("*_zones.csv"))
    seen = []
    monkeypatch.setattr(driver, "_process_image", lambda *a, **kw: seen.append((len(a), kw)) or {})
    driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"])
    driver.batch_process(tmp_path, tmp_path / "out", workers=1, verbose=False)
    driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / "z.png")
    driver.batch_process(tmp_path, tmp_path / "out", workers=1, verbose=False, zones="z.png", nodata=0)
    assert seen == [(12, {}), (12, {}), (12, {"zones": tmp_path / "z.png"}), (13, {"zones": "z.png"})]


def test_driver_reads_the_labels_and_refuses_another_size(recorded, tmp_path):
    from PIL import Image
    Image.fromarray(IMG3).save(tmp_path / "a.png")
    Image.fromarray(ZONES.astype(np.uint16)).save(tmp_path / "z.png")
    Image.fromarray(ZONES.astype(np.uint8).T.copy()).save(tmp_path / "t.png")
    driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI", "NDWI"], zones=tmp_path / "z.png", nodata=3)
    names = [c[0] for c in recorded]
    assert names == ["lars_h_process_image_zones", "lars_h_process_image_masked"]
    a = recorded[0][1]
    assert a[6] == 5 and a[16:18] == (1, 3) and a[20:22] == (2, 5)                        # both indices, nodata 3, uint16 labels, Z = 5
    lines = (tmp_path / "out" / "a_zones.csv").read_text().splitlines()
    assert lines[0] == ",".join(driver.ZONE_CSV_COLUMNS) and len(lines) == 1 + 2 * 5
    assert lines[1].startswith("1,NDVI,0,nan") and lines[6].startswith("1,NDWI,0,nan")
    with pytest.raises(ValueError, match=r"t\.png: the label raster has shape \(9, 6\), a\.png is \(6, 9\)"):
        driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / "t.png")


def test_driver_main_takes_zones(monkeypatch, tmp_path):
    seen = {}

    def fake(*args, **kwargs):
        seen.clear()
        seen.update(kwargs)
        return {}
    monkeypatch.setattr(driver, "batch_process", fake)
    assert driver.main([str(tmp_path), str(tmp_path), "--zones", "plots.tif", "--nodata", "0", "--quiet"]) == 0
    assert seen["zones"] == "plots.tif" and seen["nodata"] == 0
    assert driver.main([str(tmp_path), str(tmp_path), "--quiet"]) == 0
    assert "zones" not in seen


# ---------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------
def test_api_surface_is_unchanged():
    with open(os.path.join(ROOT, "tests", "golden", "codec_surface.json")) as f:
        golden = json.load(f)
    for name in ("zonal_statistics", "process_image_zones", "zonal_rows"):
        assert name not in api.__all__ and not hasattr(api, name)
        assert getattr(lars, name) is getattr(zones_mod, name)
    assert json.dumps(golden).count("zon") == 0
    assert list(inspect.signature(api.process_image).parameters) == ["img_array", "indices", "white_balance", "want_arrays", "want_hist", "want_rgba",
                                                                     "want_entries", "want_png", "want_tiff"]
    assert list(inspect.signature(lars.process_image_masked).parameters)[:3] == ["img_array", "valid", "nodata"]


def test_zonal_rows_keys():
    stats = {"zone": np.array([1, 2]), "pixels": np.array([3, 0]), "mean": np.array([0.5, np.nan]), "median": np.array([0.25, np.nan]),
             "min": np.array([-1.0, np.nan]), "max": np.array([1.0, np.nan]), "coverage": np.array([100 / 3, np.nan])}
    rows = lars.zonal_rows(stats, "NDVI")
    assert [list(r) for r in rows] == [["Zone", "Pixels", "Mean NDVI", "Median NDVI", "Min NDVI", "Max NDVI", "Vegetation Coverage (%)"]] * 2
    assert rows[0] == {"Zone": 1, "Pixels": 3, "Mean NDVI": 0.5, "Median NDVI": 0.25, "Min NDVI": -1.0, "Max NDVI": 1.0,
                       "Vegetation Coverage (%)": 100 / 3}
    assert rows[1]["Pixels"] == 0 and np.isnan(rows[1]["Mean NDVI"])
    assert all(type(v) in (int, float) for r in rows for v in r.values())
    assert list(rows[0])[2:] == list(orc.stats_app(np.zeros(2, np.float32), "NDVI"))              # analyze_index's five keys, in its order
    figures = {k: v for k, v in stats.items() if k not in ("zone", "pixels")}
    result = {"zones": {"zone": stats["zone"], "pixels": stats["pixels"], "NDWI": figures}}
    water = lars.zonal_rows(result, "NDWI")
    assert list(water[0])[-1] == "Water Coverage (%)" and lars.zonal_rows(result["zones"], "NDWI")[0] == water[0]
    with pytest.raises(KeyError):
        lars.zonal_rows(result, "NDVI")
    with pytest.raises(ValueError, match="Unknown index type"):
        lars.zonal_rows(stats, "EVI")


# ---------------------------------------------------------------------------
# the knob
# ---------------------------------------------------------------------------
def test_zone_split_pixels_default_and_range():
    assert _ffi.get_tuning("zone_split_pixels") == 131072
    with _ffi.tuning(zone_split_pixels=64):
        assert _ffi.get_tuning("zone_split_pixels") == 64
        for bad in (63, 0, -1, 2 ** 30 + 1):
            with pytest.raises(_ffi.LarsError) as e:
                _ffi.set_tuning(zone_split_pixels=bad)
            assert str(e.value) == f"liblars_hip error -1: lars_set_tuning: zone_split_pixels is 64 .. 1073741824 (got {bad})"
            assert _ffi.get_tuning("zone_split_pixels") == 64
        _ffi.set_tuning(zone_split_pixels=2 ** 30)
    assert _ffi.get_tuning("zone_split_pixels") == 131072
