"""Zone margins without a device (DESIGN.md "Zone margins"): the model the GPU tests compare with is checked against itself (brute
force over all pixel pairs against scipy's exact distance transform), the host's rule margin -> margin2, every refusal of
``shrink_zones`` and of ``Shrunk`` before any library call, and what crosses to the library with and without a margin."""
import ctypes as C
import math

import numpy as np
import pytest

import lars_image_processing_amd as lars
import zone_margin_model as zm
from lars_image_processing_amd import _ffi, driver, zones


def test_brute_force_agrees_with_scipy_on_200_fuzzed_rasters():
    """Sizes 1 .. 23 on each side, labels 0 .. 3, every third raster blocky: D2 itself, not one threshold."""
    rng = np.random.default_rng(20261021)
    for k in range(200):
        h, w = (int(v) for v in rng.integers(1, 24, 2))
        lab = zm.fuzz_labels(rng, h, w, blocky=k % 3 == 0)
        a, b = zm.d2_brute(lab), zm.d2_scipy(lab)
        assert a.tobytes() == b.tobytes(), (k, h, w)


def test_a_zone_that_fills_the_raster_is_infinitely_deep():
    """... where scipy alone would answer with a finite distance that means nothing."""
    from scipy.ndimage import distance_transform_edt
    full = np.full((3, 3), 2, dtype=np.uint8)
    assert np.isfinite(distance_transform_edt(full == 2)).all()
    assert (zm.d2_scipy(full) == zm.INF).all() and (zm.d2_brute(full) == zm.INF).all()
    assert zm.shrink(full, 254 * 254).tobytes() == full.tobytes()


def test_margin2_is_the_largest_n_whose_root_is_within_the_margin():
    """sqrt(n) for every n of 0 .. 254^2 gives n, the float64 just below it n - 1, and 254.0 the cap."""
    for n in range(0, 254 * 254 + 1):
        m = math.sqrt(n)
        assert zones._margin2(m, "t") == n == zm.margin2(m), n
        if n:
            below = math.nextafter(m, 0.0)
            assert zones._margin2(below, "t") == n - 1 == zm.margin2(below), n
    assert zones._margin2(254.0, "t") == 64516 and zones._margin2(254, "t") == 64516
    assert zones._margin2(math.sqrt(3), "t") == 3 and zones._margin2(0.999, "t") == 0 and zones._margin2(np.float32(2.5), "t") == 6
    assert zones._margin2(np.int64(7), "t") == 49


# ---------------------------------------------------------------------------
# refusals: every one of them before any library call
# ---------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def refuse(name, *args):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")
    monkeypatch.setattr(_ffi, "call", refuse)


LAB = np.array([[0, 1, 1, 0], [2, 2, 1, 0], [2, 2, 0, 0]], dtype=np.uint8)
PLANE = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
IMG = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
SQUARE = [(0.0, 0.0), (3.0, 0.0), (3.0, 3.0), (0.0, 3.0)]
BAD_MARGINS = [
    (True, TypeError, "margin must be a number of pixels"),
    (np.bool_(False), TypeError, "margin must be a number of pixels"),
    ("2", TypeError, "margin must be a number of pixels"),
    ([2], TypeError, "margin must be a number of pixels"),
    (2 + 0j, TypeError, "margin must be a number of pixels"),
    (float("nan"), ValueError, "margin must be finite"),
    (float("inf"), ValueError, "margin must be finite"),
    (-0.5, ValueError, "margin must be 0 to 254 pixels"),
    (254.5, ValueError, "margin must be 0 to 254 pixels"),
    (math.nextafter(254.0, 255.0), ValueError, "margin must be 0 to 254 pixels"),
    (1000, ValueError, "margin must be 0 to 254 pixels"),
]


@pytest.mark.parametrize("margin, error, words", BAD_MARGINS)
def test_a_bad_margin_is_refused_before_any_launch(no_launch, margin, error, words):
    for who, call in (("shrink_zones", lambda: lars.shrink_zones(LAB, margin)),
                      ("shrink_zones", lambda: lars.shrink_zones([SQUARE], margin, shape=(3, 4))),
                      ("Shrunk", lambda: lars.zonal_statistics(PLANE, lars.Shrunk(LAB, margin), "NDVI")),
                      ("Shrunk", lambda: lars.zonal_statistics(PLANE, lars.Shrunk([SQUARE], margin), "NDVI")),
                      ("Shrunk", lambda: lars.zonal_statistics(PLANE, lars.Shrunk(lars.Regions(mask=LAB > 0), margin), "NDVI")),
                      ("Shrunk", lambda: lars.process_image_zones(IMG, lars.Shrunk(LAB, margin)))):
        with pytest.raises(error, match=words) as e:
            call()
        assert str(e.value).startswith(who + ": ")


def test_shrink_zones_needs_a_margin(no_launch):
    with pytest.raises(TypeError, match="shrink_zones: margin must be a number of pixels"):
        lars.shrink_zones(LAB, None)


def test_outlines_and_a_margin_are_refused_together(no_launch):
    outlined = lars.Regions(mask=LAB > 0, want_outlines=True)
    for margin in (1, 0.5):
        with pytest.raises(ValueError, match=r"Shrunk: Regions\(want_outlines=True\) cannot be combined with a margin"):
            lars.zonal_statistics(PLANE, lars.Shrunk(outlined, margin), "NDVI")
    with pytest.raises(TypeError, match="Shrunk: these zones are shrunk already"):
        lars.Shrunk(lars.Shrunk(LAB, 1), 1)
    with pytest.raises(TypeError, match="shrink_zones: zones must be a label raster or polygons, got Shrunk"):
        lars.shrink_zones(lars.Shrunk(LAB, 1), 1)


@pytest.mark.parametrize("call, error, words", [
    (lambda: lars.shrink_zones(LAB, 1, shape=(3, 4)), ValueError, "shape and transform belong to polygons"),
    (lambda: lars.shrink_zones(LAB, 1, transform=(0, 1, 0, 0, 0, 1)), ValueError, "shape and transform belong to polygons"),
    (lambda: lars.shrink_zones([SQUARE], 1), ValueError, "shape is required with polygons"),
    (lambda: lars.shrink_zones([SQUARE], 1, shape=(0, 4)), ValueError, "shape must be"),
    (lambda: lars.shrink_zones([SQUARE], 1, shape=(3, 4), n_zones=1), ValueError, "n_zones cannot be given with polygons"),
    (lambda: lars.shrink_zones([SQUARE], 1, shape=(3, 4), transform=(0, 1, 0, 0, 0, 1), n_zones=1), ValueError, "n_zones cannot be given with polygons"),
    (lambda: lars.shrink_zones([SQUARE[:2]], 1, shape=(3, 4)), ValueError, "polygon 0 ring 0 has 2 vertices"),
    (lambda: lars.shrink_zones(lars.Regions(mask=LAB > 0), 1), TypeError, "a label raster or polygons, got Regions"),
    (lambda: lars.shrink_zones(LAB.astype(np.float32), 1), TypeError, "zones must be an integer array"),
    (lambda: lars.shrink_zones(LAB[0], 1), ValueError, r"zones must be an \[H, W\] array"),
    (lambda: lars.shrink_zones(np.zeros((0, 4), dtype=np.uint8), 1), ValueError, "zones is empty"),
    (lambda: lars.shrink_zones(np.zeros((3, 4), dtype=np.uint8), 1), ValueError, "the largest label is 0"),
    (lambda: lars.shrink_zones(LAB.astype(np.int16) - 1, 1), ValueError, "negative label"),
    (lambda: lars.shrink_zones(LAB.astype(np.int64), 1, n_zones=1), ValueError, "label outside 0 .. 1"),
    (lambda: lars.shrink_zones(LAB, 1, n_zones=0), ValueError, "n_zones must be 1 to 65535"),
    (lambda: lars.shrink_zones(LAB, 1, n_zones=2.0), TypeError, "n_zones must be an int"),
])
def test_shrink_zones_refuses_before_any_launch(no_launch, call, error, words):
    with pytest.raises(error, match=words) as e:
        call()
    assert "shrink_zones" in str(e.value)


def test_shrink_zones_refuses_a_transform_without_an_inverse(no_launch):
    with pytest.raises(ValueError, match="to_pixel: the transform .* is singular"):
        lars.shrink_zones([SQUARE], 1, shape=(3, 4), transform=(0, 0, 0, 0, 0, 0))


def test_the_driver_refuses_a_margin_without_zones(no_launch, tmp_path):
    with pytest.raises(ValueError, match="zone_margin shrinks the zones of the picture"):
        driver.process_image(tmp_path / "a.png", tmp_path, indices=["NDVI"], zone_margin=2)
    with pytest.raises(ValueError, match="zone_margin and regions_geojson do not go together"):
        driver.batch_process(tmp_path, tmp_path, regions=("NDVI", "above", 0.2, 1), regions_geojson=True, zone_margin=2)
    for argv in (["in", "out", "--zone-margin", "2"], ["in", "out", "--zones", "z.png", "--zone-margin", "255"],
                 ["in", "out", "--zones", "z.png", "--zone-margin", "nan"],
                 ["in", "out", "--regions", "NDVI:above:0.2", "--regions-geojson", "--zone-margin", "2"]):
        with pytest.raises(SystemExit):
            driver.main(argv)


# ---------------------------------------------------------------------------
# what crosses to the library
# ---------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    calls = []

    def record(name, *args):
        calls.append((name, args))
        for arg in args:                                           # the counts a call leaves: no bad label, no region
            if isinstance(getattr(arg, "_obj", None), C.c_int64):
                arg._obj.value = 0
        if name.startswith("lars_h_process_image"):
            stats = args[10]._obj
            for k in range(3):
                stats[k].count = 1
            if name != "lars_h_process_image":
                args[18]._obj.value = 5
        return 0
    monkeypatch.setattr(_ffi, "call", record)
    return calls


def three_kinds():
    return (("", LAB), ("_polygons", [SQUARE]), ("_regions", lars.Regions(mask=LAB > 0)))


def test_no_margin_and_margin_0_bind_the_entry_points_they_always_did(recorded):
    for kind, z in three_kinds():
        want = None
        for zones in (z, lars.Shrunk(z, None), lars.Shrunk(z, 0), lars.Shrunk(z, 0.0)):
            recorded.clear()
            lars.zonal_statistics(PLANE, zones, "NDVI")
            lars.process_image_zones(IMG, zones, indices=["NDVI"])
            (n1, a1), (n2, a2) = recorded
            assert n1 == f"lars_h_zonal_stats{kind}_f32"
            assert n2 == ("lars_h_process_image_regions" if kind == "_regions" else f"lars_h_process_image_zones{kind}")
            want = want or (len(a1), len(a2))
            assert (len(a1), len(a2)) == want
    recorded.clear()
    outlined = lars.Regions(mask=LAB > 0, want_outlines=True)
    lars.zonal_statistics(PLANE, lars.Shrunk(outlined, 0), "NDVI")
    assert recorded[0][0] == "lars_h_zonal_stats_regions_outlines_f32"


def test_a_margin_binds_the_margin_entry_points_with_margin2_last(recorded):
    for kind, z in three_kinds():
        recorded.clear()
        lars.zonal_statistics(PLANE, z, "NDVI")
        lars.process_image_zones(IMG, z, indices=["NDVI"])
        lars.zonal_statistics(PLANE, lars.Shrunk(z, math.sqrt(2)), "NDVI")
        lars.process_image_zones(IMG, lars.Shrunk(z, 0.5), indices=["NDVI"])
        (_, b1), (_, b2), (n1, a1), (n2, a2) = recorded
        assert n1 == f"lars_h_zonal_stats{kind}_margin_f32" and len(a1) == len(b1) + 1 and a1[-1] == 2
        assert n2 == ("lars_h_process_image_regions_margin" if kind == "_regions" else f"lars_h_process_image_zones{kind}_margin")
        assert len(a2) == len(b2) + 1 and a2[-1] == 0
        assert _ffi.SIGNATURES[n1][1][:-1] == _ffi.SIGNATURES[n1.replace("_margin", "")][1]
        assert _ffi.SIGNATURES[n2][1][:-1] == _ffi.SIGNATURES[n2.replace("_margin", "")][1]


def test_shrink_zones_binds_one_call_and_keeps_the_dtype(recorded):
    for dtype, width in ((np.uint8, 1), (np.uint16, 2), (np.int32, 4), (np.int64, 4), (np.int8, 4), (np.uint32, 4)):
        recorded.clear()
        out = lars.shrink_zones(LAB.astype(dtype), 3)
        (name, args), = recorded
        assert name == "lars_h_shrink_zones" and args[1:6] == (width, 3, 4, 2, 9)
        assert out.dtype == dtype and out.shape == LAB.shape
    recorded.clear()
    out = lars.shrink_zones([SQUARE, SQUARE], 1.5, shape=(3, 4))
    (name, args), = recorded
    assert name == "lars_h_rasterize_zones_margin" and args[5:9] == (2, 3, 4, 1) and args[-1] == 2
    assert out.dtype == np.uint8 and out.shape == (3, 4)


def test_the_driver_hands_its_margin_to_the_zones_call(recorded, tmp_path):
    from PIL import Image
    Image.fromarray(IMG).save(tmp_path / "a.png")
    Image.fromarray(LAB.astype(np.uint16)).save(tmp_path / "z.png")
    driver.process_image(tmp_path / "a.png", tmp_path / "out", indices=["NDVI"], zones=tmp_path / "z.png", zone_margin=1.5)
    name, args = recorded[0]
    assert name == "lars_h_process_image_zones_margin" and args[-1] == 2
    header = (tmp_path / "out" / "a_zones.csv").read_text().splitlines()[0]
    recorded.clear()
    driver.process_image(tmp_path / "a.png", tmp_path / "out2", indices=["NDVI"], zones=tmp_path / "z.png")
    assert recorded[0][0] == "lars_h_process_image_zones" and (tmp_path / "out2" / "a_zones.csv").read_text().splitlines()[0] == header
