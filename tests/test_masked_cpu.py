"""Nodata-aware processing without a GPU: the NumPy model (masked_model.py) against the oracle and against np.percentile /
np.ma computed directly, the argument checks of process_image_masked / valid_mask / the driver (all before any launch), and the
default call, which must bind what it bound before: ``api.process_image`` keeps its recorded signature
(tests/golden/codec_surface.json), the mask arguments are ``process_image_masked``'s."""
import warnings

import numpy as np
import pytest

import masked_cases as mc
import masked_model as mm
import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api, driver
from oracle import index_oracle as orc


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("white_balance", [True, False])
def test_model_with_every_pixel_valid_is_the_oracle(dtype, white_balance):
    img = mc.image(37, 53, 4, dtype)
    got = mm.masked_model(img, np.ones((37, 53), dtype=bool), white_balance=white_balance)
    src = orc.wb_app(img) if white_balance else img
    if white_balance:
        assert np.array_equal(got["corrected"], src)
    assert got["valid_pixels"] == 37 * 53
    for t in mm.INDEX_NAMES:
        plane = orc.index_app(src, t)
        assert np.array_equal(got["indices"][t]["index"].view(np.uint32), plane.view(np.uint32))
        assert got["indices"][t]["stats"] == orc.stats_app(plane, t)
        assert np.array_equal(got["indices"][t]["hist"], orc.hist50(plane))
        assert np.array_equal(got["indices"][t]["rgba"], orc.colormap_closed_form(plane, api.colormap_lut(orc.colormap_name(t))))


def test_model_on_a_framed_picture_is_numpy_ma():
    img, valid = mc.framed_picture()
    got = mm.masked_model(img, valid)
    f = img.astype(np.float32)
    corrected = np.zeros_like(img)
    for band in range(3):
        lo, hi = np.percentile(f[:, :, band][valid], (2, 98))                     # the valid samples only
        corrected[:, :, band][valid] = np.clip((f[:, :, band][valid] - lo) / (hi - lo) * 255, 0, 255).astype(np.float32).astype(np.uint8)
    assert np.array_equal(got["corrected"], corrected)
    assert not got["corrected"][~valid].any()
    nir, red = corrected[:, :, 2].astype(np.float32), corrected[:, :, 0].astype(np.float32)
    ndvi = np.ma.masked_array(np.clip((nir - red) / (nir + red + 1e-10), -1, 1), mask=~valid)
    plane = got["indices"]["NDVI"]["index"]
    assert np.array_equal(plane[valid], ndvi.compressed())
    assert np.all(plane.view(np.uint32)[~valid] == 0x7FC00000)
    st = got["indices"]["NDVI"]["stats"]
    assert st["Median NDVI"] == float(np.ma.median(ndvi))
    assert st["Min NDVI"] == float(ndvi.min()) and st["Max NDVI"] == float(ndvi.max())
    assert st["Vegetation Coverage (%)"] == float((ndvi > 0.2).sum() / valid.sum() * 100)     # relative to |V|
    assert abs(st["Mean NDVI"] - float(ndvi.mean())) < 1e-6
    assert got["indices"]["NDVI"]["hist"].sum() == valid.sum()
    assert not got["indices"]["NDVI"]["rgba"][~valid].any()


def test_framed_picture_tells_a_masked_histogram_from_an_unmasked_one():
    """The picture test_gpu_masked.py uses to catch a kernel that ignores the mask in its histograms."""
    img, valid = mc.framed_picture()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        unmasked = orc.wb_app(img)
    masked = mm.masked_model(img, valid)["corrected"]
    assert not np.array_equal(unmasked[valid], masked[valid])
    for band in range(3):
        assert np.percentile(img[:, :, band], 2) == 0 < np.percentile(img[:, :, band][valid], 2)


def test_valid_rule():
    img = mc.image(5, 7, 4)
    img[0, 0, :3] = 0
    img[0, 1, :2] = 0                                   # two channels only: stays valid
    img[1, 1, 3] = 0
    user = np.ones((5, 7), dtype=np.int32)
    user[4, 6] = 0
    v = mm.valid_rule(img, user, alpha=True, nodata=0)
    want = np.ones((5, 7), dtype=bool)
    want[0, 0] = want[1, 1] = want[4, 6] = False
    assert np.array_equal(v, want)


def test_no_valid_pixel_in_the_model():
    with pytest.raises(ValueError, match="no valid pixel"):
        mm.masked_model(mc.image(3, 5, 3), np.zeros((3, 5), dtype=bool))


# ---------------------------------------------------------------------------
# argument checks: every one of them before any launch
# ---------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def refuse(name, *args):
        raise AssertionError(f"{name} was called: the arguments should have been refused first")
    monkeypatch.setattr(_ffi, "call", refuse)


IMG3 = mc.image(6, 9, 3)
IMG4 = mc.image(6, 9, 4)


@pytest.mark.parametrize("kwargs, error", [
    (dict(valid=np.ones((9, 6), dtype=bool)), ValueError),              # wrong shape
    (dict(valid=np.ones((6, 9, 1), dtype=bool)), ValueError),
    (dict(valid=np.ones(54, dtype=np.uint8)), ValueError),
    (dict(valid=np.ones((6, 9), dtype=np.float32)), TypeError),         # wrong type
    (dict(valid=np.full((6, 9), "x")), TypeError),
    (dict(valid="beta"), TypeError),
    (dict(valid="alpha"), ValueError),                                  # three channels
    (dict(nodata=256), ValueError),                                     # outside uint8
    (dict(nodata=-1), ValueError),
    (dict(nodata=0.5), TypeError),
    (dict(nodata=True), TypeError),
    (dict(nodata=0, want_entries=True), ValueError),
    (dict(valid=np.ones((6, 9), dtype=bool), want_png="palette"), ValueError),
])
def test_process_image_refuses_before_any_launch(no_launch, kwargs, error):
    with pytest.raises(error):
        lars.process_image_masked(IMG3, **kwargs)


def test_palette_refusal_says_why(no_launch):
    for kwargs in (dict(want_entries=True), dict(want_png="palette")):
        with pytest.raises(ValueError, match="palette has no free entry"):
            lars.process_image_masked(IMG4, valid="alpha", **kwargs)


def test_nodata_range_follows_the_sample_type(no_launch):
    with pytest.raises(ValueError, match="outside the range"):
        lars.process_image_masked(IMG3.astype(np.uint16), nodata=65536)
    with pytest.raises(ValueError, match="outside the range"):
        lars.valid_mask(IMG3, nodata=300)


@pytest.mark.parametrize("kwargs, error", [
    (dict(alpha=True), ValueError),
    (dict(nodata=-3), ValueError),
    (dict(nodata="0"), TypeError),
])
def test_valid_mask_refuses_before_any_launch(no_launch, kwargs, error):
    with pytest.raises(error):
        lars.valid_mask(IMG3, **kwargs)
    with pytest.raises(TypeError):
        lars.valid_mask(IMG3.astype(np.float32))


def test_driver_refuses_png8_with_a_mask(no_launch, tmp_path):
    for kwargs in (dict(nodata=0), dict(alpha_mask=True)):
        with pytest.raises(ValueError, match="palette has no free entry"):
            driver.process_image(tmp_path / "a.png", tmp_path, indices=["NDVI"], lut_format="png8", **kwargs)
        with pytest.raises(ValueError, match="palette has no free entry"):
            driver.batch_process(tmp_path, tmp_path, lut_format="png8", **kwargs)


def test_driver_main_takes_the_mask_options(monkeypatch, tmp_path):
    seen = {}

    def fake(*args, **kwargs):
        seen.update(kwargs)
        return {}
    monkeypatch.setattr(driver, "batch_process", fake)
    assert driver.main([str(tmp_path), str(tmp_path), "--nodata", "0", "--alpha-mask", "--quiet"]) == 0
    assert seen["nodata"] == 0 and seen["alpha_mask"] is True
    assert driver.main([str(tmp_path), str(tmp_path), "--quiet"]) == 0
    assert seen["nodata"] is None and seen["alpha_mask"] is False


# ---------------------------------------------------------------------------
# the default call binds what it bound before
# ---------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """_ffi.call replaced by a recorder that fills in what the result dict divides by."""
    calls = []

    def record(name, *args):
        calls.append((name, args))
        if name.startswith("lars_h_process_image"):
            stats = args[10]._obj
            for k in range(3):
                stats[k].count = 1
            if name == "lars_h_process_image_masked":
                args[18]._obj.value = 5
        return 0
    monkeypatch.setattr(_ffi, "call", record)
    return calls


@pytest.mark.parametrize("kwargs, name, nargs", [
    (dict(want_rgba=True, want_hist=True), "lars_h_process_image", 14),
    (dict(want_entries=True), "lars_h_process_image", 14),
    (dict(want_png=True), "lars_h_process_image_png", 17),
    (dict(want_png="palette"), "lars_h_process_image_png", 17),
    (dict(want_tiff=True), "lars_h_process_image_tiff_f32", 19),
    (dict(want_tiff="deflate+predictor"), "lars_h_process_image_tiff_float32", 20),
])
def test_default_call_is_unchanged(recorded, kwargs, name, nargs):
    res = api.process_image(IMG3, **kwargs)
    again = lars.process_image_masked(IMG3, valid=None, nodata=None, **kwargs)
    assert [c[0] for c in recorded] == [name, name]
    (_, a), (_, b) = recorded
    assert len(a) == len(b) == nargs
    # image shape, sample type, white balance, index mask and histogram flag: the head every route opens with
    assert a[1:8] == b[1:8] == (6, 9, 3, _ffi.U8, 1, 7, int(bool(kwargs.get("want_hist"))))
    assert [type(x) for x in a] == [type(x) for x in b]
    assert [x for x in a if isinstance(x, int)] == [x for x in b if isinstance(x, int)]
    assert "valid_pixels" not in res and "valid_pixels" not in again
    assert set(res["indices"]["NDVI"]) == {"index", "rgba", "entry", "png", "tiff", "hist", "stats"}


def test_masked_call_binds_the_masked_entry_point(recorded):
    valid = np.ones((6, 9), dtype=np.int16)
    valid[2, 3] = 0
    res = lars.process_image_masked(IMG4, indices=["NDWI"], valid=valid, nodata=255, want_rgba=True)
    (name, a), = recorded
    assert name == "lars_h_process_image_masked" and len(a) == 25
    assert a[1:8] == (6, 9, 4, _ffi.U8, 1, 4, 0)
    assert a[15:18] == (0, 1, 255) and a[19:22] == (0, 0, 0)            # no alpha rule, nodata 255, no file
    assert res["valid_pixels"] == 5
    recorded.clear()
    lars.process_image_masked(IMG4, valid="alpha", want_tiff="deflate")
    (name, a), = recorded
    assert a[14] is None and a[15:18] == (1, 0, 0) and a[19] == 8


def test_process_image_keeps_its_signature(no_launch):
    """tests/test_codec_surface_cpu.py holds it to the recorded one; a mask goes to process_image_masked."""
    with pytest.raises(TypeError):
        api.process_image(IMG3, valid=np.ones((6, 9), dtype=bool))
    with pytest.raises(TypeError):
        api.process_image(IMG3, nodata=0)
    assert lars.process_image is api.process_image and lars.process_image_masked is not api.process_image
