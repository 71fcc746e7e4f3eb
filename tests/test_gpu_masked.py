"""Nodata-aware processing on the device (csrc/masked.hip: process_image_masked(valid=..., nodata=...), valid_mask, the driver's
--nodata) against the NumPy model of the definition (masked_model.py): everything bit for bit, the mean within the
project's tolerance of 1e-6 of max(|mean|, mean|x|) against the float64 mean."""
import functools
import io

import numpy as np
import pytest

import masked_cases as mc
import masked_model as mm
import lars_image_processing_amd as lars
from lars_image_processing_amd import driver, tiffio

pytestmark = pytest.mark.gpu

ALL = list(mm.INDEX_NAMES)


@functools.lru_cache(maxsize=None)
def picture(h, w, c, dtype="uint8"):
    img = mc.image(h, w, c, np.dtype(dtype))
    img.setflags(write=False)
    return img


def run_and_check(img, valid_bool, call_kwargs, indices=ALL, white_balance=True, want_hist=True, want_rgba=True):
    want = mm.masked_model(img, valid_bool, indices=indices, white_balance=white_balance)
    res = lars.process_image_masked(img, indices=indices, white_balance=white_balance, want_hist=want_hist, want_rgba=want_rgba, **call_kwargs)
    mm.check_result(res, want, indices, want_hist=want_hist, want_rgba=want_rgba)
    return res, want


@pytest.mark.parametrize("shape, mask_name", mc.shape_mask_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_shapes_and_masks(shape, mask_name):
    h, w, c = shape
    valid = mc.mask(mask_name, h, w)
    run_and_check(picture(h, w, c), valid, dict(valid=valid))


def nodata_picture(h, w, c, dtype, nodata):
    """A picture with a frame of ``nodata`` in R, G and NIR, and pixels that hold it in one or two channels only (valid)."""
    img = picture(h, w, c, dtype).copy()
    frame = ~mc.mask("frame", h, w)
    img[frame, :3] = nodata
    img[h // 2, w // 2, 0] = nodata
    img[h // 2, w // 3, 1:3] = nodata
    return img


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("shape", [(37, 53), (257, 255)], ids=["37x53", "257x255"])
def test_valid_array_on_both_sample_types(shape, c, dtype):
    h, w = shape
    valid = mc.mask("random_50", h, w)
    # integer masks count where they are nonzero
    run_and_check(picture(h, w, c, dtype), valid, dict(valid=valid.astype(np.int32) * 7))


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("nodata", [0, 255])
@pytest.mark.parametrize("c", [3, 4])
def test_nodata(c, nodata, dtype):
    img = nodata_picture(37, 53, c, dtype, nodata)
    valid = mm.valid_rule(img, nodata=nodata)
    assert 0 < valid.sum() < valid.size and valid[37 // 2, 53 // 2]
    run_and_check(img, valid, dict(nodata=nodata))


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_alpha_and_its_combinations(dtype):
    h, w = 257, 255
    img = picture(h, w, 4, dtype).copy()
    img[:, :, 3] = np.where(mc.mask("runs_64", h, w), img[:, :, 3] | 1, 0)
    run_and_check(img, mm.valid_rule(img, alpha=True), dict(valid="alpha"))
    img[~mc.mask("frame", h, w), :3] = 0
    run_and_check(img, mm.valid_rule(img, alpha=True, nodata=0), dict(valid="alpha", nodata=0))


def test_array_and_nodata_combine_with_and():
    img = nodata_picture(37, 53, 3, "uint8", 0)
    user = mc.mask("checkerboard", 37, 53)
    valid = mm.valid_rule(img, user, nodata=0)
    assert valid.sum() < min(user.sum(), mm.valid_rule(img, nodata=0).sum())
    run_and_check(img, valid, dict(valid=user, nodata=0))
    # 8-bit masks cross as they are: any nonzero byte counts
    run_and_check(img, valid, dict(valid=user.astype(np.uint8) * 200, nodata=0))
    run_and_check(img, valid, dict(valid=-user.astype(np.int8), nodata=0))


@pytest.mark.parametrize("white_balance", [True, False])
@pytest.mark.parametrize("indices", [["NDVI"], ["GNDVI"], ["NDWI"], ALL], ids=lambda v: "+".join(v))
@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_outputs(dtype, indices, white_balance):
    h, w = 64, 67
    valid = mc.mask("frame", h, w)
    img = picture(h, w, 3, dtype)
    run_and_check(img, valid, dict(valid=valid), indices=indices, white_balance=white_balance)
    # statistics alone: no plane, no histogram, no picture
    want = mm.masked_model(img, valid, indices=indices, white_balance=white_balance)
    res = lars.process_image_masked(img, indices=indices, white_balance=white_balance, want_arrays=False, valid=valid)
    mm.check_result(res, want, indices, want_hist=False, want_rgba=False, want_arrays=False)
    for t in indices:
        assert res["indices"][t]["index"] is None and res["indices"][t]["hist"] is None and res["indices"][t]["rgba"] is None


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_constant_channel_among_the_valid_pixels(dtype):
    """p98 == p2 in one channel: whatever the table kernel gives for that histogram, the reference gives too."""
    h, w = 37, 53
    valid = mc.mask("checkerboard", h, w)
    img = picture(h, w, 3, dtype).copy()
    img[valid, 0] = 77                                   # red is constant where it counts, and only there
    run_and_check(img, valid, dict(valid=valid))
    img[valid, 2] = 0
    run_and_check(img, valid, dict(valid=valid))


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
def test_histograms_leave_the_frame_out(dtype):
    """Percentiles over the rectangle and over the valid pixels differ here (test_masked_cpu.py checks that they do)."""
    img, valid = mc.framed_picture(dtype=np.dtype(dtype))
    res, _ = run_and_check(img, valid, dict(valid=valid))
    plain = lars.process_image(img)
    assert not np.array_equal(plain["corrected"][valid], res["corrected"][valid])
    run_and_check(img, valid, dict(nodata=0))


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_valid_mask(shape):
    h, w, _ = shape
    for c, dtype in ((3, "uint8"), (4, "uint8"), (5, "uint8"), (3, "uint16"), (4, "uint16")):
        img = nodata_picture(h, w, c, dtype, 0)
        assert np.array_equal(lars.valid_mask(img), np.ones((h, w), dtype=np.uint8))
        assert np.array_equal(lars.valid_mask(img, nodata=0), mm.valid_rule(img, nodata=0).astype(np.uint8))
        if c >= 4:
            img[:, :, 3] = np.where(mc.mask("random_50", h, w), img[:, :, 3] | 1, 0)
            assert np.array_equal(lars.valid_mask(img, alpha=True), mm.valid_rule(img, alpha=True).astype(np.uint8))
            assert np.array_equal(lars.valid_mask(img, nodata=0, alpha=True), mm.valid_rule(img, alpha=True, nodata=0).astype(np.uint8))


def test_png_files_are_the_rgba_planes():
    from PIL import Image
    h, w = 257, 255
    valid = mc.mask("frame", h, w)
    img = picture(h, w, 3)
    want = mm.masked_model(img, valid)
    res = lars.process_image_masked(img, want_arrays=False, want_png=True, valid=valid)
    mm.check_result(res, want, ALL, want_hist=False, want_rgba=False, want_arrays=False)
    for t in ALL:
        back = Image.open(io.BytesIO(res["indices"][t]["png"]))
        assert back.mode == "RGBA"
        assert np.array_equal(np.asarray(back), want["indices"][t]["rgba"]), t
        assert not np.asarray(back)[~valid].any()


@pytest.mark.parametrize("mode", [True, "deflate+predictor"])
def test_tiff_files_are_the_planes_with_their_nans(mode):
    h, w = 257, 255
    valid = mc.mask("runs_64", h, w)
    img = picture(h, w, 3)
    want = mm.masked_model(img, valid)
    res = lars.process_image_masked(img, want_arrays=False, want_tiff=mode, valid=valid)
    mm.check_result(res, want, ALL, want_hist=False, want_rgba=False, want_arrays=False)
    for t in ALL:
        back = tiffio.read_tiff(res["indices"][t]["tiff"])
        assert back.dtype == np.float32
        assert np.array_equal(back.view(np.uint32), want["indices"][t]["index"].view(np.uint32)), t
        assert np.all(back.view(np.uint32)[~valid] == 0x7FC00000)


def test_no_valid_pixel():
    img = picture(37, 53, 4).copy()
    with pytest.raises(ValueError, match="process_image: no valid pixel"):
        lars.process_image_masked(img, valid=np.zeros((37, 53), dtype=bool))
    img[:, :, :3] = 9
    with pytest.raises(ValueError, match="process_image: no valid pixel"):
        lars.process_image_masked(img, nodata=9)
    img[:, :, 3] = 0
    with pytest.raises(ValueError, match="process_image: no valid pixel"):
        lars.process_image_masked(img, valid="alpha")
    assert not lars.valid_mask(img, alpha=True).any()


def test_unmasked_call_after_a_masked_one_is_what_it_was():
    """The masked job's buffers come from the same per-thread workspace: nothing of them may show in the next call."""
    def same(a, b):
        assert np.array_equal(a["corrected"], b["corrected"])
        for t in ALL:
            for key in ("index", "rgba", "hist"):
                assert np.array_equal(a["indices"][t][key], b["indices"][t][key]), (t, key)
            assert a["indices"][t]["stats"] == b["indices"][t]["stats"]
            assert a["indices"][t]["png"] == b["indices"][t]["png"]

    for c in (3, 4):
        img = picture(257, 255, c)
        valid = mc.mask("random_50", 257, 255)
        for kwargs in (dict(want_rgba=True, want_hist=True), dict(want_arrays=False), dict(want_png=True, want_hist=True)):
            before = lars.process_image(img, **kwargs)
            lars.process_image_masked(img, valid=valid, want_hist=True, want_rgba=True)
            same(before, lars.process_image(img, **kwargs))
            lars.process_image_masked(img, valid=valid, want_tiff=True)
            same(before, lars.process_image(img, **kwargs))
            assert "valid_pixels" not in before


def test_driver_with_nodata(tmp_path):
    from PIL import Image
    img = nodata_picture(64, 67, 3, "uint8", 0)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    Image.fromarray(img).save(src / "plot.png")
    stats = driver.process_image(src / "plot.png", out, process_wb=True, indices=ALL, index_tiff=True, nodata=0)
    valid = mm.valid_rule(img, nodata=0)
    want = mm.masked_model(img, valid)
    res = {"valid_pixels": want["valid_pixels"], "corrected": np.asarray(Image.open(out / "white_balanced" / "plot_wb.tif")), "indices": {}}
    for t in ALL:
        res["indices"][t] = {"stats": stats[t], "rgba": np.asarray(Image.open(out / t / f"plot_{t.lower()}.png")),
                             "index": tiffio.read_tiff(out / t / f"plot_{t.lower()}_f32.tif")}
    mm.check_result(res, want, ALL, want_hist=False)
    assert driver.main([str(src), str(tmp_path / "out2"), "--ndvi", "--nodata", "0", "--png-encoder", "device", "--workers", "1", "--quiet"]) == 0
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out2" / "NDVI" / "plot_ndvi.png")), want["indices"]["NDVI"]["rgba"])
    # the default leaves the frame in: other statistics
    assert driver.process_image(src / "plot.png", tmp_path / "out3", indices=["NDVI"])["NDVI"] != stats["NDVI"]
