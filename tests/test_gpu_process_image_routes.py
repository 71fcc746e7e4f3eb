"""The route matrix of the single-picture path (process_image, process_image_masked, process_image_zones): every index subset,
white balance on and off, every output option, every kind of mask, at pictures of a few pixels.

For each (picture, indices, white balance, mask) the plainest call -- planes and histograms, nothing else -- is the reference:
without a mask it is checked against the oracle as test_gpu_parity.test_odd_shapes_against_oracle does, with one against
masked_model.py.  Every other call of the group must then give the same ``corrected``, planes, histograms, statistics and
``valid_pixels``, and its pictures and files must decode to what the plain calls return.  Everything is compared exactly but the
mean of masked and zone calls, whose double sum follows the order the device placed the values in: that one by
masked_model.check_result's tolerance.

Thinned: nothing.  The product of want_arrays and the nine output options is run in full (entries and palettes only without a
mask, zones with and without ``want_rgba``: what the API allows)."""
import itertools
import warnings

import numpy as np
import pytest

import masked_model as mm
import lars_image_processing_amd as lars
from lars_image_processing_amd import tiffio
from oracle import index_oracle as orc
from test_gpu_parity import assert_stats_close

pytestmark = pytest.mark.gpu

NAMES = mm.INDEX_NAMES
SUBSETS = [[t for k, t in enumerate(NAMES) if bits >> k & 1] for bits in range(1, 8)]
PICTURES = {"u8_1x1x3": ((1, 1, 3), np.uint8), "u8_3x5x3": ((3, 5, 3), np.uint8), "u8_37x41x4": ((37, 41, 4), np.uint8),
            "u16_37x41x3": ((37, 41, 3), np.uint16)}
OPTIONS = {"plain": {}, "rgba": dict(want_rgba=True), "entries": dict(want_entries=True), "png": dict(want_png=True),
           "palette": dict(want_png="palette"), "tiff": dict(want_tiff=True), "tiff_predictor": dict(want_tiff="predictor"),
           "deflate": dict(want_tiff="deflate"), "deflate_predictor": dict(want_tiff="deflate+predictor")}
NO_MASK_FOR = ("entries", "palette")                  # the 256 colormap entries leave no free one for "no data"
VARIANTS = ("none", "valid", "nodata", "alpha", "zones")
N_ZONES = 3


def quarter_out(h, w, seed):
    """About a quarter of the pixels out, the first one in, and (where there is more than one) the last one out."""
    valid = np.random.default_rng(seed).random((h, w)) >= 0.25
    valid.flat[-1] = False
    valid.flat[0] = True
    return valid


def picture(name, variant):
    """-> (image, the keywords that name the mask, the boolean mask they mean or None, labels or None)"""
    (h, w, c), dtype = PICTURES[name]
    rng = np.random.default_rng(h * 1000 + w * 10 + c)
    img = rng.integers(1, np.iinfo(dtype).max + 1, (h, w, c), dtype=dtype)       # no sample is 0: nodata=0 hits only where it is put
    out = ~quarter_out(h, w, 5)
    if variant == "nodata":
        img[out, :3] = 0
    if c == 4:
        img[out, 3] = 0
    img.setflags(write=False)
    labels = None
    if variant == "zones":
        labels = rng.integers(0, N_ZONES + 1, (h, w)).astype(np.uint8)
        labels.flat[0] = 0
    kwargs = {"none": {}, "valid": dict(valid=~out), "nodata": dict(nodata=0), "alpha": dict(valid="alpha"), "zones": dict(valid=~out)}[variant]
    return img, kwargs, (None if variant == "none" else ~out), labels


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


_decoded = {}


def decoded(kind, data):
    """The array a file holds; most files of a group are the same bytes, so each is decoded once."""
    key = (kind, data)
    if key not in _decoded:
        _decoded[key] = lars.decode_png(data) if kind == "png" else tiffio.read_tiff(data)
    return _decoded[key]


def check_reference(img, ref, indices, white_balance, model):
    """The plainest call against the oracle, or against the model of the masked definition."""
    if model is not None:
        mm.check_result(ref, model, indices, want_rgba=False)
        return
    assert "valid_pixels" not in ref
    src = img
    if white_balance:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            src = orc.wb_app(img)
        np.testing.assert_array_equal(ref["corrected"], src)
    else:
        assert ref["corrected"] is None
    for t in indices:
        want = orc.index_app(src, t)
        np.testing.assert_array_equal(u32(ref["indices"][t]["index"]), u32(want))
        assert_stats_close(ref["indices"][t]["stats"], orc.stats_app(want, t), want)
        np.testing.assert_array_equal(ref["indices"][t]["hist"], orc.hist50(want))


def check_same(res, ref, indices, want_arrays, model, where):
    """``res`` gives what the reference call ``ref`` gave; ``model`` (masked and zone calls) carries the mean's tolerance."""
    assert res.get("valid_pixels") == ref.get("valid_pixels"), where
    assert list(res["indices"]) == list(indices), where
    if ref["corrected"] is None:
        assert res["corrected"] is None, where
    else:
        assert np.array_equal(res["corrected"], ref["corrected"]), where
    for t in indices:
        got, exp = res["indices"][t], ref["indices"][t]
        if want_arrays:
            assert np.array_equal(u32(got["index"]), u32(exp["index"])), (where, t)
        else:
            assert got["index"] is None, (where, t)
        assert np.array_equal(got["hist"], exp["hist"]), (where, t)
        assert list(got["stats"]) == list(exp["stats"]), (where, t)
        if model is None:
            assert got["stats"] == exp["stats"], (where, t)
            continue
        m = model["indices"][t]
        for key, val in exp["stats"].items():
            if key.startswith("Mean"):
                assert abs(got["stats"][key] - m["mean64"]) <= 1e-6 * max(abs(m["mean64"]), m["meanabs"]), (where, t, key)
            else:
                assert got["stats"][key] == val, (where, t, key)


def check_pictures_and_files(res, ref, indices, option, rgba_of, where):
    """``rgba_of[t]``: the RGBA picture of index t, from the entries call without a mask, from the model with one."""
    for t in indices:
        got, plane = res["indices"][t], ref["indices"][t]["index"]
        present = {key for key in ("rgba", "entry", "png", "tiff") if got[key] is not None}
        assert present == ({"plain": set(), "rgba": {"rgba"}, "entries": {"entry"}, "png": {"png"}, "palette": {"png"}}.get(option, {"tiff"})), (where, t)
        if option == "rgba":
            assert np.array_equal(got["rgba"], rgba_of[t]), (where, t)
        elif option == "png":
            assert np.array_equal(decoded("png", got["png"]), rgba_of[t]), (where, t)
        elif option == "palette":
            lut = lars.colormap_lut(orc.colormap_name(t))
            assert lars.png_info(got["png"])["mode"] == "P", (where, t)
            assert np.array_equal(lut[decoded("png", got["png"])], rgba_of[t]), (where, t)
        elif "tiff" in present:
            back = decoded("tiff", got["tiff"])
            assert back.dtype == np.float32 and np.array_equal(u32(back), u32(plane)), (where, t)      # NaNs included


def check_zones(res, ref, indices, labels, valid, where):
    """The zone figures are zonal_statistics' of the reference plane under the same mask."""
    assert list(res["zones"]) == ["zone", "pixels", *indices], where
    for t in indices:
        plane = ref["indices"][t]["index"]
        want = lars.zonal_statistics(plane, labels, t, valid=valid, n_zones=N_ZONES, want_hist=True)
        got = {"zone": res["zones"]["zone"], "pixels": res["zones"]["pixels"], **res["zones"][t]}
        for key in ("zone", "pixels", "median", "min", "max", "coverage", "hist"):
            assert np.array_equal(got[key], want[key], equal_nan=True), (where, t, key)
        for z in range(N_ZONES):
            values = plane[valid & (labels == z + 1)].astype(np.float64)
            if values.size == 0:
                assert np.isnan(got["mean"][z]) and np.isnan(want["mean"][z]), (where, t, z)
                continue
            tol = 1e-6 * max(abs(values.mean()), np.abs(values).mean())
            assert abs(got["mean"][z] - values.mean()) <= tol and abs(want["mean"][z] - values.mean()) <= tol, (where, t, z)


def cases():
    for name, variant in itertools.product(PICTURES, VARIANTS):
        if variant != "alpha" or PICTURES[name][0][2] == 4:
            yield name, variant


@pytest.mark.parametrize("white_balance", [True, False], ids=["wb", "raw"])
@pytest.mark.parametrize("name, variant", list(cases()))
def test_route_matrix(name, variant, white_balance):
    img, mask_kwargs, valid, labels = picture(name, variant)
    for indices in SUBSETS:
        common = dict(indices=indices, white_balance=white_balance, want_hist=True)
        call = lars.process_image if valid is None else lars.process_image_masked
        ref = call(img, want_arrays=True, **common, **mask_kwargs)
        model = None if valid is None else mm.masked_model(img, valid, indices=indices, white_balance=white_balance)
        check_reference(img, ref, indices, white_balance, model)
        if valid is None:
            entries = lars.process_image(img, want_arrays=False, want_entries=True, **common)["indices"]
            rgba_of = {t: lars.colormap_lut(orc.colormap_name(t))[entries[t]["entry"]] for t in indices}
        else:
            assert ref["valid_pixels"] == int(valid.sum())
            rgba_of = {t: model["indices"][t]["rgba"] for t in indices}
        if variant == "zones":
            for want_arrays, want_rgba in itertools.product((True, False), (True, False)):
                where = (indices, want_arrays, want_rgba)
                res = lars.process_image_zones(img, labels, n_zones=N_ZONES, want_arrays=want_arrays, want_rgba=want_rgba, **common, **mask_kwargs)
                check_same(res, ref, indices, want_arrays, model, where)
                check_pictures_and_files(res, ref, indices, "rgba" if want_rgba else "plain", rgba_of, where)
                check_zones(res, ref, indices, labels, valid, where)
            continue
        for want_arrays, (option, extra) in itertools.product((True, False), OPTIONS.items()):
            if valid is not None and option in NO_MASK_FOR:
                continue
            where = (indices, want_arrays, option)
            res = call(img, want_arrays=want_arrays, **common, **extra, **mask_kwargs)
            check_same(res, ref, indices, want_arrays, model, where)
            check_pictures_and_files(res, ref, indices, option, rgba_of, where)
            if option == "entries":
                for t in indices:
                    assert res["indices"][t]["entry"].dtype == np.uint8 and res["indices"][t]["entry"].shape == img.shape[:2]


def test_refused_combinations():
    img, kwargs, _, labels = picture("u8_37x41x4", "zones")
    for mask_kwargs in (kwargs, dict(nodata=0), dict(valid="alpha")):
        with pytest.raises(ValueError, match="the 256-entry palette has no free entry for 'no data'"):
            lars.process_image_masked(img, want_entries=True, **mask_kwargs)
        with pytest.raises(ValueError, match="the 256-entry palette has no free entry for 'no data'"):
            lars.process_image_masked(img, want_png="palette", **mask_kwargs)
    for call, mask_kwargs in ((lars.process_image, {}), (lars.process_image_masked, kwargs)):
        for png, tiff in itertools.product((True, "palette"), (True, "predictor", "deflate", "deflate+predictor")):
            with pytest.raises(ValueError, match="want_tiff or want_png, not both"):
                call(img, want_png=png, want_tiff=tiff, **mask_kwargs)
        with pytest.raises(ValueError, match="want_png replaces want_rgba / want_entries"):
            call(img, want_png=True, want_rgba=True, **mask_kwargs)
        with pytest.raises(ValueError, match="want_rgba or want_entries, not both"):
            call(img, want_rgba=True, want_entries=True, **mask_kwargs)
    with pytest.raises(TypeError):
        lars.process_image_zones(img, labels, want_entries=True)              # zones take want_rgba only
    with pytest.raises(ValueError, match="zone statistics need at least one index"):
        lars.process_image_zones(img, labels, indices=[])
