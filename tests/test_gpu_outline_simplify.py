"""Simplified outlines on the device (csrc/outline_simplify.hip) through every public way to them -- region_outlines(simplify=),
Regions(want_outlines=True, simplify=) in zonal_statistics and process_image_zones, simplify_outlines -- against the model of the
definition (outline_simplify_model.py) on the model's traces: ring rows and vertices bit for bit."""
import numpy as np
import pytest

import outline_simplify_cases as oc
import outline_simplify_model as sm
import outlines_model as om
import regions_model as gm
import lars_image_processing_amd as lars
from test_gpu_regions import ROOM, SHAPES, picture

pytestmark = pytest.mark.gpu

PLAIN_KEYS = {"outlines", "ring_area2", "n_rings", "n_vertices"}


def same_simplified(part, want, n):
    """``part`` holds the model's simplified outlines ``want`` of ``n`` regions."""
    assert (part["n_rings"], part["n_vertices"], part["n_vertices_traced"]) == (want["n_rings"], want["n_vertices"], want["n_vertices_traced"]), \
        (part["n_rings"], part["n_vertices"], part["n_vertices_traced"], want["n_rings"], want["n_vertices"], want["n_vertices_traced"])
    assert part["ring_area2"].dtype == np.int64 and np.array_equal(part["ring_area2"], want["ring_area2"])
    verts, ring_starts, poly_starts = om.polygons(want, n)
    p = part["outlines"]
    assert isinstance(p, lars.Polygons) and len(p) == n
    assert p.verts.dtype == np.float64 and p.verts.flags["C_CONTIGUOUS"] and p.ring_starts.dtype == np.int32 and p.poly_starts.dtype == np.int32
    assert np.array_equal(p.ring_starts, ring_starts), (p.ring_starts[:8], ring_starts[:8])
    assert np.array_equal(p.poly_starts, poly_starts)
    bad = np.flatnonzero((p.verts != verts).any(axis=1))
    assert bad.size == 0, (len(bad), bad[:5].tolist(), p.verts[bad[:5]].tolist(), verts[bad[:5]].tolist())


def check(name, connectivity, tq):
    mask, model, traced = oc.labelled(name, connectivity)
    got = lars.region_outlines(mask, connectivity=connectivity, simplify=tq / 16)
    n = model["n_regions"]
    assert got["n_regions"] == n and np.array_equal(got["labels"], model["labels"])
    if n == 0:
        assert got["outlines"] is None and got["n_rings"] == 0 and got["n_vertices"] == 0 and got["n_vertices_traced"] == 0
        return got
    same_simplified(got, oc.simplified(name, connectivity, tq), n)
    return got


@pytest.mark.parametrize("connectivity", [4, 8])
def test_all_masks_of_three_by_three(connectivity):
    for tq in oc.GPU_TQS:
        check("all_3x3", connectivity, tq)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("chunk", range(4))
def test_fuzzed_masks(chunk, connectivity):
    for seed in range(chunk * 50, chunk * 50 + 50):
        for tq in oc.GPU_TQS:
            check("fuzz_%d" % seed, connectivity, tq)


@pytest.mark.parametrize("axis", [0, 1], ids=["heights", "widths"])
def test_every_height_and_width(axis):
    shorter = 0
    for n in range(1, 67):
        name = "size_%dx37" % n if axis == 0 else "size_37x%d" % n
        got = check(name, 4 if n % 2 else 8, 16)
        shorter += got["n_vertices"] < got["n_vertices_traced"]
    assert shorter > 40


@pytest.mark.parametrize("connectivity", [4, 8])
def test_checkerboard_every_ring_collapses_and_stays_as_traced(connectivity):
    got = check("checkerboard", connectivity, 16)
    want = oc.simplified("checkerboard", connectivity, 16)
    assert want["restored"].sum() >= want["n_rings"] - 1 and got["n_rings"] > 1900
    if connectivity == 4:
        plain = lars.region_outlines(oc.named()["checkerboard"], connectivity=4)
        assert got["n_vertices"] == got["n_vertices_traced"] == 8192 and np.array_equal(got["outlines"].verts, plain["outlines"].verts)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_comb_of_24_teeth_takes_several_batches_of_rounds(connectivity):
    want = oc.simplified("comb_24", connectivity, 16)
    assert want["rounds"] > 2 * oc.BATCH
    got = check("comb_24", connectivity, 16)
    assert got["n_vertices"] == want["n_vertices"] < got["n_vertices_traced"]
    check("comb_24", connectivity, 8)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_serpentine_one_ring_across_several_workgroups(connectivity):
    traced = oc.labelled("serpentine", connectivity)[2]
    assert traced["n_rings"] == 1 and traced["n_vertices"] >= 3 * oc.CHUNK
    for tq in (8, 16, 48):
        check("serpentine", connectivity, tq)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_several_labels_whose_rings_end_mid_wave(connectivity):
    traced = oc.labelled("blobs", connectivity)[2]
    assert (np.cumsum(traced["ring_count"] + 1)[:-1] % 64 != 0).sum() > 20 and len(set(traced["ring_label"].tolist())) > 3
    for tq in oc.GPU_TQS:
        check("blobs", connectivity, tq)


def test_no_tolerance_is_the_unsimplified_call():
    mask = oc.labelled("fuzz_31", 8)[0]
    plain = lars.region_outlines(mask)
    assert PLAIN_KEYS < set(plain) and "n_vertices_traced" not in plain
    for nothing in (None, 0, 0.01):
        got = lars.region_outlines(mask, simplify=nothing)
        assert set(got) == set(plain)
        for key in set(plain) - {"outlines"}:
            assert np.array_equal(got[key], plain[key]) and np.asarray(got[key]).dtype == np.asarray(plain[key]).dtype, key
        for key in ("verts", "ring_starts", "poly_starts"):
            assert getattr(got["outlines"], key).tobytes() == getattr(plain["outlines"], key).tobytes(), key
    assert lars.region_outlines(mask, simplify=1)["n_vertices"] < plain["n_vertices"]


def test_five_runs_give_the_same_bytes():
    mask = oc.labelled("serpentine", 8)[0] ^ oc.smooth_mask(100, 100, 5)
    runs = [lars.region_outlines(mask, connectivity=4, simplify=1.5) for _ in range(5)]
    for r in runs[1:]:
        assert r["ring_area2"].tobytes() == runs[0]["ring_area2"].tobytes() and r["n_vertices"] == runs[0]["n_vertices"]
        for key in ("verts", "ring_starts", "poly_starts"):
            assert getattr(r["outlines"], key).tobytes() == getattr(runs[0]["outlines"], key).tobytes(), key


def test_every_traced_vertex_lies_within_the_tolerance_of_its_ring():
    """What the docstrings promise in place of rasterize_zones giving the labels back, on the device's own output."""
    mask, model, traced = oc.labelled("fuzz_77", 8)
    got = lars.region_outlines(mask, simplify=2)
    assert got["n_vertices"] < got["n_vertices_traced"]
    p = got["outlines"]
    for i in range(traced["n_rings"]):
        ring = p.verts[p.ring_starts[i]:p.ring_starts[i + 1], ::-1].astype(np.int64)
        chain = [tuple(v) for v in ring.tolist()] + [tuple(ring[0].tolist())]
        s, c = traced["ring_start"][i], traced["ring_count"][i]
        for v in traced["verts"][s:s + c].tolist():
            assert any(not sm.far(*sm.measure(a, b, tuple(v)), 32) for a, b in zip(chain, chain[1:])), (i, v)


def test_simplify_outlines_is_the_keyword(tmp_path):
    for name, connectivity, tolerance in (("fuzz_55", 8, 1), ("blobs", 4, 0.5), ("comb_24", 8, 3)):
        mask = oc.labelled(name, connectivity)[0]
        plain = lars.region_outlines(mask, connectivity=connectivity)
        direct = lars.region_outlines(mask, connectivity=connectivity, simplify=tolerance)
        later = lars.simplify_outlines(plain, tolerance)
        assert set(later) == set(direct) and later["n_vertices_traced"] == plain["n_vertices"] == direct["n_vertices_traced"]
        assert later["n_vertices"] == direct["n_vertices"] and np.array_equal(later["ring_area2"], direct["ring_area2"]) and later["ring_area2"].dtype == np.int64
        for key in ("verts", "ring_starts", "poly_starts"):
            assert getattr(later["outlines"], key).tobytes() == getattr(direct["outlines"], key).tobytes(), key
        assert later["labels"] is plain["labels"] and plain["n_vertices"] == len(plain["outlines"].verts)
        same_simplified(later, oc.simplified(name, connectivity, int(tolerance * 16)), plain["n_regions"])


@pytest.mark.parametrize("shape", SHAPES)
def test_zonal_statistics_with_simplified_outlines(shape):
    _, _, masked, _ = picture(shape, "none")
    plane = masked["indices"]["NDVI"]["index"]
    plain = lars.zonal_statistics(plane, lars.Regions(above=0.2, max_regions=ROOM, want_labels=True, want_outlines=True), "NDVI")
    got = lars.zonal_statistics(plane, lars.Regions(above=0.2, max_regions=ROOM, want_labels=True, want_outlines=True, simplify=1), "NDVI")
    n = len(got["zone"])
    assert n > 3 and set(got) == set(plain) | {"n_vertices_traced"}
    for key in ("zone", "pixels", "mean", "median", "min", "max", "coverage", "labels"):
        assert np.array_equal(got[key], plain[key], equal_nan=True), key
    want = sm.simplify(om.trace(gm.label(plane > np.float32(0.2), 8)["labels"], 8), 16)
    same_simplified(got, want, n)
    assert got["n_vertices_traced"] == plain["n_vertices"] > got["n_vertices"]
    again = lars.simplify_outlines(plain, 1)
    assert again["outlines"].verts.tobytes() == got["outlines"].verts.tobytes() and again["mean"] is plain["mean"]


@pytest.mark.parametrize("shape", SHAPES)
def test_process_image_zones_with_simplified_outlines(shape):
    img, kwargs, masked, _ = picture(shape, "none")
    plain = lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, max_regions=ROOM, want_labels=True, want_outlines=True), **kwargs)
    got = lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, max_regions=ROOM, want_labels=True, want_outlines=True, simplify=1.4375),
                                   **kwargs)
    n = len(got["zones"]["zone"])
    assert n > 3 and set(got["zones"]) == set(plain["zones"]) | {"n_vertices_traced"}
    assert np.array_equal(got["zones"]["pixels"], plain["zones"]["pixels"]) and got["corrected"].tobytes() == plain["corrected"].tobytes()
    assert np.array_equal(got["zones"]["labels"], plain["zones"]["labels"])
    for t in ("NDVI", "GNDVI", "NDWI"):
        for key in ("mean", "median", "min", "max", "coverage"):
            assert np.array_equal(got["zones"][t][key], plain["zones"][t][key], equal_nan=True), (t, key)
    want = sm.simplify(om.trace(gm.label(masked["indices"]["NDVI"]["index"] > np.float32(0.2), 8)["labels"], 8), 23)
    same_simplified(got["zones"], want, n)
    again = lars.simplify_outlines(plain, 1.4375)
    assert again["zones"]["outlines"].verts.tobytes() == got["zones"]["outlines"].verts.tobytes() and again["corrected"] is plain["corrected"]


def test_room_for_the_traced_vertices_and_for_the_kept_ones():
    """max_vertices is the room of the vertices written: short for the traced ones it still serves, short for the kept ones the call
    ends with their number."""
    img, kwargs, masked, _ = picture((64, 80), "none")
    plane = masked["indices"]["NDVI"]["index"]
    traced = om.trace(gm.label(plane > np.float32(0.2), 4)["labels"], 4)
    want = sm.simplify(traced, 16)
    v, kept = traced["n_vertices"], want["n_vertices"]
    assert 16 < kept < v - 8
    got = lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, want_outlines=True, max_vertices=kept, simplify=1), "NDVI")
    assert (got["n_vertices"], got["n_vertices_traced"]) == (kept, v)
    same_simplified(got, want, len(got["zone"]))
    with pytest.raises(ValueError, match=rf"zonal_statistics: the outlines have {v} vertices, more than max_vertices = {kept}: raise min_pixels .* or max_vertices"):
        lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, want_outlines=True, max_vertices=kept), "NDVI")
    with pytest.raises(ValueError, match=rf"zonal_statistics: the outlines have {kept} vertices, more than max_vertices = {kept - 1}: raise min_pixels .* or max_vertices"):
        lars.zonal_statistics(plane, lars.Regions(above=0.2, connectivity=4, want_outlines=True, max_vertices=kept - 1, simplify=1), "NDVI")
    with pytest.raises(ValueError, match=rf"process_image_zones: the outlines have {kept} vertices, more than max_vertices = 16"):
        lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, connectivity=4, want_outlines=True, max_vertices=16, simplify=1), **kwargs)


def test_driver_writes_the_simplified_regions_geojson(tmp_path):
    import masked_cases as mc
    from PIL import Image

    from lars_image_processing_amd import driver
    img = mc.image(64, 80, 3)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(img).save(src / "field.png")
    flags = ["--ndvi", "--gndvi", "--no-ndwi", "--workers", "1", "--quiet", "--regions", "GNDVI:above:0.25:2", "--regions-geojson"]
    assert driver.main([str(src), str(tmp_path / "out"), *flags, "--regions-simplify", "1.5"]) == 0
    want = lars.process_image_zones(img, lars.Regions(index="GNDVI", above=0.25, min_pixels=2, want_outlines=True, simplify=1.5), indices=["NDVI", "GNDVI"],
                                    want_arrays=False)["zones"]
    assert want["n_vertices"] < want["n_vertices_traced"]
    back = lars.polygons_from_geojson(tmp_path / "out" / "field_regions.geojson")
    assert len(back) == len(want["zone"]) > 3
    for k in range(len(back)):
        rings = want["outlines"].rings(k)
        assert len(back[k]) == len(rings)
        for mine, theirs in zip(back[k], rings):
            assert np.array_equal(mine[:-1], theirs) and np.array_equal(mine[-1], theirs[0])
    assert driver.main([str(src), str(tmp_path / "plain"), *flags]) == 0
    plain = lars.polygons_from_geojson(tmp_path / "plain" / "field_regions.geojson")
    assert sum(len(r) for p in plain for r in p) > sum(len(r) for p in back for r in p)
    assert open(tmp_path / "plain" / "field_zones.csv").read() == open(tmp_path / "out" / "field_zones.csv").read()
