"""The three sources of labels in turn on one thread (csrc/host_zones.cpp): a label raster, polygons, regions with their labels and
outlines, rasterize_zones, label_regions, region_outlines, regions that find nothing, and the first call again -- on one 33 x 65
plane and on one 33 x 65 picture (one side beyond the labeller's 32 x 32 tile).  Every call carves the thread's one workspace anew
from its own source, so what an earlier call left there must not show: the first and the last results are the same bytes, the
regions' labels handed back as a raster and their outlines handed back as polygons give the regions' figures, and no region is zero
rows and no ring."""
import numpy as np
import pytest

import outlines_model as om
import regions_model as gm
import zonal_cases as zc
import zone_raster_cases as rc
import zone_raster_model as zrm
import lars_image_processing_amd as lars
from test_gpu_zone_raster import same_figures, zone_meanabs

pytestmark = pytest.mark.gpu

SHAPE = (33, 65)
NOTHING = 2.0                                                            # no index value lies above it: no region
INDEX_NAMES = ("NDVI", "GNDVI", "NDWI")


def same_bytes(a, b):
    """Two zone parts: every array but the mean bit for bit (the mean's double sum follows the order the device placed the values in)."""
    assert set(a) == set(b)
    for key in a:
        if key != "mean":
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() and np.asarray(a[key]).dtype == np.asarray(b[key]).dtype, key


def check_empty(part, with_outlines):
    assert len(part["zone"]) == 0 and len(part["pixels"]) == 0 and all(len(part["regions"][k]) == 0 for k in ("area", "bbox", "centroid"))
    assert ("outlines" in part) == with_outlines
    if with_outlines:
        assert part["outlines"] is None and (part["n_rings"], part["n_vertices"], len(part["ring_area2"])) == (0, 0, 0)


def in_turn(call, part, plane_of, index):
    """``call(zones, **kw)`` is zonal_statistics or process_image_zones on the one raster, ``part(result)`` the zone part of its result
    with the figures of one index, ``plane_of(result)`` the plane those figures are of, ``index`` what names that plane to
    ``Regions`` (None: the call has one plane only)."""
    labels, nz = zc.labels("grid8", *SHAPE)
    labels = labels.astype(np.uint8)
    polygons = rc.jittered_grid(3, 4, SHAPE, seed=5)
    first = call(labels, n_zones=nz)
    plane = plane_of(first)

    by_polygons = call(lars.Polygons(polygons, want_labels=True))
    made = zrm.labels(polygons, SHAPE)
    assert np.array_equal(part(by_polygons)["labels"], made)
    same_figures(part(by_polygons), part(call(made, n_zones=len(polygons))), zone_meanabs(plane, made, None, len(polygons)))

    found = part(call(lars.Regions(above=0.2, index=index, want_labels=True, want_outlines=True)))
    want = gm.label(plane > np.float32(0.2), 8, 1)
    r = want["n_regions"]
    assert r >= 1 and len(found["zone"]) == r and np.array_equal(found["labels"], want["labels"]) and np.array_equal(found["regions"]["area"], want["area"])
    traced = om.trace(want["labels"], 8)
    assert (found["n_rings"], found["n_vertices"]) == (traced["n_rings"], traced["n_vertices"]) and len(found["outlines"]) == r

    assert np.array_equal(lars.rasterize_zones(polygons, SHAPE), made)
    mask = plane > np.float32(0.2)
    labelled = lars.label_regions(mask)
    assert labelled["n_regions"] == r and np.array_equal(labelled["labels"], want["labels"])
    outlined = lars.region_outlines(mask)
    assert np.array_equal(outlined["labels"], want["labels"]) and np.array_equal(outlined["outlines"].verts, found["outlines"].verts)
    assert np.array_equal(outlined["ring_area2"], traced["ring_area2"])

    for with_outlines in (True, False):
        check_empty(part(call(lars.Regions(above=NOTHING, index=index, want_outlines=with_outlines))), with_outlines)

    meanabs = zone_meanabs(plane, want["labels"], None, r)
    same_figures(part(call(found["labels"], n_zones=r)), found, meanabs)                     # the regions' labels as a raster
    same_figures(part(call(found["outlines"])), found, meanabs)                              # the regions' outlines as polygons

    last = call(labels, n_zones=nz)
    same_bytes(part(first), part(last))
    same_figures(part(first), part(last), zone_meanabs(plane, labels, None, nz))
    return first, last


def test_a_plane():
    plane = zc.plane(*SHAPE)
    in_turn(lambda zones, **kw: lars.zonal_statistics(plane, zones, "NDVI", want_hist=True, **kw), lambda result: result, lambda result: plane, None)


def test_a_picture():
    img, _, _ = zc.plots_picture(*SHAPE)

    def part(result):
        return {**{k: v for k, v in result["zones"].items() if k not in INDEX_NAMES}, **result["zones"]["NDVI"]}
    first, last = in_turn(lambda zones, **kw: lars.process_image_zones(img, zones, want_hist=True, **kw), part, lambda result: result["indices"]["NDVI"]["index"],
                          "NDVI")
    assert first["valid_pixels"] == last["valid_pixels"] and first["corrected"].tobytes() == last["corrected"].tobytes()
    for t in INDEX_NAMES:
        assert first["indices"][t]["index"].tobytes() == last["indices"][t]["index"].tobytes()
        same_bytes(first["zones"][t], last["zones"][t])
