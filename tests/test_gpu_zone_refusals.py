"""What the zone entry points that open the device first refuse, message for message (zone_refusal_cases.py): lars_h_zonal_stats_f32,
_polygons_f32, _regions_f32 and _regions_outlines_f32, lars_h_label_regions, lars_h_region_outlines and lars_h_rasterize_zones on a
4 x 5 raster.  A refused call launches nothing and leaves *bad_labels and *n_regions -1.  Then each of them once with good arguments,
straight after a refusal on the same thread, against the models: a refusal leaves the thread's workspace usable."""
import ctypes as C

import numpy as np
import pytest

import outlines_model as om
import regions_model as gm
import zonal_model as zm
import zone_raster_model as rm
import zone_refusal_cases as zr
from lars_image_processing_amd import zones as lz
from zone_refusal_cases import H, KEPT, W

pytestmark = pytest.mark.gpu

REGION_PLANE = ("x", "mask", "mode", "t", "connectivity", "min_pixels", "valid", "h", "w", "threshold", "want_hist", "capacity", "zone_stats",
                "zone_medians", "table", "n_regions", "labels_out", "label_bytes", "label_bytes_out")
LABEL_REGIONS = ("mask", "h", "w", "connectivity", "min_pixels", "label_bytes", "labels_out", "label_bytes_out", "table", "capacity", "n_regions")
POLYGON_HEAD = ("verts", "nverts", "ring_starts", "nrings", "poly_starts", "npolys")
ENTRIES = {
    "lars_h_zonal_stats_f32": (("x", "zones", "zone_bytes", "valid", "h", "w", "nzones", "threshold", "want_hist", "zone_stats", "zone_medians",
                                "bad_labels"), zr.raster_arguments),
    "lars_h_zonal_stats_polygons_f32": (("x",) + POLYGON_HEAD + ("valid", "h", "w", "threshold", "want_hist", "zone_stats", "zone_medians", "labels_out",
                                                                "label_bytes"), zr.polygon_arguments),
    "lars_h_zonal_stats_regions_f32": (REGION_PLANE, lambda: zr.region_arguments(False)),
    "lars_h_zonal_stats_regions_outlines_f32": (REGION_PLANE + ("outlines",), lambda: zr.region_arguments(True)),
    "lars_h_label_regions": (LABEL_REGIONS, lambda: zr.region_arguments(False)),
    "lars_h_region_outlines": (LABEL_REGIONS + ("outlines",), lambda: zr.region_arguments(True)),
    "lars_h_rasterize_zones": (POLYGON_HEAD + ("h", "w", "label_bytes", "labels_out"), zr.polygon_arguments),
}
MOST = {"lars_h_label_regions": 0x7FFFFFFF, "lars_h_region_outlines": 0x7FFFFFFF}


def raster():
    return {"x": zr.plane(), "valid": None, "h": H, "w": W, "threshold": np.float32(0.2), "want_hist": 1}


NO_PLANE = "x must be a non-empty [h][w] float32 array"
NO_RECORDS = "the zones' records and medians are required"


def cases():
    """(entry point, name, changes, message, the outline counts afterwards or None, *n_regions afterwards)"""
    out = []
    for entry in ENTRIES:
        outlined = entry.endswith(("outlines", "outlines_f32"))
        kept = (KEPT,) * 3 if outlined else None
        if "zonal_stats" in entry:
            out += [(entry, "x_null", {"x": None}, NO_PLANE, kept, -1), (entry, "h_0", {"h": 0}, NO_PLANE, kept, -1), (entry, "w_below_0", {"w": -1}, NO_PLANE, kept, -1)]
        if entry == "lars_h_zonal_stats_f32":
            out += [(entry, name, change, text, None, -1) for name, (change, text) in zr.RASTER_FAULTS.items()]
            out += [(entry, "x_null_and_zone_bytes_3", {"x": None, "zone_bytes": 3}, NO_PLANE, None, -1)]
        elif "regions" not in entry and "outlines" not in entry:                 # polygons
            if "zonal_stats" in entry:
                out += [(entry, "records_null", {"zone_stats": None}, NO_RECORDS, None, -1), (entry, "medians_null", {"zone_medians": None}, NO_RECORDS, None, -1),
                        (entry, "records_null_and_npolys_0", {"zone_stats": None, "npolys": 0}, NO_RECORDS, None, -1)]
            else:
                out += [(entry, "labels_null", {"labels_out": None}, "labels == NULL", None, -1),
                        (entry, "labels_null_and_npolys_0", {"labels_out": None, "npolys": 0}, "labels == NULL", None, -1)]
            out += [(entry, name, change, text, None, -1) for name, (change, text) in zr.POLYGON_FAULTS.items()]
            out += [(entry, "raster_above_2_to_24", {"h": 1, "w": (1 << 24) + 1}, zr.POLYGON_RASTER, None, -1)]
        else:
            plane_call = "zonal_stats" in entry
            if plane_call:
                out += [(entry, "records_null", {"zone_stats": None}, NO_RECORDS, kept, -1), (entry, "medians_null", {"zone_medians": None}, NO_RECORDS, kept, -1),
                        (entry, "records_null_and_connectivity_5", {"zone_stats": None, "connectivity": 5}, NO_RECORDS, kept, -1)]
            else:
                required = "mask and labels are required"
                out += [(entry, "mask_null", {"mask": None}, required, kept, -1), (entry, "labels_null", {"labels_out": None}, required, kept, -1),
                        (entry, "labels_null_and_connectivity_5", {"labels_out": None, "connectivity": 5}, required, kept, -1)]
            if entry == "lars_h_region_outlines":                                 # answered before anything else of the call
                out += [(entry, "outlines_null", {"outlines": None}, "outlines == NULL", None, KEPT),
                        (entry, "outlines_null_and_mask_null", {"outlines": None, "mask": None}, "outlines == NULL", None, KEPT)]
            out += [(entry, "raster_of_2_to_31_pixels", {"h": 1 << 16, "w": 1 << 15}, zr.REGION_RASTER, kept, -1)]
            out += [(entry, name, *row, -1) for name, row in zr.region_faults(outlined, MOST.get(entry, zr.ZONES_MAX), needs_mask=not plane_call).items()]
            if outlined:
                out += [(entry, "outline_raster_of_2_to_29_pixels", {"h": 1 << 15, "w": 1 << 14}, zr.OUTLINE_RASTER.format(1 << 15, 1 << 14), (-1,) * 3, -1)]
    return out


CASES = {f"{entry[len('lars_h_'):]}-{name}": (entry, *rest) for entry, name, *rest in cases()}


def refuse(name):
    entry, change, text, counts, found = CASES[name]
    order, zones = ENTRIES[entry]
    a = {**raster(), **zones(), **change}
    if counts:
        a["outlines"].n_rings = a["outlines"].n_vertices = a["outlines"].n_edges = KEPT
    status, message = zr.invoke(entry, order, a)
    assert status == -1 and message == f"{entry}: {text}"
    if "bad_labels" in a:
        assert a["bad_labels"].value == -1
    if "capacity" in a and a["n_regions"] is not None:
        assert a["n_regions"].value == found and a["label_bytes_out"].value == KEPT
    if counts:
        assert zr.counts_of(a["outlines"]) == counts


def test_no_two_rows_of_an_entry_point_share_a_name():
    assert len(CASES) == len(cases())
    assert {e for e, *_ in CASES.values()} == set(ENTRIES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(name):
    refuse(name)


def good(entry):
    """The good call of ``entry`` straight after one of its refusals -> its arguments, filled."""
    refuse(next(n for n, row in CASES.items() if row[0] == entry))
    order, zones = ENTRIES[entry]
    a = {**raster(), **zones()}
    status, message = zr.invoke(entry, order, a)
    assert status == 0, message
    return a


def figures(a, nz):
    count, out = lz._figures(a["zone_stats"].reshape(-1)[:nz], a["zone_medians"].reshape(-1, 2)[:nz], True)
    return {"zone": np.arange(1, nz + 1, dtype=np.int64), "pixels": count, **out}


def check_regions(a, with_outlines):
    want = gm.label(zr.MASK, 8, 1)
    r = want["n_regions"]
    assert a["n_regions"].value == r and a["label_bytes_out"].value == 1
    assert np.array_equal(a["labels_out"].reshape(-1).view(np.uint8)[:H * W].reshape(H, W), want["labels"])
    table = a["table"][:r]
    for key in ("area", "bbox", "row_sum", "col_sum"):
        assert np.array_equal(table[key], want[key]), key
    if with_outlines:
        o, traced = a["outlines"], om.trace(want["labels"], 8)
        assert zr.counts_of(o) == (traced["n_rings"], traced["n_vertices"], traced["n_edges"])
        assert np.array_equal(o.vert_rows[:o.n_vertices], traced["verts"])
        for field in ("label", "key", "start", "count", "area2"):
            assert np.array_equal(o.ring_rows[:o.n_rings][field], traced["ring_" + field]), field
    return want


def test_label_raster_after_a_refusal():
    a = good("lars_h_zonal_stats_f32")
    assert a["bad_labels"].value == 0
    zm.check_zone_figures(figures(a, 2), zm.zonal_model(zr.plane(), zr.ZONES, "NDVI", n_zones=2), "NDVI")


def test_polygons_after_a_refusal():
    want = rm.labels(zr.SQUARES, (H, W))
    a = good("lars_h_zonal_stats_polygons_f32")
    assert np.array_equal(a["labels_out"], want)
    zm.check_zone_figures(figures(a, 2), zm.zonal_model(zr.plane(), want, "NDVI", n_zones=2), "NDVI")
    assert np.array_equal(good("lars_h_rasterize_zones")["labels_out"], want)


@pytest.mark.parametrize("with_outlines", [False, True])
def test_regions_after_a_refusal(with_outlines):
    tail = "_outlines_f32" if with_outlines else "_f32"
    a = good("lars_h_zonal_stats_regions" + tail)
    want = check_regions(a, with_outlines)
    zm.check_zone_figures(figures(a, want["n_regions"]), zm.zonal_model(zr.plane(), want["labels"], "NDVI", n_zones=want["n_regions"]), "NDVI")
    check_regions(good("lars_h_region_outlines" if with_outlines else "lars_h_label_regions"), with_outlines)
