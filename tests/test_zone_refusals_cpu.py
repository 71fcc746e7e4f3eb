"""What lars_h_process_image_zones, _zones_polygons, _regions and _regions_outlines refuse, message for message (zone_refusal_cases.py):
every check of the picture, of the entry points themselves and of the three kinds of zones, on a 4 x 5 uint8 picture.  These entry
points answer before they touch a device, so the table runs without one; every row has a fault, so none ever reaches it.  After each
refusal the out-parameters hold what the header promises: *valid_pixels, *bad_labels and *n_regions -1, the outline counts -1 once the
outline room itself was looked at and untouched before that."""
import ctypes as C

import numpy as np
import pytest

import zone_refusal_cases as zr
from zone_refusal_cases import H, KEPT, W

HEAD = ("img", "h", "w", "channels", "dtype", "apply_wb", "index_mask", "want_hist", "out_wb", "out_index", "stats", "medians", "out_rgba", "cmap_lut",
        "valid", "use_alpha", "has_nodata", "nodata", "valid_pixels")
REGION_TAIL = ("mask", "source_index", "mode", "t", "connectivity", "min_pixels", "capacity", "zone_stats", "zone_medians", "table", "n_regions",
               "labels_out", "label_bytes", "label_bytes_out")
ENTRIES = {
    "lars_h_process_image_zones": (HEAD + ("zones", "zone_bytes", "nzones", "zone_stats", "zone_medians", "bad_labels"), zr.raster_arguments),
    "lars_h_process_image_zones_polygons": (HEAD + ("verts", "nverts", "ring_starts", "nrings", "poly_starts", "npolys", "zone_stats", "zone_medians",
                                                    "labels_out", "label_bytes"), zr.polygon_arguments),
    "lars_h_process_image_regions": (HEAD + REGION_TAIL, lambda: zr.region_arguments(False)),
    "lars_h_process_image_regions_outlines": (HEAD + REGION_TAIL + ("outlines",), lambda: zr.region_arguments(True)),
}


def picture():
    return {"img": np.full((H, W, 4), 9, dtype=np.uint8), "h": H, "w": W, "channels": 4, "dtype": 1, "apply_wb": 0, "index_mask": 1, "want_hist": 0,
            "out_wb": None, "out_index": None, "stats": None, "medians": None, "out_rgba": None, "cmap_lut": None, "valid": None, "use_alpha": 0,
            "has_nodata": 0, "nodata": 0, "valid_pixels": C.c_int64(KEPT)}


NO_RECORDS = "the zones' records and medians are required"
INDEX_MASK = "index_mask must name one to three indices"
# the picture's own checks and the entry points' own, the same for the four: name -> (changes, message)
PICTURE_FAULTS = {
    "img_null": ({"img": None}, "image must be a non-empty [h][w][>=3] array"),
    "h_0": ({"h": 0}, "image must be a non-empty [h][w][>=3] array"),
    "w_below_0": ({"w": -1}, "image must be a non-empty [h][w][>=3] array"),
    "channels_2": ({"channels": 2}, "image must be a non-empty [h][w][>=3] array"),
    "dtype_3": ({"dtype": 3}, "dtype must be LARS_U8 or LARS_U16"),
    "alpha_of_3_channels": ({"use_alpha": 1, "channels": 3}, "the alpha rule needs 4 or more channels, got 3"),
    "nodata_256": ({"has_nodata": 1, "nodata": 256}, "nodata 256 is outside the sample type's range"),
    "nodata_below_0": ({"has_nodata": 1, "nodata": -1}, "nodata -1 is outside the sample type's range"),
    "nodata_65536_of_uint16": ({"dtype": 2, "has_nodata": 1, "nodata": 65536}, "nodata 65536 is outside the sample type's range"),
    "rgba_without_colormap": ({"out_rgba": zr.Ptr3(np.zeros((H, W, 4), dtype=np.uint8), None, None)},
                              "out_rgba[0] needs cmap_lut[0] (the 256 colormap entries leave no free one for \"no data\": entry planes are not built with a mask)"),
    "index_mask_0": ({"index_mask": 0}, INDEX_MASK),
    "index_mask_8": ({"index_mask": 8}, INDEX_MASK),
    # two faults: the picture is looked at before the mask of indices, and both before the zones
    "dtype_3_and_index_mask_0": ({"dtype": 3, "index_mask": 0}, "dtype must be LARS_U8 or LARS_U16"),
    "index_mask_0_and_no_records": ({"index_mask": 0, "zone_stats": None}, INDEX_MASK),
}


def cases():
    """(entry point, name, changes, message, the outline counts afterwards or None)"""
    out = []
    for entry in ENTRIES:
        kept = (KEPT,) * 3 if entry.endswith("outlines") else None
        out += [(entry, name, change, text, kept) for name, (change, text) in PICTURE_FAULTS.items()]
        if entry == "lars_h_process_image_zones":
            out += [(entry, name, change, text, None) for name, (change, text) in zr.RASTER_FAULTS.items()]
            out += [(entry, "img_null_and_zones_null", {"img": None, "zones": None}, "image must be a non-empty [h][w][>=3] array", None),
                    (entry, "index_mask_8_and_zone_bytes_3", {"index_mask": 8, "zone_bytes": 3}, INDEX_MASK, None)]
            continue
        out += [(entry, "records_null", {"zone_stats": None}, NO_RECORDS, kept), (entry, "medians_null", {"zone_medians": None}, NO_RECORDS, kept)]
        if entry == "lars_h_process_image_zones_polygons":
            out += [(entry, name, change, text, None) for name, (change, text) in zr.POLYGON_FAULTS.items()]
            # h and w are the picture's: nothing of the picture is read before the polygons are refused
            out += [(entry, "raster_above_2_to_24", {"h": (1 << 24) + 1, "w": 1}, zr.POLYGON_RASTER, None),
                    (entry, "records_null_and_npolys_0", {"zone_stats": None, "npolys": 0}, NO_RECORDS, None)]
            continue
        source = "source_index {} is not among the indices of index_mask"
        out += [(entry, "source_index_3", {"mask": None, "mode": 1, "source_index": 3}, source.format(3), kept),
                (entry, "source_index_below_0", {"mask": None, "mode": 1, "source_index": -1}, source.format(-1), kept),
                (entry, "source_index_outside_index_mask", {"mask": None, "mode": 1, "source_index": 1, "index_mask": 5}, source.format(1), kept),
                (entry, "source_index_3_and_connectivity_5", {"mask": None, "mode": 1, "source_index": 3, "connectivity": 5}, source.format(3), kept),
                (entry, "medians_null_and_source_index_3", {"mask": None, "mode": 1, "source_index": 3, "zone_medians": None}, NO_RECORDS, kept),
                (entry, "raster_of_2_to_31_pixels", {"h": 1 << 16, "w": 1 << 15}, zr.REGION_RASTER, kept)]
        out += [(entry, name, *row) for name, row in zr.region_faults(kept is not None, zr.ZONES_MAX).items()]
        if kept:
            out += [(entry, "outline_raster_of_2_to_29_pixels", {"h": 1 << 15, "w": 1 << 14}, zr.OUTLINE_RASTER.format(1 << 15, 1 << 14), (-1,) * 3),
                    (entry, "outline_raster_of_2_to_29_pixels_and_rings_null", {"h": 1 << 15, "w": 1 << 14, "outlines": zr.outlines(ring_ptr=False)},
                     zr.OUTLINE_RASTER.format(1 << 15, 1 << 14), (-1,) * 3)]
    return out


CASES = {f"{entry[len('lars_h_process_image_'):]}-{name}": (entry, change, text, counts) for entry, name, change, text, counts in cases()}


def test_every_kind_has_its_rows():
    assert len(CASES) == len(cases())                                             # no two rows of one entry point share a name
    for entry in ENTRIES:
        assert sum(1 for e, *_ in CASES.values() if e == entry) >= len(PICTURE_FAULTS) + len(zr.RASTER_FAULTS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(name):
    entry, change, text, counts = CASES[name]
    order, zones = ENTRIES[entry]
    a = {**picture(), **zones(), **change}
    if counts:
        a["outlines"].n_rings = a["outlines"].n_vertices = a["outlines"].n_edges = KEPT
    status, message = zr.invoke(entry, order, a)
    assert status == -1 and message == f"{entry}: {text}"
    assert a["valid_pixels"].value == -1
    if "bad_labels" in a:
        assert a["bad_labels"].value == -1
    if a.get("n_regions") is not None:
        assert a["n_regions"].value == -1 and a["label_bytes_out"].value == KEPT
    if counts:
        assert zr.counts_of(a["outlines"]) == counts


def test_outlines_null_is_the_call_without_outlines():
    """lars_h_process_image_regions forwards to _regions_outlines with NULL outlines, and the messages name the call that was made."""
    order, zones = ENTRIES["lars_h_process_image_regions_outlines"]
    a = {**picture(), **zones(), "outlines": None, "connectivity": 5}
    status, message = zr.invoke("lars_h_process_image_regions_outlines", order, a)
    assert status == -1 and message == "lars_h_process_image_regions: connectivity must be 4 or 8, got 5"
    assert a["valid_pixels"].value == -1 and a["n_regions"].value == -1
