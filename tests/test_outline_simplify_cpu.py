"""The definition of simplified outlines (outline_simplify_model.py) against a second, naive statement of it -- plain recursion,
distances as fractions -- on traced rings, its properties, and every check ``region_outlines(simplify=)``, ``Regions(simplify=)`` and
``simplify_outlines`` make on the host.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import outline_simplify_cases as oc
import outline_simplify_model as sm
import lars_image_processing_amd as lars
from lars_image_processing_amd import zones


# ---- the naive statement ----
def distance2(a, b, p):
    """The squared distance from p to the segment a b, exactly."""
    ab, ap = (b[0] - a[0], b[1] - a[1]), (p[0] - a[0], p[1] - a[1])
    len2 = ab[0] ** 2 + ab[1] ** 2
    if len2 == 0:
        return Fraction(ap[0] ** 2 + ap[1] ** 2)
    t = max(Fraction(0), min(Fraction(1), Fraction(ap[0] * ab[0] + ap[1] * ab[1], len2)))
    foot = (a[0] + t * ab[0], a[1] + t * ab[1])
    return (p[0] - foot[0]) ** 2 + (p[1] - foot[1]) ** 2


def naive_keep(chain, a, b, tolerance2, keep):
    if b - a < 2:
        return
    d = [distance2(chain[a], chain[b], chain[k]) for k in range(a + 1, b)]
    k = a + 1 + d.index(max(d))                                       # the first of the largest
    if d[k - a - 1] > tolerance2:
        keep.add(k)
        naive_keep(chain, a, k, tolerance2, keep)
        naive_keep(chain, k, b, tolerance2, keep)


def naive_ring(pts, tq):
    n = len(pts)
    keep = {0}
    naive_keep(pts + [pts[0]], 0, n, Fraction(tq * tq, 256), keep)
    out = [pts[i] for i in sorted(keep - {n})]
    own, got = sm.area2(pts), sm.area2(out)
    if len(out) < 3 or got == 0 or (got > 0) != (own > 0):
        return pts, True
    return out, False


def ring_points(traced, i):
    s, c = int(traced["ring_start"][i]), int(traced["ring_count"][i])
    return [tuple(v) for v in traced["verts"][s:s + c].tolist()]


def check_against_naive(traced, tq):
    """The model's rings are the naive statement's, and have the three properties; -> [(vertices traced, written, restored)]"""
    want = sm.simplify(traced, tq)
    assert want["n_rings"] == traced["n_rings"] and np.array_equal(want["ring_label"], traced["ring_label"]) and np.array_equal(want["ring_key"], traced["ring_key"])
    assert np.array_equal(want["ring_start"], np.cumsum(want["ring_count"]) - want["ring_count"]) and want["n_vertices"] == int(want["ring_count"].sum())
    tolerance2, rows = Fraction(tq * tq, 256), []
    for i in range(traced["n_rings"]):
        pts, out = ring_points(traced, i), ring_points(want, i)
        naive, back = naive_ring(pts, tq)
        assert out == naive and bool(want["restored"][i]) == back, (i, tq)
        assert int(want["ring_area2"][i]) == sm.area2(out)
        # a subsequence that holds v[0]
        assert out[0] == pts[0]
        at, places = 0, []
        for v in out:
            at = pts.index(v, at) + 1
            places.append(at - 1)
        # restored exactly when the result collapses
        kept, _ = sm.kept_of(pts, tq)
        result = [pts[k] for k in kept]
        collapses = len(result) < 3 or sm.area2(result) == 0 or (sm.area2(result) > 0) != (sm.area2(pts) > 0)
        assert collapses == back and (out == pts if back else out == result)
        # every dropped vertex is within the tolerance of the segment between its kept neighbours
        if not back:
            chain, ends = pts + [pts[0]], kept + [len(pts)]
            for a, b in zip(ends, ends[1:]):
                for k in range(a + 1, b):
                    assert distance2(chain[a], chain[b], chain[k]) <= tolerance2, (i, tq, k)
        rows.append((len(pts), len(out), back))
    return rows


@pytest.mark.parametrize("connectivity", [4, 8])
def test_all_masks_of_three_by_three(connectivity):
    traced = oc.labelled("all_3x3", connectivity)[2]
    for tq in oc.TQS:
        check_against_naive(traced, tq)


@pytest.mark.parametrize("chunk", range(4))
def test_fuzzed_masks_of_two_kinds(chunk):
    kinds = set()
    for seed in range(chunk * 50, chunk * 50 + 50):
        kinds.add(oc.fuzz_mask(seed)[1])
        traced = oc.labelled("fuzz_%d" % seed, 4 if seed % 4 < 2 else 8)[2]
        for tq in oc.TQS:
            check_against_naive(traced, tq)
    assert kinds == {"noise", "smooth"}


def test_the_smoothed_masks_lose_vertices():
    """The condition on the case set: among the smoothed masks, at least half of the rings with more than 8 vertices lose a vertex and
    are not restored at a tolerance of one pixel -- so no suite passes on rings that all stay as traced."""
    long_rings = shorter = 0
    for seed in range(1, oc.FUZZ, 2):
        assert oc.fuzz_mask(seed)[1] == "smooth"
        for connectivity in (4, 8):
            traced, want = oc.labelled("fuzz_%d" % seed, connectivity)[2], oc.simplified("fuzz_%d" % seed, connectivity, 16)
            big = traced["ring_count"] > 8
            long_rings += int(big.sum())
            shorter += int((big & (want["ring_count"] < traced["ring_count"]) & ~want["restored"]).sum())
    assert long_rings >= 200 and 2 * shorter >= long_rings, (long_rings, shorter)


def test_the_level_by_level_statement_is_the_model():
    for name, connectivity in (("comb_24", 8), ("serpentine", 4), ("blobs", 8), ("checkerboard", 8), ("fuzz_7", 8), ("fuzz_12", 4)):
        traced = oc.labelled(name, connectivity)[2]
        for tq in (8, 16, 48):
            one, two = sm.simplify(traced, tq), sm.simplify_levels(traced, tq)
            assert set(one) == set(two) and all(np.array_equal(one[k], two[k]) for k in one), (name, tq)


def test_the_named_cases_are_what_they_are_for():
    comb = oc.simplified("comb_24", 8, 16)
    assert comb["n_rings"] == 1 and comb["rounds"] > 2 * oc.BATCH and not comb["restored"].any()      # about two levels a tooth: several host batches
    for connectivity in (4, 8):
        snake = oc.labelled("serpentine", connectivity)[2]
        assert snake["n_rings"] == 1 and snake["n_vertices"] >= 3 * oc.CHUNK                        # one stretch across several workgroups
        board = oc.simplified("checkerboard", connectivity, 16)
        assert board["restored"].sum() >= board["n_rings"] - 1 and board["n_rings"] > 1900
    blobs = oc.labelled("blobs", 8)[2]
    ends = np.cumsum(blobs["ring_count"] + 1)
    assert blobs["n_rings"] > 20 and (ends[:-1] % 64 != 0).sum() > 20 and len(set(blobs["ring_label"].tolist())) > 3     # rings that end mid-wave


def test_hand_built_rings():
    """What the GPU entry test feeds the device, judged by the model and the naive statement first."""
    for name in oc.hand_built():
        given, tq, want = oc.hand_case(name)
        check_against_naive(given, tq)
    for tq, b, p, diff in oc.NEAR:                                    # the near-collinear vertex: less than 256 from the threshold, on either side
        m, len2 = sm.measure((0, 0), b, p)
        assert 256 * m - tq * tq * len2 == diff and 0 < abs(diff) < 256 and sm.far(m, len2, tq) == (diff > 0)
        kept = oc.hand_case("near_%d_%s" % (tq, "above" if diff > 0 else "below"))[2]
        assert kept["ring_count"].tolist() == ([4, 4] if diff > 0 else [3, 3])
    assert max(tq * tq * (b[0] ** 2 + b[1] ** 2) for tq, b, _, _ in oc.NEAR).bit_length() == 55
    m, len2 = sm.measure((0, oc.M), (oc.M, 0), (oc.M, oc.M))          # the corner against the diagonal of the largest raster
    assert m == oc.M ** 4 and m.bit_length() == 60 and (4064 * 4064 * len2).bit_length() == 55
    flip = oc.hand_case("flip")
    assert flip[2]["restored"].tolist() == [True] and np.array_equal(flip[2]["verts"], flip[0]["verts"])
    pts = ring_points(flip[0], 0)
    result = [pts[k] for k in sm.kept_of(pts, flip[1])[0]]
    assert len(result) >= 3 and sm.area2(result) * sm.area2(pts) < 0
    assert oc.hand_case("triangle_thin")[2]["restored"].tolist() == [True] and oc.hand_case("triangle")[2]["ring_count"].tolist() == [3]
    square = oc.hand_case("square_equal_maxima")[2]                   # (0, 8) and (8, 0) are as far from the diagonal: the smaller index wins, both stay
    assert square["ring_count"].tolist() == [4, 4]
    pinch = oc.hand_case("pinch")
    assert pinch[2]["ring_count"].tolist() == [10, 10]               # stretches between the two visits of a point: len2 == 0


# ---- the host's checks ----
def test_simplify_tq():
    who = "region_outlines"
    assert zones._simplify_tq(None, who) == 0 and zones._simplify_tq(0, who) == 0 and zones._simplify_tq(0.01, who) == 0
    assert zones._simplify_tq(0.03, who) == 0 and zones._simplify_tq(0.03125, who) == 1 and zones._simplify_tq(np.float32(0.5), who) == 8
    assert zones._simplify_tq(1, who) == 16 and zones._simplify_tq(1.4375, who) == 23 and zones._simplify_tq(np.int64(3), who) == 48
    assert zones._simplify_tq(254, who) == 4064 == sm.TQ_MAX
    for tolerance in (0.2, 1.47, 17.03, 253.99):
        assert zones._simplify_tq(tolerance, who) == math.floor(tolerance * 16 + 0.5)
    for bad in (-1, -0.001, 254.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="region_outlines: simplify must be"):
            zones._simplify_tq(bad, who)
    for bad in (True, np.bool_(False), "1", b"1", [1], (1,)):
        with pytest.raises(TypeError, match="region_outlines: simplify must be a number of pixels or None"):
            zones._simplify_tq(bad, who)


def test_refusals_on_the_host():
    mask = np.ones((4, 4), dtype=bool)
    with pytest.raises(ValueError, match="region_outlines: simplify must be 0 to 254 pixels"):
        lars.region_outlines(mask, simplify=300)
    with pytest.raises(TypeError, match="region_outlines: simplify must be a number"):
        lars.region_outlines(mask, simplify="1")
    wide = np.zeros((1, 32768), dtype=bool)
    with pytest.raises(ValueError, match="region_outlines: the raster is 1 x 32768; outlines are simplified on at most 32767 a side"):
        lars.region_outlines(wide, simplify=1)
    with pytest.raises(ValueError, match="Regions: simplify is the tolerance of the outlines: it needs want_outlines=True"):
        lars.Regions(mask=mask, simplify=1)
    with pytest.raises(ValueError, match="Regions: simplify is the tolerance of the outlines"):
        lars.Regions(above=0.2, simplify=0)
    with pytest.raises(ValueError, match="Regions: simplify must be 0 to 254"):
        lars.Regions(above=0.2, want_outlines=True, simplify=-2)
    assert lars.Regions(above=0.2, want_outlines=True, simplify=None).simplify_tq == 0
    assert lars.Regions(above=0.2, want_outlines=True, simplify=0.5).simplify_tq == 8
    tall = lars.Regions(mask=np.zeros((32768, 1), dtype=bool), want_outlines=True, simplify=2)
    with pytest.raises(ValueError, match="zonal_statistics: the raster is 32768 x 1; outlines are simplified on at most 32767 a side"):
        lars.zonal_statistics(np.zeros((32768, 1), dtype=np.float32), tall, "NDVI")


def outlines_dict(verts):
    polys = lars.Polygons([np.asarray(verts, dtype=np.float64)])
    return {"outlines": polys, "ring_area2": np.array([200], dtype=np.int64), "n_rings": 1, "n_vertices": len(verts)}


def test_simplify_outlines_refusals_on_the_host():
    good = [[0, 0], [10, 0], [10, 10], [0, 10]]
    for bad, text in (([[0, 0], [10.5, 0], [10, 10], [0, 10]], "whole numbers"), ([[0, 0], [32768, 0], [10, 10], [0, 10]], "whole numbers of 0 to 32767"),
                      ([[0, 0], [-1, 0], [10, 10], [0, 10]], "whole numbers of 0 to 32767")):
        with pytest.raises(ValueError, match="simplify_outlines: the vertices must be " + text):
            lars.simplify_outlines(outlines_dict(bad), 1)
    with pytest.raises(TypeError, match="simplify_outlines: result must be the dict"):
        lars.simplify_outlines([good], 1)
    with pytest.raises(ValueError, match="simplify_outlines: this result holds no outlines"):
        lars.simplify_outlines({"labels": np.zeros((2, 2))}, 1)
    with pytest.raises(ValueError, match="simplify_outlines: simplify must be 0 to 254"):
        lars.simplify_outlines(outlines_dict(good), 255)
    with pytest.raises(ValueError, match="ring_area2 has shape"):
        lars.simplify_outlines({**outlines_dict(good), "ring_area2": np.zeros(2, dtype=np.int64)}, 1)
    # no tolerance, or no region: a copy, nothing to run
    given = outlines_dict(good)
    for nothing in (None, 0, 0.01):
        got = lars.simplify_outlines(given, nothing)
        assert got is not given and set(got) == set(given) and all(got[k] is given[k] for k in given)
    empty = {"outlines": None, "ring_area2": np.zeros(0, dtype=np.int64), "n_rings": 0, "n_vertices": 0}
    assert lars.simplify_outlines(empty, 2) == empty


def test_driver_takes_the_tolerance_only_with_the_geojson(tmp_path):
    from lars_image_processing_amd import driver
    with pytest.raises(ValueError, match="regions_simplify is the tolerance of the outlines in the GeoJSON: it goes with regions_geojson"):
        driver._zones_argument(None, None, "NDVI:above:0.2", False, None, 1.0)
    assert driver._zones_argument(None, None, "NDVI:above:0.2", True, None, 1.5) == {"regions": "NDVI:above:0.2", "regions_geojson": True, "regions_simplify": 1.5}
    assert "regions_simplify" not in driver._zones_argument(None, None, "NDVI:above:0.2", True)
    for flags in (["--regions-simplify", "1"], ["--regions", "NDVI:above:0.2", "--regions-simplify", "1"],
                  ["--regions", "NDVI:above:0.2", "--regions-geojson", "--regions-simplify", "300"]):
        with pytest.raises(SystemExit):
            driver.main([str(tmp_path), str(tmp_path / "out"), *flags])
