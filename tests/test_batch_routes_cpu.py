"""TileBatch.process' route planner (batch.plan_process) over the full grid of its inputs, against a decision table (no GPU)."""
import itertools

import numpy as np
import pytest

from lars_image_processing_amd import batch
from lars_image_processing_amd._ffi import U8, U16

TYPES = ("NDVI", "GNDVI", "NDWI")
SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(TYPES, r)]
NPIX = (32 * 32, 33 * 31, 1 << 28, (1 << 28) + 1)         # npix % 4 == 0 or not, npix * 6 below or above 2^30
OUTPUTS = ("none", "planes", "missing plane", "wb plane")  # what ``outputs`` holds (a missing plane changes no decision)


def _one_read(c):
    return (c["route"] != "classic" and not c["reuse"] and c["code"] == U8 and c["channels"] in (3, 4)
            and (c["ntiles"] == 1 or c["npix"] % 4 == 0))


def _select(c):
    return (c["medians"] and c["code"] == U8 and c["channels"] == 3 and c["npix"] * 6 < (1 << 30)
            and (c["ntiles"] == 1 or c["npix"] % 4 == 0))


# First matching row wins: what process() did before the planner existed, branch by branch.
TABLE = [
    (ValueError, lambda c: c["route"] == "joint" and c["reuse"] and c["outputs"] == "none"),
    ("measure", lambda c: _one_read(c) and c["outputs"] == "none" and c["route"] == "auto" and not c["medians"] and not c["sumsq"]),
    ("one-read", lambda c: _one_read(c) and c["outputs"] == "none"),
    (ValueError, lambda c: c["route"] == "joint" and c["outputs"] == "none"),
    ("one-read+planes", lambda c: _one_read(c) and c["outputs"] != "wb plane"
        and (c["medians"] or c["hist"] or len(c["indices"]) == 1 or set(c["indices"]) == {"GNDVI", "NDWI"})),
    ("select", lambda c: _select(c) and c["outputs"] == "none" and len(c["indices"]) in (1, 3)),
    ("per-pixel+select", _select),
    ("per-pixel+radix", lambda c: c["medians"]),
    ("per-pixel", lambda c: True),
]


def expected(c):
    return next(route for route, when in TABLE if when(c))


def plan(c):
    return batch.plan_process(c["code"], c["channels"], c["ntiles"], c["npix"], c["indices"], c["white_balance"], c["hist"],
                              c["medians"], c["sumsq"], c["route"], outputs=c["outputs"] != "none",
                              wb_plane=c["outputs"] == "wb plane", reuse=c["reuse"])


def grid():
    keys = ("code", "channels", "ntiles", "npix", "indices", "route", "medians", "hist", "sumsq", "outputs", "reuse", "white_balance")
    for values in itertools.product((U8, U16), (3, 4), (1, 7), NPIX, SUBSETS, ("auto", "joint", "classic"),
                                    (False, True), (False, True), (False, True), OUTPUTS, (False, True), (True,)):
        yield dict(zip(keys, values))


def test_planner_follows_the_decision_table():
    seen = {}
    for c in grid():
        want = expected(c)
        if want is ValueError:
            with pytest.raises(ValueError, match="route='joint'"):
                plan(c)
        else:
            assert plan(c) == want, c
            assert plan(dict(c, white_balance=False)) == want, c
        seen[want] = seen.get(want, 0) + 1
    assert set(seen) == {ValueError, "measure", "one-read", "one-read+planes", "select", "per-pixel+select", "per-pixel",
                         "per-pixel+radix"}, seen


def test_after_measuring_the_planner_takes_the_route_picked():
    for c in grid():
        if expected(c) == "measure":
            assert plan(dict(c, route="joint")) == "one-read" and plan(dict(c, route="classic")) == "per-pixel", c


def test_planner_messages():
    base = dict(code=U8, channels=3, ntiles=2, npix=1024, indices=TYPES, white_balance=True, hist=False, medians=False, sumsq=False,
                route="joint", outputs="none", reuse=False)
    with pytest.raises(ValueError, match="cannot honour recompute_tables=False"):
        plan(dict(base, reuse=True))
    with pytest.raises(ValueError, match="3 or 4 channels"):
        plan(dict(base, code=U16))
    for bad in ("Joint", "one-read", "", None):
        with pytest.raises(ValueError, match="route must be auto, joint or classic"):
            plan(dict(base, route=bad))


def test_index_mask():
    assert batch.index_mask(()) == 0
    for sub in SUBSETS:
        assert batch.index_mask(sub) == sum(1 << TYPES.index(t) for t in sub)


def test_pair_medians():
    """The float32 mean of the two middle values; NDWI = 0 - GNDVI (so a zero median of GNDVI gives +0.0 for NDWI)."""
    rng = np.random.default_rng(0)
    pairs = rng.uniform(-1, 1, (6, 2, 2)).astype(np.float32)
    pairs[0] = 0.0
    pairs[1, 1] = (-0.0, 0.0)
    pairs[2, 0] = (np.nan, 0.5)
    med = batch.pair_medians(pairs, ("NDVI", "NDWI"))
    mid = ((pairs[:, :, 0] + pairs[:, :, 1]) / np.float32(2)).astype(np.float32)
    assert med.dtype == np.float64 and med.shape == (6, 3)
    np.testing.assert_array_equal(med[:, 0], mid[:, 0].astype(np.float64))
    assert np.isnan(med[:, 1]).all()
    assert (np.float32(0) - mid[:, 1]).astype(np.float64).tobytes() == med[:, 2].tobytes()
    assert not np.signbit(med[:2, 2]).any()
    per_index = rng.uniform(-1, 1, (3, 5, 2)).astype(np.float32)
    med = batch.pair_medians(per_index, ("GNDVI", "NDWI"), per_index=True)
    assert np.isnan(med[:, 0]).all()
    for k in (1, 2):
        np.testing.assert_array_equal(med[:, k], ((per_index[k, :, 0] + per_index[k, :, 1]) / np.float32(2)).astype(np.float64))
    values = pairs[3]
    assert batch.medians_from_pairs(values) == batch.medians_from_pairs(values, TYPES)
    got = batch.medians_from_pairs(values)
    assert got["NDVI"] == float(mid[3, 0]) and got["GNDVI"] == float(mid[3, 1]) and got["NDWI"] == float(np.float32(0) - mid[3, 1])
