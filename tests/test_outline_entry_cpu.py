"""The label rasters of outline_label_cases.py without a device: the model of the definition (outlines_model.py) agrees with its own
walk through the stages of csrc/outlines.hip on labels no labeller writes, and every case has the counts it was built for -- on and
next to the chunks, segments and rounds of the kernels -- so that test_gpu_outline_entry.py relies on nothing that is only assumed."""
import numpy as np
import pytest

import outline_label_cases as lc
import outlines_model as om

ALL = sorted(lc.cases()) + sorted(lc.understated_cases())


def pixels_of(labels):
    """{label: pixels} of the labels above 0."""
    values, counts = np.unique(labels[labels > 0], return_counts=True)
    return dict(zip(values.tolist(), counts.tolist()))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ALL)
def test_the_model_and_its_staged_walk_agree_and_the_facts_hold(name, connectivity):
    c = lc.find(name)
    labels, facts = lc.positive(c["labels"]), c["facts"]
    traced = lc.model_trace("scattered" if name.startswith("understated_") else name, connectivity)
    assert om.same(traced, om.trace_staged(labels, connectivity))
    assert traced["n_edges"] == len(om.edges_of(labels)) and traced["n_vertices"] == int(traced["ring_count"].sum()) == len(traced["verts"])
    order = np.lexsort((traced["ring_key"], traced["ring_label"]))    # sorted by (label, key)
    assert np.array_equal(order, np.arange(traced["n_rings"])) and len(set(traced["ring_key"].tolist())) == traced["n_rings"]
    pixels = pixels_of(labels)
    assert sorted(pixels) == sorted(set(traced["ring_label"].tolist())) and len(pixels) == facts["distinct"]
    for label, n in pixels.items():                                   # a label's rings, holes included, enclose its pixels
        assert int(traced["ring_area2"][traced["ring_label"] == label].sum()) == 2 * n, label
    for key, have in (("rings", traced["n_rings"]), ("edges", traced["n_edges"]), ("vertices", traced["n_vertices"]), ("pixels", sum(pixels.values()))):
        if key in facts:
            assert have == facts[key], (key, have, facts[key])
    assert traced["n_rings"] >= facts.get("min_rings", 0)
    assert om.same(lc.reordered(traced, 4), traced)
    assert c["passes"] == lc.passes_of(c["n_labels"]) and 0 <= c["n_labels"] <= lc.TOP
    assert c["labels"].dtype == np.int32 and (c["labels"].size <= 10 ** 4 or c["labels"].shape[0] == 2 and c["labels"].shape[1] <= 8194)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_scattered_has_every_value_and_rings_of_one_label_in_three_sort_chunks(connectivity):
    c = lc.cases()["scattered"]
    assert c["labels"].shape == (70, 130) and c["n_labels"] == lc.TOP and c["passes"] == 4
    assert set(np.unique(c["labels"]).tolist()) == set(lc.VALUES) and 0.17 < (c["labels"] == 0).mean() < 0.23
    traced = lc.model_trace("scattered", connectivity)
    assert traced["n_rings"] > 2 * lc.CHUNK                           # three sort chunks or more
    chunk_of = np.argsort(np.argsort(traced["ring_key"])) // lc.CHUNK   # where the sort finds a ring: its number in key order
    for label in (v for v in lc.VALUES if v > 0):                     # every label has rings in every chunk: equal keys far apart
        mine = chunk_of[traced["ring_label"] == label]
        assert len(set(mine.tolist())) >= c["facts"]["spread_chunks"] and len(mine) > 64, label
    assert (traced["ring_area2"] < 0).any() and traced["ring_count"].max() > 4          # holes, and rings that are no single pixel
    assert set((traced["ring_label"].astype(np.int64) >> 24).tolist()) >= {0, 1, 0x7F}  # the fourth pass has something to order


def test_the_strips_stand_on_and_next_to_the_chunk_edges():
    rings = sorted({q for q, d in lc.STRIPS if d == 0} & {2047, 2048, 2049, 4096, 4097})
    assert rings == [lc.CHUNK - 1, lc.CHUNK, lc.CHUNK + 1, 2 * lc.CHUNK, 2 * lc.CHUNK + 1]
    assert {4 * q + 2 * d for q, d in lc.STRIPS} >= set(lc.STRIP_EDGES)
    assert lc.STRIP_EDGES == (1022, 1024, 1026, 2046, 2048, 2050, 4096)
    assert {q // lc.ROUND * lc.ROUND - q for q, d in lc.STRIPS} >= {0, -1}           # a ring count on a sort round and one past it
    assert max(c["labels"].shape[1] for c in lc.cases().values()) == 8194
    assert sorted(h * w for h, w in lc.BLOCKS) == [2047, 2048, 2049]
    for rule, passes, distinct in (("descending", 2, 4097), ("repeated", 1, 251), ("low_byte", 2, 7)):
        c = lc.cases()[f"strip_4097_0_{rule}"]
        assert (c["passes"], c["facts"]["distinct"]) == (passes, distinct)
        values = c["labels"][0, ::2]
        assert values.tolist() == [lc.LABEL_RULES[rule](4097, k) for k in range(4097)]
    low = lc.cases()["strip_4097_0_low_byte"]["labels"][0, ::2]
    assert set((low & 255).tolist()) == {3}                           # the first pass moves nothing, the second everything
    assert lc.cases()["stripes_1_16777217"]["passes"] == 4 and lc.cases()["stripes_1_2"]["passes"] == 1
    domino = lc.cases()["strip_255_2_repeated"]["labels"]
    assert domino.shape == (2, 2 * 253 + 3 * 2) and not domino[1].any() and domino[0, -3] == domino[0, -2] != 0 and domino[0, -1] == 0


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(lc.understated_cases()))
def test_understated_n_labels_order_by_the_low_bytes(name, connectivity):
    c = lc.understated_cases()[name]
    assert c["passes"] == {0: 1, 255: 1, 256: 2, 65535: 2}[c["n_labels"]]
    traced, want = lc.model_trace("scattered", connectivity), lc.expected(name, connectivity)
    mask = (1 << (8 * c["passes"])) - 1
    low = want["ring_label"].astype(np.int64) & mask
    assert np.array_equal(np.lexsort((want["ring_key"], low)), np.arange(want["n_rings"]))     # sorted by (low bytes, key)
    assert not np.array_equal(want["ring_label"], traced["ring_label"]) and (np.diff(want["ring_label"].astype(np.int64)) < 0).any()
    by_key = {int(k): i for i, k in enumerate(traced["ring_key"])}    # every ring is there once, with its own row and vertices
    assert sorted(want["ring_key"].tolist()) == sorted(by_key) and all(want[k] == traced[k] for k in lc.COUNTS)
    assert np.array_equal(want["ring_start"], np.cumsum(want["ring_count"]) - want["ring_count"]) and want["ring_start"].dtype == np.int32
    for i in list(range(0, want["n_rings"], 97)) + [want["n_rings"] - 1]:
        j = by_key[int(want["ring_key"][i])]
        assert (want["ring_label"][i], want["ring_area2"][i], want["ring_count"][i]) == (traced["ring_label"][j], traced["ring_area2"][j], traced["ring_count"][j])
        assert np.array_equal(want["verts"][want["ring_start"][i]:][:want["ring_count"][i]], traced["verts"][traced["ring_start"][j]:][:traced["ring_count"][j]])
    for k in lc.FIELDS:
        assert want[k].dtype == traced[k].dtype and want[k].shape == traced[k].shape


def test_scratch_for_no_edge_room_is_the_pixels_and_a_little():
    """edge_capacity 0 is a legal room, not an argument outside the rules: 4 bytes a pixel, and the arrays that hold one ring."""
    from lars_image_processing_amd import _ffi
    lib = _ffi.load()
    for h, w in ((70, 130), (5, 7), (2, 8194)):
        assert 4 * h * w <= lib.lars_region_outline_scratch_bytes(h, w, 0) < 4 * h * w + 14 * 256, (h, w)
        assert lib.lars_region_outline_scratch_bytes(h, w, 4 * h * w) > 35 * 4 * h * w and lib.lars_region_outline_scratch_bytes(h, w, 4 * h * w + 1) == 0


def test_background_has_no_edge():
    c = lc.background()
    assert c["labels"].shape == (5, 7) and (c["labels"] <= 0).all() and (c["labels"] < 0).sum() > 10 and (c["labels"] == 0).sum() > 10
    for connectivity in (4, 8):
        traced = om.trace(lc.positive(c["labels"]), connectivity)
        assert (traced["n_edges"], traced["n_rings"], traced["n_vertices"]) == (0, 0, 0)
        assert om.same(traced, om.trace_staged(lc.positive(c["labels"]), connectivity))
