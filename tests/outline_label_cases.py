"""Label rasters of the outline tracer's device entry (test_outline_entry_cpu.py, test_gpu_outline_entry.py): what lars_d_region_outline
takes by its contract (include/lars_hip.h "region outlines") and no labeller writes.  Labels that are not 1 .. R, not connected and not
in raster order put rings that are far apart in key order next to each other after the sort by label, run its third and fourth pass,
and leave many rings to a label; the strips and blocks put the edge, ring and pixel counts on and next to the 2048-item scan chunks
(OL_CHUNK), the 1024-edge scatter segments (OL_SEG * 64) and the 256-entry sort rounds of csrc/outlines.hip.

A case is a dict: ``labels`` (int32 [h, w]), ``n_labels`` (what the call is handed), ``passes`` (the sort passes that gives: one per
byte of n_labels, one at least) and ``facts``, the counts the case was built for, which test_outline_entry_cpu.py asserts of the model's
trace before the device tests rely on them.  ``expected(case, connectivity)`` is the model's trace, in the order ``passes`` passes leave."""
import functools

import numpy as np

import outlines_model as om

CHUNK = 2048                            # OL_CHUNK of csrc/outlines.hip: the items of a scan chunk, the rings of a sort chunk
SEGMENT = 1024                          # OL_SEG * 64: the edges a wave folds in k_ol_scatter
ROUND = 256                             # the entries of a sort round
TOP = (1 << 31) - 1
VALUES = (0, -5, 1, 2, 255, 256, 257, 65535, 65536, (1 << 24) - 1, 1 << 24, 0x01010101, 0x7F00FF00, TOP)
FIELDS = ("ring_label", "ring_key", "ring_start", "ring_count", "ring_area2", "verts")
COUNTS = ("n_edges", "n_rings", "n_vertices")


def passes_of(n_labels):
    """The passes of the ring sort: ``for (shift = 0; shift == 0 || (n_labels >> shift) != 0; shift += 8)``."""
    return max(1, (int(n_labels).bit_length() + 7) // 8)


def case(labels, n_labels, **facts):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    labels.setflags(write=False)
    return {"labels": labels, "n_labels": int(n_labels), "passes": passes_of(n_labels), "facts": facts}


def scattered_raster(h=70, w=130, seed=1):
    """Every pixel one of VALUES: 0 for a fifth of them, the others alike.  Three nests (a pixel of 1 in a ring of 256 in a ring of
    2^31 - 1) are set into it, so that there are holes and labels inside labels under connectivity 4 as well."""
    p = np.full(len(VALUES), 0.8 / (len(VALUES) - 1))
    p[0] = 0.2
    lab = np.random.default_rng(seed).choice(np.array(VALUES, dtype=np.int64), size=(h, w), p=p).astype(np.int32)
    for y, x in ((9, 11), (h // 2, w // 2), (h - 5, w - 5)):
        lab[y:y + 5, x:x + 5] = TOP
        lab[y + 1:y + 4, x + 1:x + 4] = 256
        lab[y + 2, x + 2] = 1
    return lab


def scattered(h=70, w=130, seed=1):
    return case(scattered_raster(h, w, seed), TOP, distinct=len([v for v in VALUES if v > 0]), min_rings=2 * CHUNK + 1, spread_chunks=3)


def understated(n_labels, h=70, w=130, seed=1):
    """The scattered raster with an n_labels below its labels: they sort by their low bytes only."""
    return case(scattered_raster(h, w, seed), n_labels, distinct=len([v for v in VALUES if v > 0]), min_rings=2 * CHUNK + 1)


LABEL_RULES = {
    "descending": lambda q, k: q - k,
    "repeated": lambda q, k: 1 + (97 * k) % 251,
    "low_byte": lambda q, k: 256 * (1 + k % 7) + 3,
}


def strip(q, dominoes, rule):
    """Two rows, the second empty; q isolated pieces on the first, a free column after each, the last ``dominoes`` of them two pixels
    long: q rings of four vertices, 4 * q + 2 * dominoes edges, the same under both connectivities.  Piece k has label rule(q, k)."""
    assert 0 <= dominoes <= q
    length = np.where(np.arange(q) >= q - dominoes, 2, 1)
    first = np.cumsum(length + 1) - (length + 1)
    lab = np.zeros((2, int((length + 1).sum())), dtype=np.int32)
    values = np.array([LABEL_RULES[rule](q, k) for k in range(q)], dtype=np.int32)
    lab[0, first] = values
    lab[0, first[length == 2] + 1] = values[length == 2]
    return case(lab, values.max(), rings=q, edges=4 * q + 2 * dominoes, vertices=4 * q, pixels=q + dominoes, distinct=len(set(values.tolist())))


# (q, dominoes): the ring count on and next to one and two sort chunks, then E = 4 * q + 2 * dominoes on and next to the scatter
# segment, the scan chunk and two of them
STRIPS = ((2047, 0), (2048, 0), (2049, 0), (4096, 0), (4097, 0), (255, 1), (255, 2), (256, 1), (511, 1), (512, 0), (512, 1), (1024, 0))
STRIP_EDGES = (SEGMENT - 2, SEGMENT, SEGMENT + 2, CHUNK - 2, CHUNK, CHUNK + 2, 2 * CHUNK)


def blocks(h, w):
    """One full region, with a one-pixel hole where one fits: h * w pixels of raster on and next to a scan chunk."""
    lab = np.ones((h, w), dtype=np.int32)
    hole = h >= 3 and w >= 3
    if hole:
        lab[h // 2, w // 2] = 0
    return case(lab, 1, rings=2 if hole else 1, edges=2 * (h + w) + (4 if hole else 0), vertices=8 if hole else 4, pixels=h * w - int(hole), distinct=1)


BLOCKS = ((1, 2048), (23, 89), (3, 683))


def stripes(other=2, h=40, w=66):
    """Vertical one-pixel stripes of the labels 1 and ``other`` in turn: in id order the edges of neighbouring rings alternate, so a wave
    of k_ol_scatter holds many rings at once and meets each again and again."""
    lab = np.where(np.arange(w) % 2 == 0, 1, other).astype(np.int32)[None, :].repeat(h, axis=0)
    return case(lab, max(1, other), rings=w, edges=w * (2 * h + 2), vertices=4 * w, pixels=h * w, distinct=2)


def background(h=5, w=7):
    """Zeros and labels below 0: no region."""
    lab = np.zeros((h, w), dtype=np.int32)
    lab[::2, 1::2] = -1
    lab[1, :] = -(1 << 31)
    lab[3, 2:5] = -7
    return case(lab, 4, rings=0, edges=0, vertices=0, pixels=0, distinct=0)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: case}, every case but the understated ones (``understated_cases``) and the background (``background``)."""
    out = {"scattered": scattered(), "stripes_1_2": stripes(2), "stripes_1_16777217": stripes((1 << 24) + 1)}
    for h, w in BLOCKS:
        out[f"blocks_{h}x{w}"] = blocks(h, w)
    for q, dominoes in STRIPS:
        for rule in sorted(LABEL_RULES):
            out[f"strip_{q}_{dominoes}_{rule}"] = strip(q, dominoes, rule)
    return out


UNDERSTATED = (0, 255, 256, 65535)      # the passes they give: 1, 1, 2, 2


@functools.lru_cache(maxsize=None)
def understated_cases():
    return {f"understated_{n}": understated(n) for n in UNDERSTATED}


def positive(labels):
    """What the tracer sees: a label below 0 is background."""
    return np.where(labels > 0, labels, 0).astype(np.int32)


def reordered(trace, passes):
    """``trace`` (om.trace: rings sorted by (label, key)) in the order ``passes`` sort passes leave: the rings in key order, sorted stably
    by the low 8 * passes bits of their label.  ring_* and verts are rebuilt in that order, one ring's vertices staying together; rows
    keep their full label.  Four passes: the trace itself."""
    by_key = np.argsort(trace["ring_key"], kind="stable")
    low = trace["ring_label"][by_key].astype(np.int64) & ((1 << (8 * passes)) - 1)
    order = by_key[np.argsort(low, kind="stable")]
    count = trace["ring_count"][order]
    start = (np.cumsum(count) - count).astype(np.int32)
    pieces = [trace["verts"][s:s + c] for s, c in zip(trace["ring_start"][order].tolist(), count.tolist())]
    verts = np.concatenate(pieces).astype(np.int32).reshape(-1, 2) if pieces else trace["verts"].copy()
    out = dict(trace)
    out.update(ring_label=trace["ring_label"][order], ring_key=trace["ring_key"][order], ring_start=start, ring_count=count,
               ring_area2=trace["ring_area2"][order], verts=verts)
    return out


def find(name):
    return cases()[name] if name in cases() else understated_cases()[name]


@functools.lru_cache(maxsize=None)
def model_trace(name, connectivity):
    """om.trace of a named case's labels as the tracer sees them, made once; nobody writes to it."""
    traced = om.trace(positive(find(name)["labels"]), connectivity)
    for v in traced.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return traced


@functools.lru_cache(maxsize=None)
def expected(name, connectivity):
    """What lars_d_region_outline is to write for the named case: the model's trace, in the order the case's passes leave."""
    c = find(name)
    traced = model_trace("scattered" if name.startswith("understated_") else name, connectivity)
    return traced if c["passes"] >= 4 else reordered(traced, c["passes"])
