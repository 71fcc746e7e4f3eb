"""The cases of the simplified outlines (DESIGN.md "Simplified outlines"), shared by test_outline_simplify_cpu.py and the GPU tests: masks
(all 512 of 3 x 3, 200 fuzzed ones of two kinds, the named corners) with their labels, traces and simplified rings from the models,
each computed once, and hand-built rings no tracer writes."""
import functools

import numpy as np
from scipy import ndimage

import outline_simplify_model as sm
import outlines_model as om
import regions_model as gm

TQS = (1, 8, 11, 16, 23, 48, 4064)      # the model's; the device runs 8, 16, 23 and 48
GPU_TQS = (8, 16, 23, 48)
FUZZ = 200
CHUNK = 2048                            # the largest chunk of csrc/outline_simplify.hip: OS_CHUNK, the items of a scan chunk
BATCH = 8                               # OS_BATCH: the rounds between two reads of the status
SMOOTH_SIGMA = 1.5


def all_3x3():
    """Every mask of 3 x 3 side by side, a background column between them: three pixels cannot reach across it."""
    raster = np.zeros((3, 4 * 512), dtype=bool)
    for k in range(512):
        raster[:, 4 * k:4 * k + 3] = ((k >> np.arange(9).reshape(3, 3)) & 1) != 0
    return raster


def smooth_mask(h, w, seed, sigma=SMOOTH_SIGMA):
    """Noise smoothed with a Gaussian filter and cut at its median: blobs with curved edges, which lose vertices."""
    x = ndimage.gaussian_filter(np.random.default_rng(seed).random((h, w)), sigma, mode="reflect")
    return x > np.median(x)


def fuzz_mask(seed):
    """-> (mask up to 40 x 40, "noise" or "smooth"): raw noise of a random density for even seeds, smoothed noise for odd ones."""
    rng = np.random.default_rng(1000 + seed)
    h, w = (int(v) for v in rng.integers(1, 41, 2))
    if seed % 2 == 0:
        return rng.random((h, w)) < rng.uniform(0.2, 0.8), "noise"
    return smooth_mask(max(h, 8), max(w, 8), 2000 + seed), "smooth"


def checkerboard(n=64):
    y, x = np.mgrid[0:n, 0:n]
    return (x + y) % 2 == 0


def comb(teeth=24):
    """A spine along the top and ``teeth`` teeth of growing length under it: Douglas-Peucker peels them off one or two a level."""
    mask = np.zeros((teeth + 2, 2 * teeth), dtype=bool)
    mask[0, :] = True
    for i in range(teeth):
        mask[1:i + 2, 2 * i] = True
    return mask


def serpentine(h=100, w=100):
    """Diagonal staircase stripes two pixels wide, two apart, joined at alternating ends into one path: a single region whose outer
    ring turns at every pixel."""
    y, x = np.mgrid[0:h, 0:w]
    s = x + y
    stripe, gap, pair = s % 4 < 2, s % 4 >= 2, (s // 4) % 2
    begin = (y == 0) | ((x == w - 1) & (s >= w - 1))                  # where a stripe begins: the top row, then the right column
    end = (x == 0) | ((y == h - 1) & (s >= h - 1))                    # and where it ends: the left column, then the bottom row
    return stripe | (gap & begin & (pair == 0)) | (gap & end & (pair == 1))


def blobs():
    """Several regions whose rings differ in length: their slots end in the middle of a wave."""
    mask = np.zeros((60, 90), dtype=bool)
    rng = np.random.default_rng(77)
    for k in range(11):
        cy, cx, r = 6 + 9 * (k % 6), 8 + 14 * (k // 2), 2.5 + 0.7 * k
        y, x = np.mgrid[0:60, 0:90]
        mask |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    return mask & (rng.random(mask.shape) < 0.97)


@functools.lru_cache(maxsize=None)
def named():
    return {"checkerboard": checkerboard(), "comb_24": comb(24), "serpentine": serpentine(), "blobs": blobs(), "all_3x3": all_3x3()}


@functools.lru_cache(maxsize=None)
def labelled(name, connectivity, min_pixels=1):
    """(mask, regions_model.label's dict, outlines_model.trace's dict) of a case: ``name`` a key of named(), "fuzz_<seed>" or
    "size_<h>x<w>"."""
    if name.startswith("fuzz_"):
        mask = fuzz_mask(int(name[5:]))[0]
    elif name.startswith("size_"):
        h, w = (int(v) for v in name[5:].split("x"))
        mask = smooth_mask(h, w, 31 * h + w, sigma=1.2)
    else:
        mask = named()[name]
    model = gm.label(mask, connectivity, min_pixels)
    return mask, model, om.trace(model["labels"], connectivity)


@functools.lru_cache(maxsize=None)
def simplified(name, connectivity, tq, min_pixels=1):
    """outline_simplify_model.simplify of the case's trace."""
    return sm.simplify(labelled(name, connectivity, min_pixels)[2], tq)


# ---- hand-built rings, in outlines_model.trace's layout ----
def rings_of(rings, labels=None):
    """``rings``: lists of (row, col); -> the dict outline_simplify_model.simplify takes, ring k labelled labels[k] (default k + 1)."""
    labels = list(labels) if labels is not None else list(range(1, len(rings) + 1))
    counts = [len(r) for r in rings]
    starts = np.cumsum([0] + counts)
    verts = np.array([p for r in rings for p in r], dtype=np.int32).reshape(-1, 2)
    return {"verts": verts, "ring_label": np.array(labels, dtype=np.int32), "ring_key": np.arange(len(rings), dtype=np.int32) * 4,
            "ring_start": starts[:-1].astype(np.int32), "ring_count": np.array(counts, dtype=np.int32),
            "ring_area2": np.array([sm.area2([(int(a), int(b)) for a, b in r]) for r in rings], dtype=np.int64), "n_rings": len(rings),
            "n_vertices": len(verts), "n_edges": 0}


M = sm.COORDINATE_MAX
# chords from (0, 0) and a vertex p between their ends whose 256 * cross^2 differs from tq^2 * len2 by less than 256: found by solving
# cross = c for the c next to tq * sqrt(len2) / 16.  (tq, b, p, 256 * m - tq^2 * len2)
NEAR = ((23, (32767, 9328), (339, 98), 239), (23, (32767, 19274), (9152, 5385), -181),
        (4063, (32272, 8505), (7340, 2197), 15), (4063, (32327, 5741), (31252, 5808), -154))


def near_ring(b, p):
    """(0, 0) -> p -> b -> a far corner: once the corner and b are kept, p is judged against the chord (0, 0) -> b alone."""
    corner = (0, M) if sm.area2([(0, 0), p, b, (0, M)]) != 0 else (M, 0)
    return [(0, 0), p, b, corner]


def hand_built():
    """{name: (rings, tq)}"""
    wiggle = [(0, 0)] + [(k % 2, k) for k in range(1, 40)] + [(0, 40), (30, 40), (30, 0)]          # one long edge that wiggles by a pixel
    pinch = [(0, 0), (0, 10), (10, 10), (20, 20), (20, 30), (30, 30), (30, 20), (20, 20), (10, 10), (10, 0)]      # (10, 10) and (20, 20) twice
    lobes = [(0, 0)] + [(k % 2, 3 * k) for k in range(1, 20)] + [(0, 60), (2, 60), (2, 58), (40, 30), (2, 2), (2, 0)]
    # self-crossing: dropping (19, 48) turns a doubled area of -270 into +22
    flip = [(16, 175), (22, 76), (28, 170), (15, 7), (19, 48), (23, 162), (0, 27), (24, 193)]
    cases = {
        "triangle": ([[(0, 0), (0, 9), (7, 0)]], 16),
        "triangle_thin": ([[(0, 0), (1, 300), (0, 600)]], 48),
        "square_equal_maxima": ([[(0, 0), (0, 8), (8, 8), (8, 0)], [(5, 5), (5, 25), (25, 25), (25, 5)]], 16),
        "diamond_equal_maxima": ([[(0, 10), (10, 20), (20, 10), (10, 0)], [(0, 10), (6, 14), (10, 20), (14, 14), (20, 10), (14, 6), (10, 0), (6, 6)]], 16),
        "wiggle": ([wiggle], 16),
        "pinch": ([pinch, [p[::-1] for p in pinch][::-1]], 16),
        "lobes": ([lobes], 23),
        "flip": ([flip], 48),
        "corners_of_the_limit": ([[(0, 0), (0, M), (M, M), (M, 0)], [(M, 0), (M, M), (0, M), (0, 0)], [(0, M), (M, M), (M, 0)],
                                  [(0, 0), (1, M // 2), (0, M), (M, M), (M - 1, M // 2), (M, 0)]], 4064),
        "many_small": ([[(r, c), (r, c + 1 + k % 3), (r + 1 + k % 2, c + 1 + k % 3), (r + 1 + k % 2, c)] for k, (r, c) in
                        enumerate((4 * (i // 40), 5 * (i % 40)) for i in range(300))], 8),
    }
    for tq, b, p, diff in NEAR:
        cases["near_%d_%s" % (tq, "above" if diff > 0 else "below")] = ([near_ring(b, p), near_ring(b, p)[::-1]], tq)
    return cases


@functools.lru_cache(maxsize=None)
def hand_case(name):
    """-> (the rings as a trace-layout dict, tq, the model's result)"""
    rings, tq = hand_built()[name]
    given = rings_of(rings)
    return given, tq, sm.simplify(given, tq)
