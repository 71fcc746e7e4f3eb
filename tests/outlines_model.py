"""The definition of region_outlines (DESIGN.md "Region outlines", include/lars_hip.h "region outlines") in NumPy / Python: the oracle of
test_outlines_cpu.py and test_gpu_outlines.py, as regions_model.py is for the labels.

``labels[h][w]``: 0 = background, 1 .. R = regions, each one connected set under ``connectivity``.  Vertices are pixel corners: corner
(r, c) is the upper-left corner of pixel (r, c).  A pixel (y, x) of label L owns one directed edge per side whose neighbour is not L
(outside the raster counts as not L), clockwise on the screen:

    side 0, top     (y, x)         -> (y, x + 1)      east
    side 1, right   (y, x + 1)     -> (y + 1, x + 1)  south
    side 2, bottom  (y + 1, x + 1) -> (y + 1, x)      west
    side 3, left    (y + 1, x)     -> (y, x)          north

with the id 4 * (y * w + x) + side.  The successor of an edge is the first that exists of: the right turn (the next side of the same
pixel), straight on (the same side of the next pixel along the edge), the left turn (the previous side of the pixel diagonally ahead on
the outer side) -- in this order under connectivity 4, in the opposite order under 8.  Rings are the cycles of the successor; a ring's
key is its smallest edge id, its vertices the start corners of the edges whose predecessor has another side, from the first such edge
at or after the smallest edge.  Rings are sorted by (label, key)."""
import numpy as np

DY = (0, 1, 0, -1)                      # the direction of side s: east, south, west, north
DX = (1, 0, -1, 0)
START = ((0, 0), (0, 1), (1, 1), (1, 0))                              # the start corner of side s, from the pixel's own corner


def edges_of(labels):
    """The sorted edge ids of a label raster."""
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = lab
    flat = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ids = []
    for s in range(4):
        oy, ox = DY[(s + 3) % 4], DX[(s + 3) % 4]                     # the outer side of side s
        other = pad[1 + oy:1 + oy + h, 1 + ox:1 + ox + w]
        ids.append(4 * flat[(lab > 0) & (other != lab)] + s)
    return np.sort(np.concatenate(ids))


def successor(lab, e, edge_set, connectivity):
    h, w = lab.shape
    p, s = divmod(int(e), 4)
    y, x = divmod(p, w)
    oy, ox = DY[(s + 3) % 4], DX[(s + 3) % 4]
    right = 4 * p + (s + 1) % 4
    ay, ax = y + DY[s], x + DX[s]
    straight = 4 * (ay * w + ax) + s if 0 <= ay < h and 0 <= ax < w else -1
    by, bx = ay + oy, ax + ox
    left = 4 * (by * w + bx) + (s + 3) % 4 if 0 <= by < h and 0 <= bx < w else -1
    label = lab[y, x]

    def exists(f):
        return f >= 0 and f in edge_set and lab[divmod(f // 4, w)] == label
    order = (right, straight, left) if connectivity == 4 else (left, straight, right)
    found = [f for f in order if exists(f)]
    assert found, "an edge without a successor"
    return found[0]


def start_corner(e, w):
    p, s = divmod(int(e), 4)
    y, x = divmod(p, w)
    return y + START[s][0], x + START[s][1]


def trace(labels, connectivity=8):
    """-> {"verts": int32 [V, 2] (row, col), "ring_label", "ring_key", "ring_start", "ring_count": int32 [Q], "ring_area2": int64 [Q],
    "n_rings": Q, "n_vertices": V, "n_edges": E}, the rings sorted by (label, key)."""
    assert connectivity in (4, 8)
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    assert h * w < 1 << 29
    edges = edges_of(lab).tolist()
    edge_set = set(edges)
    succ = {e: successor(lab, e, edge_set, connectivity) for e in edges}
    pred = {f: e for e, f in succ.items()}
    assert len(pred) == len(succ), "two edges share a successor"
    rings, seen = [], set()
    for key in edges:                                                 # ascending: the first edge met of a ring is its smallest
        if key in seen:
            continue
        ring, e = [], key
        while e not in seen:
            seen.add(e)
            ring.append(e)
            e = succ[e]
        assert e == key
        corners = [start_corner(f, w) for f in ring if pred[f] % 4 != f % 4]
        n = len(corners)
        area2 = sum(corners[i][1] * corners[(i + 1) % n][0] - corners[(i + 1) % n][1] * corners[i][0] for i in range(n))
        rings.append((int(lab[divmod(key // 4, w)]), key, corners, area2))
    rings.sort(key=lambda r: (r[0], r[1]))
    starts = np.cumsum([0] + [len(r[2]) for r in rings])
    verts = np.array([c for r in rings for c in r[2]], dtype=np.int32).reshape(-1, 2)
    return {"verts": verts, "ring_label": np.array([r[0] for r in rings], dtype=np.int32),
            "ring_key": np.array([r[1] for r in rings], dtype=np.int32), "ring_start": starts[:-1].astype(np.int32),
            "ring_count": np.diff(starts).astype(np.int32), "ring_area2": np.array([r[3] for r in rings], dtype=np.int64),
            "n_rings": len(rings), "n_vertices": len(verts), "n_edges": len(edges)}


def trace_staged(labels, connectivity=8):
    """``trace``'s result by the stages of csrc/outlines.hip, in NumPy: edges compacted in id order, predecessors from the labels alone
    (a = the pixel behind the start is L, b = the one diagonally behind on the outer side is L), pointer doubling over (smallest index,
    steps back to it), rings numbered at their smallest edge, ordered by label with a stable sort, edges scattered to ring order, the
    vertex flags scanned."""
    assert connectivity in (4, 8)
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.int64)
    pad[1:-1, 1:-1] = lab

    def at(y, x):
        return pad[y + 1, x + 1]
    eid = edges_of(lab)
    n = len(eid)
    empty = np.zeros(0, dtype=np.int32)
    if n == 0:
        return {"verts": empty.reshape(0, 2), "ring_label": empty, "ring_key": empty, "ring_start": empty, "ring_count": empty,
                "ring_area2": np.zeros(0, dtype=np.int64), "n_rings": 0, "n_vertices": 0, "n_edges": 0}
    index_of = {int(e): i for i, e in enumerate(eid)}                 # the kernel: pixoff[pixel] + the pixel's sides below this one
    s = eid % 4
    y, x = np.divmod(eid // 4, w)
    L = lab[y, x]
    dy, dx = np.array(DY)[s], np.array(DX)[s]
    oy, ox = np.array(DY)[(s + 3) % 4], np.array(DX)[(s + 3) % 4]
    by, bx = y - dy, x - dx
    a, b = at(by, bx) == L, at(by + oy, bx + ox) == L
    corner = ~(a & ~b)
    left = b if connectivity == 8 else a & b
    straight = a & ~b
    py = np.where(left, by + oy, np.where(straight, by, y))
    px = np.where(left, bx + ox, np.where(straight, bx, x))
    ps = np.where(left, (s + 1) % 4, np.where(straight, s, (s + 3) % 4))
    jump = np.array([index_of[int(e)] for e in 4 * (py * w + px) + ps], dtype=np.int64)
    low, off = np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    reach = 1
    while reach < n:                                                  # ceil(log2(n)) rounds
        take = low[jump] < low
        low, off, jump = np.where(take, low[jump], low), np.where(take, off[jump] + reach, off), jump[jump]
        reach *= 2
    heads = np.flatnonzero(low == np.arange(n))                       # in key order
    ringno = np.full(n, -1, dtype=np.int64)
    ringno[heads] = np.arange(len(heads))
    rlabel = L[heads]
    rlen = np.bincount(ringno[low], minlength=len(heads))
    order = np.argsort(rlabel, kind="stable")                         # by (label, key)
    ebase = np.zeros(len(heads), dtype=np.int64)
    ebase[order] = np.cumsum(rlen[order]) - rlen[order]
    spos = np.empty(len(heads), dtype=np.int64)
    spos[order] = np.arange(len(heads))
    slot = ebase[ringno[low]] + off
    assert sorted(slot.tolist()) == list(range(n))
    ring_order = np.empty(n, dtype=np.int64)
    ring_order[slot] = np.arange(n)
    is_vertex = corner[ring_order]
    vidx = np.cumsum(is_vertex) - is_vertex
    rows, cols = y + np.array(START)[s, 0], x + np.array(START)[s, 1]
    verts = np.stack((rows[ring_order][is_vertex], cols[ring_order][is_vertex]), axis=-1).astype(np.int32)
    term = np.where(s == 0, -y, np.where(s == 1, x + 1, np.where(s == 2, y + 1, -x)))
    area2 = np.zeros(len(heads), dtype=np.int64)
    np.add.at(area2, spos[ringno[low]], term)
    start = vidx[ebase[order]]
    end = np.append(start[1:], is_vertex.sum())
    return {"verts": verts, "ring_label": rlabel[order].astype(np.int32), "ring_key": eid[heads][order].astype(np.int32),
            "ring_start": start.astype(np.int32), "ring_count": (end - start).astype(np.int32), "ring_area2": area2,
            "n_rings": len(heads), "n_vertices": len(verts), "n_edges": n}


def same(one, other):
    """Do two traces agree in every field, bit for bit?"""
    return all(np.array_equal(one[k], other[k]) and np.asarray(one[k]).dtype == np.asarray(other[k]).dtype for k in one) and set(one) == set(other)


def polygons(traced, n_regions):
    """The rings as ``Polygons`` holds them: (verts float64 [V, 2] as (x, y) = (col, row), ring_starts int32 [Q + 1], poly_starts int32
    [R + 1]); polygon k - 1 is region k."""
    verts = traced["verts"][:, ::-1].astype(np.float64)
    ring_starts = np.concatenate((traced["ring_start"], [traced["n_vertices"]])).astype(np.int32)
    poly_starts = np.searchsorted(traced["ring_label"], np.arange(1, n_regions + 2)).astype(np.int32)
    return np.ascontiguousarray(verts), ring_starts, poly_starts


def polygon_list(traced, n_regions):
    """One list of [n, 2] float64 (x, y) rings per region, as ``rasterize_zones`` / ``zone_raster_model.labels`` take them."""
    verts, ring_starts, poly_starts = polygons(traced, n_regions)
    return [[verts[ring_starts[r]:ring_starts[r + 1]] for r in range(poly_starts[k], poly_starts[k + 1])] for k in range(n_regions)]
