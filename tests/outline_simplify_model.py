"""The definition of simplified outlines (DESIGN.md "Simplified outlines", include/lars_hip.h "simplified outlines") in Python ints:
the oracle of test_outline_simplify_cpu.py and of the GPU tests, as outlines_model.py is for the traced rings.  No floats, no
recursion: explicit stacks.  ``simplify_levels`` states the same rings by the rounds of csrc/outline_simplify.hip, in NumPy int64.

A ring of n vertices (row, col) is the chain v[0] .. v[n] with v[n] = v[0]; v[0] is the vertex the tracer wrote first.  The tolerance
is ``tq`` sixteenths of a pixel, 1 .. 4064.  For a chord a -> b and a vertex p: ab = b - a, ap = p - a, len2 = |ab|^2.  len2 == 0:
m = |ap|^2, p is far when 256 * m > tq^2.  Otherwise dot = ap . ab; m = |ap|^2 * len2 if dot <= 0, |bp|^2 * len2 if dot >= len2, else
cross(ab, ap)^2 -- the squared distance to the segment times len2 -- and p is far when 256 * m > tq^2 * len2.  Douglas-Peucker on the
chain: both ends are kept; a stretch (a, b) with b - a >= 2 takes the k in (a, b) of the largest m, the smallest k on ties; if that
vertex is far it is kept and (a, k), (k, b) are treated the same way.  A ring whose result has fewer than 3 vertices, or a doubled area
that is 0 or of the other sign than the ring's own, stays as traced."""
import numpy as np

COORDINATE_MAX = 32767
TQ_MAX = 254 * 16


def measure(a, b, p):
    """-> (m, len2) of vertex p against the chord a -> b, Python ints."""
    abr, abc = b[0] - a[0], b[1] - a[1]
    apr, apc = p[0] - a[0], p[1] - a[1]
    len2 = abr * abr + abc * abc
    if len2 == 0:
        return apr * apr + apc * apc, 0
    dot = apr * abr + apc * abc
    if dot <= 0:
        return (apr * apr + apc * apc) * len2, len2
    if dot >= len2:
        bpr, bpc = p[0] - b[0], p[1] - b[1]
        return (bpr * bpr + bpc * bpc) * len2, len2
    cross = abr * apc - abc * apr
    return cross * cross, len2


def far(m, len2, tq):
    return m > ((tq * tq * (len2 if len2 else 1)) >> 8)


def area2(pts):
    """The shoelace sum over (x, y) = (col, row) of a closed ring of (row, col) vertices."""
    n = len(pts)
    return sum(pts[i][1] * pts[(i + 1) % n][0] - pts[(i + 1) % n][1] * pts[i][0] for i in range(n))


def kept_of(pts, tq):
    """-> (the sorted indices in 0 .. n - 1 of the vertices Douglas-Peucker keeps, before the collapse rule; the depth: the number of
    levels on which a stretch was split)."""
    n = len(pts)
    chain = list(pts) + [pts[0]]
    keep = [False] * (n + 1)
    keep[0] = keep[n] = True
    depth = 0
    stack = [(0, n, 0)]
    while stack:
        a, b, level = stack.pop()
        if b - a < 2:
            continue
        best, at, best_len2 = -1, -1, 0
        for k in range(a + 1, b):
            m, len2 = measure(chain[a], chain[b], chain[k])
            if m > best:
                best, at, best_len2 = m, k, len2
        if far(best, best_len2, tq):
            keep[at] = True
            depth = max(depth, level + 1)
            stack.append((a, at, level + 1))
            stack.append((at, b, level + 1))
    return [i for i in range(n) if keep[i]], depth


def simplify_ring(pts, tq):
    """One ring, ``pts`` a list of (row, col) int pairs -> (the vertices written, their doubled area, restored: the ring stays as
    traced, the depth)."""
    pts = [(int(r), int(c)) for r, c in pts]
    own = area2(pts)
    kept, depth = kept_of(pts, tq)
    out = [pts[i] for i in kept]
    got = area2(out)
    if len(out) < 3 or got == 0 or (got > 0) != (own > 0):
        return pts, own, True, depth
    return out, got, False, depth


def simplify(traced, tq):
    """``outlines_model.trace``'s dict (or hand-built rings in its layout) -> the same keys for the simplified rings, and
    "n_vertices_traced", "restored" (bool [Q]: the ring stays as traced) and "rounds" (the deepest ring's depth).  tq == 0: as traced."""
    assert 0 <= tq <= TQ_MAX
    verts = np.asarray(traced["verts"]).reshape(-1, 2)
    q = int(traced["n_rings"])
    out, starts, counts, areas, restored, rounds = [], [], [], [], [], 0
    for i in range(q):
        s, c = int(traced["ring_start"][i]), int(traced["ring_count"][i])
        pts = [tuple(v) for v in verts[s:s + c].tolist()]
        assert all(0 <= r <= COORDINATE_MAX and 0 <= x <= COORDINATE_MAX for r, x in pts)
        if tq == 0:
            kept, a2, back, depth = pts, int(traced["ring_area2"][i]), False, 0
        else:
            kept, a2, back, depth = simplify_ring(pts, tq)
        starts.append(len(out))
        counts.append(len(kept))
        areas.append(a2)
        restored.append(back)
        rounds = max(rounds, depth)
        out.extend(kept)
    result = dict(traced)
    result.update({"verts": np.array(out, dtype=np.int32).reshape(-1, 2), "ring_start": np.array(starts, dtype=np.int32),
                   "ring_count": np.array(counts, dtype=np.int32), "ring_area2": np.array(areas, dtype=np.int64), "n_vertices": len(out),
                   "n_vertices_traced": int(traced["n_vertices"]), "restored": np.array(restored, dtype=bool), "rounds": rounds})
    return result


def simplify_levels(traced, tq):
    """``simplify``'s result by the rounds of csrc/outline_simplify.hip, in NumPy int64: one slot per vertex and one more per ring for
    the closing copy of v[0]; every round each slot inside a stretch computes its m, the stretch (named by its left end) takes the
    largest m and then the smallest slot that holds it, and if that slot is far every slot of the stretch moves its a or b there."""
    assert 1 <= tq <= TQ_MAX
    verts = np.asarray(traced["verts"]).reshape(-1, 2).astype(np.int64)
    start, count = np.asarray(traced["ring_start"]).astype(np.int64), np.asarray(traced["ring_count"]).astype(np.int64)
    q = len(start)
    sbase = np.cumsum(count + 1) - (count + 1)
    n = int((count + 1).sum())
    ring = np.repeat(np.arange(q), count + 1)
    pos = np.arange(n) - sbase[ring]
    pt = verts[start[ring] + np.where(pos == count[ring], 0, pos)]
    r, c = pt[:, 0], pt[:, 1]
    a, b = sbase[ring].copy(), (sbase + count)[ring].copy()
    kept = (pos == 0) | (pos == count[ring])
    inside = ~kept
    rounds, tq2 = 0, tq * tq
    while inside.any():
        s = np.flatnonzero(inside)
        sa, sb = a[s], b[s]
        abr, abc, apr, apc = r[sb] - r[sa], c[sb] - c[sa], r[s] - r[sa], c[s] - c[sa]
        len2, ap2, dot = abr * abr + abc * abc, apr * apr + apc * apc, apr * abr + apc * abc
        bp2 = (r[s] - r[sb]) ** 2 + (c[s] - c[sb]) ** 2
        cross = abr * apc - abc * apr
        m = np.where(len2 == 0, ap2, np.where(dot <= 0, ap2 * len2, np.where(dot >= len2, bp2 * len2, cross * cross)))
        best_m = np.zeros(n, dtype=np.int64)
        np.maximum.at(best_m, sa, m)
        far_ = m > ((tq2 * np.where(len2 == 0, 1, len2)) >> 8)
        best_k = np.full(n, n, dtype=np.int64)
        mine = (m == best_m[sa]) & far_
        np.minimum.at(best_k, sa[mine], s[mine])
        k = best_k[sa]
        split = k < n
        if not split.any():
            break
        rounds += 1
        inside[s[~split]] = False
        hit = split & (s == k)
        kept[s[hit]] = True
        inside[s[hit]] = False
        left, right = split & (s < k), split & (s > k)
        b[s[left]] = k[left]
        a[s[right]] = k[right]
    closing = pos == count[ring]
    nxt = np.where(np.append(kept[1:], True), np.arange(n) + 1, np.append(b[1:], n))     # the next kept slot of a kept one
    live = kept & ~closing
    kc = np.bincount(ring[live], minlength=q)
    term = c[live] * r[nxt[live]] - c[nxt[live]] * r[live]
    karea = np.zeros(q, dtype=np.int64)
    np.add.at(karea, ring[live], term)
    plain = ~closing
    own = np.zeros(q, dtype=np.int64)
    np.add.at(own, ring[plain], c[plain] * r[np.arange(n)[plain] + 1] - c[np.arange(n)[plain] + 1] * r[plain])
    back = (kc < 3) | (karea == 0) | ((karea > 0) != (own > 0))
    written = plain & (back[ring] | kept)
    out_count = np.where(back, count, kc)
    result = dict(traced)
    result.update({"verts": pt[written].astype(np.int32), "ring_start": (np.cumsum(out_count) - out_count).astype(np.int32),
                   "ring_count": out_count.astype(np.int32), "ring_area2": np.where(back, own, karea).astype(np.int64),
                   "n_vertices": int(written.sum()), "n_vertices_traced": int(traced["n_vertices"]), "restored": back, "rounds": rounds})
    return result
