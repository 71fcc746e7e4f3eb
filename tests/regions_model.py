"""The definition of label_regions (include/lars_hip.h "zones from regions") in NumPy / Python, and a second function that walks
through the stages of csrc/regions.hip for a given tile shape, so that the algorithm is checked on the CPU before any device runs it.

``label`` works on the runs of foreground pixels of each row: runs of neighbouring rows that touch (connectivity 4: share a column;
8: share a column or are one column apart) are joined in a union-find whose root is the earlier run, so roots come out in raster
order of the regions' first pixels.  ``label_staged`` is per pixel and slow: tile-local unions, seam unions, flatten, areas, the
scan of the flags, the relabelling and the table, with the kernels' own job lists and compare-and-retry unions."""
import numpy as np

REGION_FIELDS = ("area", "bbox", "row_sum", "col_sum")


def _table(labels, n):
    """area int64 [n], bbox int32 [n, 4] (row0, col0, row1, col1; half-open), row_sum / col_sum uint64 [n] of labels 1 .. n."""
    h, w = labels.shape
    flat = labels.ravel().astype(np.int64)
    inside = flat > 0
    ids = flat[inside] - 1
    rows, cols = np.divmod(np.flatnonzero(inside), w)
    area = np.bincount(ids, minlength=n).astype(np.int64)
    bbox = np.empty((n, 4), dtype=np.int64)
    bbox[:, :2] = max(h, w)
    bbox[:, 2:] = -1
    np.minimum.at(bbox[:, 0], ids, rows)
    np.minimum.at(bbox[:, 1], ids, cols)
    np.maximum.at(bbox[:, 2], ids, rows)
    np.maximum.at(bbox[:, 3], ids, cols)
    bbox[:, 2:] += 1
    row_sum = np.zeros(n, dtype=np.uint64)
    col_sum = np.zeros(n, dtype=np.uint64)
    np.add.at(row_sum, ids, rows.astype(np.uint64))
    np.add.at(col_sum, ids, cols.astype(np.uint64))
    return {"area": area, "bbox": bbox.astype(np.int32), "row_sum": row_sum, "col_sum": col_sum}


def _drop_small(labels, n, min_pixels):
    """Regions of fewer than min_pixels pixels -> 0, the others renumbered 1 .. R in the same order."""
    area = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    keep = area >= min_pixels
    remap = np.concatenate(([0], np.cumsum(keep) * keep)).astype(np.int32)
    return remap[labels], int(keep.sum())


def _result(labels, n):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    return {"labels": labels, "n_regions": n, **_table(labels, n)}


def centroid(result):
    """float64 [R, 2] (row, column): the quotient of the exact sums, as the package takes it."""
    area = result["area"].astype(np.int64)
    return np.stack((result["row_sum"].astype(np.float64) / area, result["col_sum"].astype(np.float64) / area), axis=-1).reshape(-1, 2)


def label(mask, connectivity=8, min_pixels=1):
    """-> {"labels": int32 [h, w], "n_regions": R, "area", "bbox", "row_sum", "col_sum"} by the definition."""
    assert connectivity in (4, 8) and min_pixels >= 1
    m = np.asarray(mask) != 0
    h, w = m.shape
    # the runs of every row, in raster order: row, first column, one past the last column
    padded = np.zeros((h, w + 2), dtype=np.int8)
    padded[:, 1:-1] = m
    step = np.diff(padded, axis=1)
    rows, starts = np.nonzero(step == 1)
    ends = np.nonzero(step == -1)[1]
    nruns = len(rows)
    parent = list(range(nruns))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = np.searchsorted(rows, np.arange(h + 1))                   # the first run of each row
    reach = 1 if connectivity == 8 else 0
    s, e = starts.tolist(), ends.tolist()
    for y in range(1, h):
        a, a_end, b, b_end = first[y - 1], first[y], first[y], first[y + 1]
        while a < a_end and b < b_end:
            if s[a] < e[b] + reach and s[b] < e[a] + reach:           # the runs touch
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e[a] < e[b]:
                a += 1
            else:
                b += 1
    roots = np.array([find(i) for i in range(nruns)], dtype=np.int64)
    is_root = roots == np.arange(nruns)
    number = np.cumsum(is_root)                                        # a root's region number: roots are in raster order
    run_label = number[roots] if nruns else np.zeros(0, dtype=np.int64)
    paint = np.zeros(h * w + 1, dtype=np.int64)
    np.add.at(paint, rows * w + starts, run_label)
    np.add.at(paint, rows * w + ends, -run_label)
    labels = np.cumsum(paint)[:-1].reshape(h, w).astype(np.int32)
    labels, n = _drop_small(labels, int(is_root.sum()), min_pixels)
    return _result(labels, n)


def label_staged(mask, connectivity=8, min_pixels=1, tile=(32, 32), chunk=2048):
    """The same result by the stages of csrc/regions.hip with tiles of ``tile`` = (rows, columns) and numbering chunks of ``chunk``
    pixels."""
    assert connectivity in (4, 8) and min_pixels >= 1
    m = np.asarray(mask) != 0
    h, w = m.shape
    th, tw = tile
    npix = h * w
    conn8 = connectivity == 8

    def find(p, x):
        q = p[x]
        while 0 <= q < x:
            x, q = q, p[q]
        return x

    def union(p, a, b):                                               # compare and retry; min(p[b], a) is the kernel's atomicMin
        while True:
            a, b = find(p, a), find(p, b)
            if a == b:
                return
            if a > b:
                a, b = b, a
            old = p[b]
            p[b] = min(old, a)
            if old == b or old < 0:
                return
            b = old

    # 1. the tiles: local indices ly * tw + lx, flattened and written out as flat indices
    parent = [-1] * npix
    for ty0 in range(0, h, th):
        for tx0 in range(0, w, tw):
            lab = [-1] * (th * tw)
            for k in range(th * tw):
                ly, lx = divmod(k, tw)
                if ty0 + ly < h and tx0 + lx < w and m[ty0 + ly, tx0 + lx]:
                    lab[k] = k
            for k in range(th * tw):
                if lab[k] < 0:
                    continue
                ly, lx = divmod(k, tw)
                if lx > 0 and lab[k - 1] >= 0:
                    union(lab, k, k - 1)
                if ly > 0 and lab[k - tw] >= 0:
                    union(lab, k, k - tw)
                if conn8 and ly > 0:
                    if lx > 0 and lab[k - tw - 1] >= 0:
                        union(lab, k, k - tw - 1)
                    if lx < tw - 1 and lab[k - tw + 1] >= 0:
                        union(lab, k, k - tw + 1)
            for k in range(th * tw):
                ly, lx = divmod(k, tw)
                if ty0 + ly >= h or tx0 + lx >= w or lab[k] < 0:
                    continue
                r = find(lab, k)
                parent[(ty0 + ly) * w + tx0 + lx] = (ty0 + r // tw) * w + tx0 + r % tw

    # 2. the seams: the kernel's two job lists
    def join(a, b):
        if parent[b] >= 0:
            union(parent, a, b)

    nh, nv = ((h - 1) // th) * w, ((w - 1) // tw) * h
    for j in range(nh + nv):
        if j < nh:
            y, x = (j // w + 1) * th, j % w
            a = y * w + x
            b = a - w
            if parent[a] < 0:
                continue
            join(a, b)
            if conn8 and x > 0:
                join(a, b - 1)
            if conn8 and x + 1 < w:
                join(a, b + 1)
        else:
            k = j - nh
            x, y = (k // h + 1) * tw, k % h
            a = y * w + x
            b = a - 1
            if parent[a] < 0:
                continue
            join(a, b)
            if conn8 and y > 0:
                join(a, b - w)
            if conn8 and y + 1 < h:
                join(a, b + w)

    # 3. roots, 4. areas at the roots
    roots = [find(parent, i) if parent[i] >= 0 else -1 for i in range(npix)]
    area = [0] * npix
    for r in roots:
        if r >= 0:
            area[r] += 1

    # 5. numbering: per-chunk totals, their exclusive scan, the per-chunk scan
    flags = [1 if roots[i] == i and area[i] >= min_pixels else 0 for i in range(npix)]
    totals = [sum(flags[c:c + chunk]) for c in range(0, npix, chunk)]
    before = [sum(totals[:k]) for k in range(len(totals))]
    count = sum(totals)
    ids = [0] * npix
    table_area = [0] * count
    for k, c in enumerate(range(0, npix, chunk)):
        run = before[k]
        for i in range(c, min(npix, c + chunk)):
            if flags[i]:
                run += 1
                ids[i] = run
                table_area[run - 1] = area[i]

    # 6. labels and the table
    labels = np.array([ids[r] if r >= 0 else 0 for r in roots], dtype=np.int32).reshape(h, w)
    out = _result(labels, count)
    assert out["area"].tolist() == table_area                         # the numbering pass and the relabel pass agree on the areas
    return out
