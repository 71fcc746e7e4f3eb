"""The definition of "zones from polygons" (include/lars_hip.h) for the tests: once in NumPy float64, once in exact
rational arithmetic.

Pixel (row i, column j) has the centre cx = j + 0.5, cy = i + 0.5.  A polygon is the pool of the edges of its rings (closed
implicitly).  An edge with y0 == y1 crosses no row; otherwise (xa, ya) is its end with the smaller y, (xb, yb) the other, it crosses
row i iff ya <= cy < yb, at xc = xa + ((cy - ya) * (xb - xa)) / (yb - ya), each operation rounded once.  The pixel is inside iff the
number of crossings of its row with xc <= cx is odd.  Polygon k writes k + 1, later polygons over earlier ones, 0 = in none."""
from fractions import Fraction

import numpy as np

DENSE_CELLS = 1 << 22              # rows x edges x columns up to which inside_mask compares every crossing with every column at once


def rings_of(polygon):
    """A polygon as the calls take it -> its list of [n, 2] float64 rings."""
    try:
        a = np.asarray(polygon, dtype=np.float64)
    except ValueError:
        a = None
    if a is not None and a.ndim == 2:
        return [a]
    return [np.asarray(r, dtype=np.float64) for r in polygon]


def edges_of(polygon):
    """(xa, ya, xb, yb): the pooled edges that can cross a row, their ends ordered by y."""
    x0, y0, x1, y1 = [], [], [], []
    for ring in rings_of(polygon):
        nxt = np.roll(ring, -1, axis=0)
        x0.append(ring[:, 0]); y0.append(ring[:, 1]); x1.append(nxt[:, 0]); y1.append(nxt[:, 1])
    x0, y0, x1, y1 = (np.concatenate(v) for v in (x0, y0, x1, y1))
    keep = y0 != y1
    x0, y0, x1, y1 = x0[keep], y0[keep], x1[keep], y1[keep]
    up = y0 < y1
    return np.where(up, x0, x1), np.where(up, y0, y1), np.where(up, x1, x0), np.where(up, y1, y0)


def inside_mask(polygon, shape, dense=None):
    """[H, W] bool: the pixels inside one polygon.  ``dense``: force one of the two evaluation orders (the tests compare them)."""
    h, w = shape
    mask = np.zeros((h, w), dtype=bool)
    xa, ya, xb, yb = edges_of(polygon)
    if xa.size == 0:
        return mask
    i0 = int(min(max(np.floor(ya.min()) - 1, 0), h))
    i1 = int(min(max(np.floor(yb.max()) + 2, 0), h))
    if i1 <= i0:
        return mask
    cx = np.arange(w, dtype=np.float64) + 0.5
    if dense is None:
        dense = (i1 - i0) * xa.size * w <= DENSE_CELLS
    if dense:
        cy = (np.arange(i0, i1, dtype=np.float64) + 0.5)[:, None]
        cross = (ya <= cy) & (cy < yb)
        with np.errstate(all="ignore"):
            xc = xa + ((cy - ya) * (xb - xa)) / (yb - ya)
        left = cross[:, :, None] & (xc[:, :, None] <= cx)
        mask[i0:i1] = (left.sum(axis=1) & 1).astype(bool)
        return mask
    for i in range(i0, i1):
        cy = i + 0.5
        m = (ya <= cy) & (cy < yb)
        if not m.any():
            continue
        xc = xa[m] + ((cy - ya[m]) * (xb[m] - xa[m])) / (yb[m] - ya[m])
        xc.sort()
        mask[i] = (np.searchsorted(xc, cx, side="right") & 1).astype(bool)
    return mask


def label_dtype(npolys):
    return np.uint8 if npolys <= 255 else np.uint16


def labels(polygons, shape, dense=None):
    """The [H, W] label raster of a list of polygons: what ``rasterize_zones(polygons, shape)`` must return, byte for byte."""
    out = np.zeros(shape, dtype=label_dtype(len(polygons)))
    for k, polygon in enumerate(polygons):
        out[inside_mask(polygon, shape, dense)] = k + 1
    return out


# ---------------------------------------------------------------------------
# the same rule without rounding
# ---------------------------------------------------------------------------
def inside_mask_exact(polygon, shape):
    """``inside_mask`` in ``fractions.Fraction``: the geometric rule.  For vertices that are multiples of 1/8 of moderate size the
    float64 rule equals it: differences and the product are exact, the quotient and the sum round once each, and an exact crossing
    that is not a pixel centre is a rational with a small denominator, hence many ulps away from every centre."""
    h, w = shape
    mask = np.zeros((h, w), dtype=bool)
    edges = []
    for ring in rings_of(polygon):
        pts = [(Fraction(float(x)), Fraction(float(y))) for x, y in ring]
        for (x0, y0), (x1, y1) in zip(pts, pts[1:] + pts[:1]):
            if y0 != y1:
                edges.append((x0, y0, x1, y1) if y0 < y1 else (x1, y1, x0, y0))
    for i in range(h):
        cy = Fraction(2 * i + 1, 2)
        xs = [xa + (cy - ya) * (xb - xa) / (yb - ya) for xa, ya, xb, yb in edges if ya <= cy < yb]
        if not xs:
            continue
        for j in range(w):
            cx = Fraction(2 * j + 1, 2)
            mask[i, j] = sum(1 for x in xs if x <= cx) & 1
    return mask


def labels_exact(polygons, shape):
    out = np.zeros(shape, dtype=label_dtype(len(polygons)))
    for k, polygon in enumerate(polygons):
        out[inside_mask_exact(polygon, shape)] = k + 1
    return out

