"""Named inputs for the polygon rasteriser (csrc/zone_raster.hip), chosen for where it can go wrong: a workgroup takes a band of 8 rows
and a tile of 256 words of 32 columns, a wave scans 64 words a step, a lane writes one pixel of 64, crossings are clipped to the tile,
and ties (a crossing on a pixel centre, a vertex on a row centre, a shared edge) must fall the way the definition says.

``CASES[name] = (polygons, (H, W))``; every polygon is a ring ``[(x, y), ...]`` or a list of rings."""
import numpy as np


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def star(cx, cy, r_out, r_in, points):
    """A star with ``2 * points`` vertices around (cx, cy)."""
    k = np.arange(2 * points)
    r = np.where(k % 2 == 0, r_out, r_in)
    a = k * (np.pi / points)
    return np.stack((cx + r * np.cos(a), cy + r * np.sin(a)), axis=1)


def comb(teeth, x0=1.0, pitch=1.5, width=0.75, y0=2.25, y1=6.25, y2=40.75):
    """A bar with ``teeth`` teeth below it: the rows of the teeth have ``2 * teeth`` crossings."""
    pts = [(x0, y0), (x0 + pitch * teeth, y0)]
    for t in range(teeth - 1, -1, -1):
        a, b = x0 + pitch * t, x0 + pitch * t + width
        pts += [(b, y1), (b, y2), (a, y2), (a, y1)]
    return pts


def jittered_grid(rows, cols, shape, seed=5, snap=None):
    """``rows x cols`` quads that share their vertices and tile a region larger than the raster, every other one turning the other way."""
    h, w = shape
    rng = np.random.default_rng(seed)
    ys = np.linspace(-3.0, h + 3.0, rows + 1)[:, None] + rng.uniform(-2.5, 2.5, (rows + 1, cols + 1))
    xs = np.linspace(-3.0, w + 3.0, cols + 1)[None, :] + rng.uniform(-2.5, 2.5, (rows + 1, cols + 1))
    ys[0], ys[-1], xs[:, 0], xs[:, -1] = -3.0, h + 3.0, -3.0, w + 3.0
    if snap:
        xs, ys = np.round(xs * snap) / snap, np.round(ys * snap) / snap
    quads = []
    for r in range(rows):
        for c in range(cols):
            q = [(xs[r, c], ys[r, c]), (xs[r, c + 1], ys[r, c + 1]), (xs[r + 1, c + 1], ys[r + 1, c + 1]), (xs[r + 1, c], ys[r + 1, c])]
            quads.append(q if (r + c) % 2 == 0 else q[::-1])
    return quads


def random_polygons(rng, shape, snap):
    """1 to 40 polygons of 3 to 12 vertices around the raster, some beyond its borders; ``snap``: vertices on multiples of 1/8."""
    h, w = shape
    out = []
    for _ in range(int(rng.integers(1, 41))):
        n = int(rng.integers(3, 13))
        cx, cy = rng.uniform(-4, w + 4), rng.uniform(-4, h + 4)
        size = rng.uniform(0.3, max(h, w) * 0.6)
        pts = np.stack((cx + rng.uniform(-size, size, n), cy + rng.uniform(-size, size, n)), axis=1)
        if snap:
            pts = np.round(pts * 8) / 8
        out.append(pts)
    return out


def fuzz_case(seed):
    rng = np.random.default_rng(1000 + seed)
    shape = (int(rng.integers(1, 97)), int(rng.integers(1, 97)))
    return random_polygons(rng, shape, snap=seed % 2 == 0), shape


def one_pixel_squares(n, width=256):
    """[n, 4, 2]: square k covers the centre of pixel k (row-major) and no other."""
    k = np.arange(n)
    x, y = (k % width).astype(np.float64), (k // width).astype(np.float64)
    corners = np.array([(0.25, 0.25), (0.75, 0.25), (0.75, 0.75), (0.25, 0.75)])
    return np.stack((x[:, None] + corners[:, 0], y[:, None] + corners[:, 1]), axis=2)


BIG = 1e9

CASES = {
    # shapes
    "triangle": ([[(2.3, 1.2), (40.7, 8.9), (15.2, 33.3)]], (37, 45)),
    "convex_quad": ([[(5.1, 3.3), (38.2, 6.8), (33.6, 29.4), (2.2, 22.9)]], (33, 41)),
    "concave": ([[(3.2, 2.1), (36.3, 4.4), (20.1, 14.7), (37.9, 30.2), (4.4, 28.8), (12.6, 15.3)]], (34, 40)),
    "bow_tie": ([[(2.2, 2.3), (30.6, 28.4), (30.6, 2.3), (2.2, 28.4)]], (31, 33)),
    "hole": ([[rect(3.3, 2.2, 40.4, 30.6), rect(10.1, 8.7, 25.8, 20.2)]], (33, 45)),
    "hole_same_direction": ([[rect(3.3, 2.2, 40.4, 30.6), rect(10.1, 8.7, 25.8, 20.2)[::-1]]], (33, 45)),
    "two_parts": ([[rect(2.2, 2.2, 12.7, 12.9), [(20.3, 5.5), (39.1, 9.9), (25.5, 25.2)]]], (30, 42)),
    # empty zones, next to a zone that is not
    "sliver": ([[(1.1, 5.6), (30.3, 5.7), (30.3, 5.75), (1.1, 5.65)], rect(2.2, 8.1, 9.9, 12.4)], (16, 33)),
    "zero_area": ([[(1.0, 1.0), (10.0, 10.0), (20.0, 20.0)], rect(2.2, 8.1, 9.9, 12.4), [(3.5, 3.5), (9.5, 3.5), (6.5, 3.5)]], (24, 24)),
    "outside": ([[(-50.0, -50.0), (-10.0, -50.0), (-10.0, -10.0)], rect(40.5, 2.0, 70.0, 20.0), rect(2.0, 30.2, 20.0, 50.0),
                 rect(-30.0, 3.0, -0.6, 9.0), rect(2.2, 8.1, 9.9, 12.4)], (24, 33)),
    # clipping
    "cut_left": ([[(-7.3, 4.2), (12.4, 2.1), (9.9, 18.8), (-3.1, 15.0)]], (22, 30)),
    "cut_right": ([[(20.3, 4.2), (42.4, 2.1), (39.9, 18.8), (23.1, 15.0)]], (22, 30)),
    "cut_top": ([[(4.3, -6.2), (22.4, -2.1), (19.9, 8.8), (6.1, 11.0)]], (22, 30)),
    "cut_bottom": ([[(4.3, 14.2), (22.4, 12.1), (19.9, 28.8), (6.1, 31.0)]], (22, 30)),
    "cut_corners": ([[(-5.0, -5.0), (6.2, -5.0), (-5.0, 6.7)], [(35.0, 27.0), (24.1, 27.0), (35.0, 15.2)]], (22, 30)),
    "far_vertices": ([[(-BIG, 3.3), (25.5, 17.2), (BIG, BIG)], [(12.5, -BIG), (BIG, 8.25), (-BIG, BIG)]], (40, 50)),
    "whole_raster": ([rect(-BIG, -BIG, BIG, BIG)], (33, 65)),
    "whole_raster_exactly": ([rect(0.0, 0.0, 65.0, 33.0)], (33, 65)),
    # ties
    "vertices_on_centres": ([rect(2.5, 2.5, 20.5, 15.5), [(30.5, 3.5), (36.5, 9.5), (30.5, 15.5), (24.5, 9.5)]], (20, 40)),
    "horizontal_edges_on_row_centres": ([[(3.2, 4.5), (18.8, 4.5), (18.8, 9.5), (12.1, 9.5), (12.1, 14.5), (3.2, 14.5)]], (20, 24)),
    "edges_through_centres": ([[(2.5, 2.5), (18.5, 18.5), (2.5, 18.5)], [(20.0, 1.0), (36.0, 9.0), (28.0, 25.0), (12.0, 17.0)],
                               [(1.5, 20.5), (11.5, 25.5), (1.5, 30.5)]], (32, 40)),
    "small_and_negative_crossings": ([rect(0.1, 1.2, 5.3, 4.6), rect(0.2, 5.2, 5.3, 8.6), rect(0.5, 9.2, 5.5, 12.6), rect(-0.3, 13.2, 5.3, 16.6),
                                      rect(1e-300, 17.2, 4.5, 20.6), rect(0.49999999999999994, 21.2, 3.5000000000000004, 24.6),
                                      rect(0.5000000000000001, 25.2, 3.4999999999999996, 28.6), [(0.05, 29.2), (0.24, 33.6), (6.2, 31.1)],
                                      [(-0.75, 34.2), (-0.2, 38.6), (6.2, 36.1)]], (40, 9)),
    "closed_ring": ([[(2.3, 1.2), (40.7, 8.9), (15.2, 33.3), (2.3, 1.2)], [rect(3.0, 20.0, 9.0, 30.0) + [(3.0, 20.0)]]], (37, 45)),
    # overlap: the later polygon wins
    "nested": ([rect(2.2, 2.2, 40.4, 30.6), rect(8.1, 6.7, 30.8, 24.2), rect(12.5, 10.5, 20.5, 18.5)], (33, 45)),
    "crossing": ([[(2.3, 1.2), (40.7, 8.9), (15.2, 33.3)], [(38.2, 2.2), (3.3, 20.1), (30.3, 31.9)], rect(10.0, 10.0, 25.0, 25.0)], (36, 44)),
    # large inputs
    "star_5000": ([star(150.2, 149.7, 160.0, 70.0, 2500)], (300, 300)),
    "comb_200": ([comb(200)], (44, 303)),
    "tall": ([[(5.2, -3.0), (60.1, 150.0), (8.8, 297.5)]], (300, 70)),
    # more than one tile of 8192 columns, more than one 64-word step: the parity carried into a tile, a quad across the seam
    "wide": ([[(-5.0, -2.0), (8300.5, 4.4), (4000.2, 11.0)], rect(8180.3, 1.2, 8205.7, 7.9), rect(8192.0, 8.0, 8250.0, 9.0)], (9, 8300)),
}

SIZES = (1, 31, 32, 33, 63, 64, 65, 257)


def size_case(n, axis):
    """A raster with ``n`` rows (axis 0) or columns (axis 1): a triangle beyond every border, a quad inside, a quad on the last pixel."""
    shape = (n, 67) if axis == 0 else (35, n)
    h, w = shape
    polys = [[(-3.3, -2.2), (w + 4.4, h * 0.4), (w * 0.3, h + 5.5)], rect(w * 0.2, h * 0.15, w * 0.7 + 0.9, h * 0.8 + 0.4),
             rect(w - 1.25, h - 1.25, w + 3.0, h + 3.0), rect(-2.0, -2.0, 0.75, 0.75)]
    return polys, shape
