"""Masks of the region tests (test_regions_cpu.py, test_gpu_regions.py): the shapes at which the stages of csrc/regions.hip can go
wrong.  A workgroup labels a T x T tile on its own; what crosses a tile border is joined afterwards, so the named masks put their
joins on borders and corners, make long chains of unions, and merge early roots late."""
import numpy as np

T = 32                                  # the tile edge of csrc/regions.hip (RG_T)
DENSITIES = (0.05, 0.41, 0.5, 0.59, 0.8)                              # 0.41 / 0.59: near the percolation thresholds of 8 / 4 neighbours
MIN_PIXELS = (1, 2, 5, 50)


def spiral(h, w):
    """A one-pixel-wide spiral from the border inwards: one region, its root the first pixel, every other pixel a long way from it."""
    m = np.zeros((h, w), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or not m[yy, xx]

    while True:
        for _ in range(4):                                            # straight on while the cell after the next is free, else turn right
            if 0 <= y + dy < h and 0 <= x + dx < w and not m[y + dy, x + dx] and free(y + 2 * dy, x + 2 * dx):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = y + dy, x + dx
        m[y, x] = True


def serpentine(h, w):
    """Every other row full, joined at alternating ends: one region that passes through every tile again and again."""
    m = np.zeros((h, w), dtype=bool)
    m[::2, :] = True
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def comb(h, w):
    """Teeth two columns apart that join only in the last row: every tooth is a root until the very end."""
    m = np.zeros((h, w), dtype=bool)
    m[:, ::2] = True
    m[h - 1, :] = True
    return m


def rings(h, w):
    """A ring inside a ring (two regions, one background region between them that is no region at all), a dot in the middle."""
    m = np.zeros((h, w), dtype=bool)
    for inset in (1, 5):
        if h - 2 * inset >= 3 and w - 2 * inset >= 3:
            m[inset, inset:w - inset] = m[h - 1 - inset, inset:w - inset] = True
            m[inset:h - inset, inset] = m[inset:h - inset, w - 1 - inset] = True
    m[h // 2, w // 2] = True
    return m


def diagonal_pair(orientation, t=T):
    """Two pixels that touch only by a corner, across the corner where four tiles meet (2t x 2t raster)."""
    m = np.zeros((2 * t, 2 * t), dtype=bool)
    (y0, x0), (y1, x1) = {"nw_se": ((t - 1, t - 1), (t, t)), "ne_sw": ((t - 1, t), (t, t - 1)),
                          "n_edge": ((t - 1, 1), (t, 2)), "w_edge": ((1, t - 1), (2, t))}[orientation]
    m[y0, x0] = m[y1, x1] = True
    return m


def named(t=T):
    """{name: mask} for tiles of edge t."""
    big = (4 * t + 3, 4 * t + 5)
    y, x = np.mgrid[0:big[0], 0:big[1]]
    cases = {
        "empty": np.zeros((t + 3, 2 * t + 1), dtype=bool),
        "full": np.ones((2 * t + 1, t + 3), dtype=bool),
        "corners": np.zeros((2 * t + 1, 2 * t + 2), dtype=bool),
        "checkerboard": ((x + y) % 2 == 0)[:2 * t + 1, :2 * t + 3],
        "spiral": spiral(*big),
        "serpentine": serpentine(*big),
        "comb": comb(2 * t + 3, 3 * t + 1),
        "rings": rings(3 * t + 2, 2 * t + 5),
        "rows_on_borders": np.zeros((3 * t, 2 * t + 1), dtype=bool),
        "columns_on_borders": np.zeros((2 * t + 1, 3 * t), dtype=bool),
    }
    c = cases["corners"]
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True
    r = cases["rows_on_borders"]
    r[t - 1, ::2] = r[t, 1::2] = r[2 * t - 1, ::2] = r[2 * t, ::2] = True   # a zigzag across one border, pairs across the next
    k = cases["columns_on_borders"]
    k[::2, t - 1] = k[1::2, t] = k[::2, 2 * t - 1] = k[::2, 2 * t] = True
    for orientation in ("nw_se", "ne_sw", "n_edge", "w_edge"):
        cases["diagonal_" + orientation] = diagonal_pair(orientation, t)
    return cases


def random_mask(h, w, density, seed):
    return np.random.default_rng(seed).random((h, w)) < density


def fuzz_case(seed, most=300):
    """-> (mask, connectivity, min_pixels): a random mask of up to most x most pixels."""
    rng = np.random.default_rng(1000 + seed)
    h, w = (int(v) for v in rng.integers(1, most + 1, size=2))
    density = DENSITIES[seed % len(DENSITIES)]
    return rng.random((h, w)) < density, (4, 8)[(seed // len(DENSITIES)) % 2], int(rng.choice(MIN_PIXELS))


def lattice(n):
    """Isolated pixels, one at every other row and column, exactly n of them, on the smallest 2^k square that holds them."""
    side = 2
    while (side // 2) ** 2 < n:
        side *= 2
    m = np.zeros((side, side), dtype=bool)
    ys, xs = np.divmod(np.arange(n), side // 2)
    m[2 * ys, 2 * xs] = True
    return m


def thresholded_field(h, w, seed=3, level=0.0):
    """A smooth random field (1/f spectrum) above its level: blobs of every size, the masks the benchmark runs on."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    spectrum = (rng.standard_normal((h, w // 2 + 1)) + 1j * rng.standard_normal((h, w // 2 + 1))) / f
    spectrum[0, 0] = 0
    field = np.fft.irfft2(spectrum, s=(h, w))
    return field / np.abs(field).max() > level
