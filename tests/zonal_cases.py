"""Label rasters and planes of the zonal tests (test_zonal_cpu.py, test_gpu_zonal.py): the smallest shapes at which the kernels
of csrc/zonal.hip can go wrong.  A lane takes one pixel, a wave 64, a workgroup 256; a wave adds once per distinct label it
holds, so 1-pixel stripes are its worst case and one zone everywhere its best."""
import numpy as np

SHAPES = [(1, 1), (1, 63), (1, 65), (7, 9), (33, 65), (255, 257), (512, 512)]
LAYOUTS = ["one_zone", "all_zero", "grid8", "stripes64", "stripes65", "last3", "tiny_zones", "gaps"]


def labels(name, h, w, seed=5):
    """-> (int64 [h, w] labels, Z) of layout ``name``, or None where the raster is too small for it."""
    n = h * w
    y, x = np.mgrid[0:h, 0:w]
    if name == "one_zone":
        return np.ones((h, w), dtype=np.int64), 1
    if name == "all_zero":                     # every zone empty: no error
        return np.zeros((h, w), dtype=np.int64), 3
    if name == "grid8":                        # 8x8-pixel plots, a 2-pixel path of label 0 between them
        if h < 8 or w < 8:
            return None
        ny, nx = (h + 9) // 10, (w + 9) // 10
        z = (y // 10) * nx + (x // 10) + 1
        z[(y % 10 >= 8) | (x % 10 >= 8)] = 0
        return z.astype(np.int64), ny * nx
    if name.startswith("stripes"):             # vertical stripes 1 pixel wide: every lane of a wave holds its own label
        k = int(name[7:])
        if w < 2:
            return None
        return (x % k + 1).astype(np.int64), k
    if name == "last3":                        # labels only in the last 3 pixels
        if n < 3:
            return None
        z = np.zeros(n, dtype=np.int64)
        z[-3:] = [2, 1, 2]
        return z.reshape(h, w), 2
    if name == "tiny_zones":                   # zones of exactly 1, 2, 3 and 4 pixels (odd and even median pairs), the rest zone 5
        if n < 11:
            return None
        z = np.full(n, 5, dtype=np.int64)
        pos = np.random.default_rng(seed + n).permutation(n)[:10]
        z[pos] = [1, 2, 2, 3, 3, 3, 4, 4, 4, 4]
        return z.reshape(h, w), 5
    if name == "gaps":                         # zone 3 of 6 and the last zone never occur
        if n < 8:
            return None
        z = np.random.default_rng(seed + n).choice([0, 1, 2, 4, 5], size=n)
        z[:4] = [1, 2, 4, 5]
        return z.reshape(h, w).astype(np.int64), 6
    raise KeyError(name)


def shape_layout_cases():
    return [(s, name) for s in SHAPES for name in LAYOUTS if labels(name, *s) is not None]


def random_labels(h, w, nz, seed=9):
    return np.random.default_rng(seed).integers(0, nz + 1, size=(h, w)).astype(np.int64)


def sparse_labels(h, w, nz=65535, seed=13):
    """Z = 65535 with most zones empty: a few hundred labels spread over the range, 1 and Z among them."""
    rng = np.random.default_rng(seed)
    used = np.unique(np.concatenate([[1, nz, nz - 1, 256, 257, 32768], rng.integers(1, nz + 1, size=200)]))
    z = rng.choice(np.concatenate([[0], used]), size=(h, w))
    z.reshape(-1)[:used.size] = used
    return z.astype(np.int64)


def plane(h, w, seed=3):
    """A hand-made float32 plane: ties, signed zeros, +-1, the coverage thresholds float32(0.2) and 0, values on histogram edges,
    both signs, subnormals, and ordinary values in between."""
    rng = np.random.default_rng(seed + 31 * h + w)
    edges = np.linspace(-1, 1, 51, dtype=np.float32)
    special = np.concatenate([
        np.array([0.0, -0.0, 1.0, -1.0, 0.2, 0.0, np.nextafter(np.float32(0.2), np.float32(1)), np.nextafter(np.float32(0.2), np.float32(-1)),
                  1e-45, -1e-45, 1e-39, -1e-39, 0.5, 0.5, 0.5, -0.25, -0.25], dtype=np.float32),
        edges, np.nextafter(edges, np.float32(-2)), np.nextafter(edges, np.float32(2))]).astype(np.float32)
    special = special[(special >= -1) & (special <= 1)]
    x = rng.uniform(-1, 1, size=h * w).astype(np.float32)
    x = np.round(x * 64) / np.float32(64) if h * w > 4096 else x          # many ties on the large rasters
    pick = rng.random(h * w) < 0.4
    x[pick] = rng.choice(special, size=int(pick.sum()))
    return np.ascontiguousarray(x.reshape(h, w).astype(np.float32))


def valid_mask(h, w, seed=17):
    m = np.random.default_rng(seed + h * w).random((h, w)) < 0.7
    m.reshape(-1)[(h * w) // 2] = True
    return m


def plots_picture(h=33, w=65, c=3, dtype=np.uint8):
    """A picture for the driver and the picture-level tests (masked_cases.image) with its grid of plots."""
    import masked_cases as mc
    z, nz = labels("grid8", h, w)
    return mc.image(h, w, c, dtype), z, nz
