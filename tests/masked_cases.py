"""Pictures and masks of the nodata-aware tests (test_masked_cpu.py, test_gpu_masked.py): the smallest shapes at which the
kernels of csrc/masked.hip can go wrong.  A lane takes four pixels, a wave 256, a workgroup 1024; the pixels after the last
whole group of four take a path of their own."""
import numpy as np

SHAPES = [(1, 1, 3), (1, 67, 3), (3, 5, 3), (37, 53, 3), (64, 64, 3), (257, 255, 3), (300, 517, 4)]
MASKS = ["all", "one_first", "one_last", "one_middle", "two", "one_invalid", "last_partial_wave", "checkerboard", "frame",
         "random_1", "random_50", "random_99", "runs_64", "runs_256"]


def image(h, w, c, dtype=np.uint8, seed=7):
    """A vegetation-like picture: NIR bright, red dark, a gradient so that the percentiles sit inside the range."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    top = 255 if np.dtype(dtype) == np.uint8 else 65535
    y, x = np.mgrid[0:h, 0:w]
    ramp = (x + 2 * y) / max(1, (w - 1) + 2 * (h - 1))
    img = np.empty((h, w, c), dtype=np.float64)
    img[:, :, 0] = 0.10 + 0.30 * ramp + 0.10 * rng.random((h, w))
    img[:, :, 1] = 0.20 + 0.40 * rng.random((h, w))
    img[:, :, 2] = 0.40 + 0.50 * (1 - ramp) * rng.random((h, w))
    for k in range(3, c):
        img[:, :, k] = rng.random((h, w))
    return np.ascontiguousarray((img * top).astype(dtype))


def mask(name, h, w, seed=11):
    """The boolean [h, w] mask ``name``, or None where the raster is too small for it (fewer pixels than it names)."""
    n = h * w
    flat = np.zeros(n, dtype=bool)
    i = np.arange(n)
    if name == "all":
        flat[:] = True
    elif name == "one_first":
        flat[0] = True
    elif name == "one_last":
        flat[-1] = True
    elif name == "one_middle":
        flat[n // 2] = True
    elif name == "two":
        if n < 2:
            return None
        flat[[n // 3, n - 1 - n // 5]] = True
        if flat.sum() != 2:
            return None
    elif name == "one_invalid":
        if n < 2:
            return None
        flat[:] = True
        flat[(2 * n) // 3] = False
    elif name == "last_partial_wave":          # the pixels after the last full run of 64
        flat[((n - 1) // 64) * 64:] = True
    elif name == "checkerboard":
        y, x = np.mgrid[0:h, 0:w]
        flat = ((x + y) % 2 == 0).reshape(-1)
    elif name == "frame":                      # a border that holds a quarter of the raster (the inside keeps sqrt(3/4) of each side)
        by, bx = int(round(h * (1 - 0.75 ** 0.5) / 2)), int(round(w * (1 - 0.75 ** 0.5) / 2))
        m = np.zeros((h, w), dtype=bool)
        m[by:h - by, bx:w - bx] = True
        flat = m.reshape(-1)
    elif name.startswith("random_"):
        p = int(name.split("_")[1]) / 100
        flat = np.random.default_rng(seed + n).random(n) < p
        flat[n // 2] = True                    # never empty
    elif name.startswith("runs_"):             # runs that start half a run before a multiple of their length
        r = int(name.split("_")[1])
        flat = ((i + r // 2) // r) % 2 == 0
    else:
        raise KeyError(name)
    if not flat.any():
        return None
    return flat.reshape(h, w)


def shape_mask_cases():
    return [(s, m) for s in SHAPES for m in MASKS if mask(m, s[0], s[1]) is not None]


def framed_picture(h=37, w=53, c=3, dtype=np.uint8):
    """A bright picture inside a black frame: np.percentile over the whole rectangle sees the frame (p2 == 0), over the valid
    pixels it does not.  Returns (image, valid)."""
    img = image(h, w, c, dtype)
    top = 255 if np.dtype(dtype) == np.uint8 else 65535
    img[:, :, :3] = (top * 0.4 + img[:, :, :3] * 0.5).astype(dtype)      # nothing inside is black
    valid = mask("frame", h, w)
    img[~valid] = 0
    return img, valid
