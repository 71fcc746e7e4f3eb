"""The floating-point predictor of TIFF (Predictor 3, libtiff's fpDiff / fpAcc) in NumPy, written out byte by byte as the
specification reads, sharing nothing with tiffio's reshaped version or with the kernels.

A row of ``wc`` float32 samples (``wc = chunk_w * samples`` for a chunky row, ``chunk_w`` for a planar one; padding columns of
a tile count) is stored as ``4 * wc`` bytes: four planes of ``wc`` bytes, plane 0 the MOST significant byte of every sample and
plane 3 the least, whatever the file's byte order.  Over the whole row, for ``q >= stride``: ``stored[q] = planes[q] -
planes[q - stride]`` modulo 256, where ``stride`` is the samples per pixel of that row; the difference runs across the plane
borders.  Reading is the running sum with that stride, then sample e is bytes acc[e], acc[wc + e], acc[2 wc + e], acc[3 wc + e].
"""
import numpy as np


def bits_of(a):
    """float32 -> its uint32 patterns (uint32 stays)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32, copy=False)


def forward(rows, stride):
    """``[nrows, wc]`` float32 or uint32 patterns -> uint8 ``[nrows, 4 * wc]`` as the file stores them."""
    u = bits_of(rows)
    nrows, wc = u.shape
    planes = np.empty((nrows, 4 * wc), dtype=np.uint8)
    for p in range(4):
        planes[:, p * wc:(p + 1) * wc] = (u >> (8 * (3 - p))) & 0xFF
    stored = planes.copy()
    for q in range(stride, 4 * wc):
        stored[:, q] = (planes[:, q].astype(np.int64) - planes[:, q - stride]) & 0xFF
    return stored


def inverse(stored, stride):
    """uint8 ``[nrows, 4 * wc]`` -> uint32 patterns ``[nrows, wc]``."""
    stored = np.asarray(stored, dtype=np.uint8)
    nrows, n = stored.shape
    assert n % 4 == 0
    wc = n // 4
    acc = stored.astype(np.int64)
    for q in range(stride, n):
        acc[:, q] = (acc[:, q] + acc[:, q - stride]) & 0xFF
    out = np.zeros((nrows, wc), dtype=np.uint32)
    for p in range(4):
        out |= acc[:, p * wc:(p + 1) * wc].astype(np.uint32) << np.uint32(8 * (3 - p))
    return out


def strip_bytes(a3, y0, rows, predictor):
    """The bytes an encoder hands to LZW for rows y0 .. y0 + rows of a chunky little-endian float32 picture ``[H, W, C]``:
    the samples as they are, or with ``predictor`` the rows of forward()."""
    part = bits_of(a3[y0:y0 + rows])
    n, w, c = part.shape
    if not predictor:
        return part.astype("<u4").tobytes()
    return forward(part.reshape(n, w * c), c).tobytes()


def values(kind, shape, seed=0):
    """float32 test pictures: ``bits`` random 32-bit patterns (NaN payloads, infinities, denormals) with -0.0, +-inf and a NaN
    planted, ``smooth`` a field in [-1, 1], ``constant``."""
    rng = np.random.default_rng(seed)
    if kind == "bits":
        u = rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
        flat = u.reshape(-1)
        special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0x00000001, 0x807FFFFF, 0xFFFFFFFF, 0], dtype=np.uint32)
        flat[:min(flat.size, special.size)] = special[:flat.size]
        return u.view(np.float32)
    if kind == "smooth":
        idx = np.indices(shape).astype(np.float64)
        x = np.sin(idx[0] * 0.37 + 0.5 * seed) * np.cos(idx[1] * 0.21)
        if len(shape) == 3:
            x = x * (1.0 - 0.13 * idx[2])
        return np.clip(x, -1, 1).astype(np.float32)
    assert kind == "constant"
    return np.full(shape, np.float32(0.3125) + seed, dtype=np.float32)
