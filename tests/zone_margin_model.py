"""The definition of a zone margin (DESIGN.md "Zone margins") restated in NumPy, for the tests of csrc/zone_margin.hip.

Labels are ``L[H][W]``, 0 = in no zone.  For a pixel ``p`` with ``L(p) != 0``, ``D2(p)`` is the smallest ``(di)^2 + (dj)^2`` to a pixel
``q`` of the raster with ``L(q) != L(p)``; no such pixel: infinity.  With ``m2`` the shrunk labels keep ``L(p)`` iff ``D2(p) > m2``.

``d2_brute`` walks all pixel pairs (small rasters); ``d2_scipy`` takes ``scipy.ndimage.distance_transform_edt`` per label, whose
squared distances are integers below 2**53 and so exact after rounding.  ``margin2`` is the host's rule for the integer the device
sees."""
import math

import numpy as np

INF = np.iinfo(np.int64).max


def margin2(m):
    """The largest ``n`` with float64 ``sqrt(n) <= m``, found by search, not by the rule under test."""
    lo, hi = 0, 254 * 254 + 1                                    # sqrt(lo) <= m < sqrt(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if math.sqrt(mid) <= m:
            lo = mid
        else:
            hi = mid
    return lo


def d2_brute(labels):
    """``D2`` as int64 ``[H, W]`` (``INF`` where nothing differs, 0 where the label is 0), over all pixel pairs."""
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    ii, jj = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w), dtype=np.int64)
    for i in range(h):
        for j in range(w):
            if lab[i, j] == 0:
                continue
            other = lab != lab[i, j]
            out[i, j] = ((ii[other] - i) ** 2 + (jj[other] - j) ** 2).min() if other.any() else INF
    return out


def d2_scipy(labels):
    """``D2`` by one exact Euclidean distance transform per label.  A label that fills the raster is taken out first: for a mask
    without a zero scipy returns a finite distance that means nothing."""
    from scipy.ndimage import distance_transform_edt
    lab = np.asarray(labels).astype(np.int64)
    out = np.zeros(lab.shape, dtype=np.int64)
    for z in np.unique(lab):
        if z == 0:
            continue
        mask = lab == z
        if mask.all():
            out[:] = INF
            continue
        d2 = np.rint(distance_transform_edt(mask) ** 2).astype(np.int64)
        out[mask] = d2[mask]
    return out


def shrink(labels, m2, d2=None):
    """The shrunk labels, in the dtype given."""
    lab = np.asarray(labels)
    d2 = d2_scipy(lab) if d2 is None else d2
    return np.where(d2 > m2, lab, 0).astype(lab.dtype)


def fuzz_labels(rng, h, w, blocky, top=3):
    """Labels 0 .. top: pixel noise, or blocks of 1 to 6 pixels on a side."""
    if not blocky:
        return rng.integers(0, top + 1, (h, w)).astype(np.uint8)
    b = int(rng.integers(1, 7))
    coarse = rng.integers(0, top + 1, (-(-h // b), -(-w // b)))
    return np.kron(coarse, np.ones((b, b), dtype=np.int64))[:h, :w].astype(np.uint8)
