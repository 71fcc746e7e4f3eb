"""The files the scaled-JPEG tests share (helper, not collected): test_jpeg_scaled_cpu.py compares the NumPy model with
Pillow on them, test_gpu_jpeg_scaled.py the device with Pillow and the model.  Everything is built at import or on first
use from seeds; nothing is stored."""
import functools
import io

import numpy as np
from PIL import Image

import jpeg_writer as W

SCALES = (2, 4, 8)
MODES = {"L": None, "444": 0, "422": 1, "420": 2}           # Pillow's subsampling argument
# (w, h): one block, edge blocks, one MCU row / column with a chroma plane at most two samples wide after scaling, 4:2:2 at 1/8
SHAPES = [(1, 1), (8, 8), (9, 17), (33, 5), (67, 93), (16, 40), (2, 200), (130, 3), (201, 333)]
MORE_SHAPES = [(7, 7), (15, 16), (17, 31), (64, 48)]        # the CPU comparison's thirteen sizes are these and SHAPES
QUALITIES = (20, 75, 98)
FUZZ_SEED, FUZZ_N = 20261019, 300
EXTREME_SEED = 20261020


def jpeg(arr, **save):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", **save)
    return b.getvalue()


def photo(rng, h, w, channels):
    """Noise over a smooth field: every coefficient gets used, the picture is not flat anywhere."""
    y, x = np.mgrid[0:h, 0:w]
    planes = [np.clip((y * (3 + c) + x * (5 - c)) % 256 * 0.6 + rng.integers(0, 110, (h, w)), 0, 255).astype(np.uint8) for c in range(channels)]
    return planes[0] if channels == 1 else np.dstack(planes)


@functools.lru_cache(maxsize=None)
def written(w, h, mode, quality=75, restart=0):
    """The Pillow-written file of that shape, seeded by it."""
    rng = np.random.default_rng([w, h, quality, list(MODES).index(mode)])
    save = {"quality": quality}
    if MODES[mode] is not None:
        save["subsampling"] = MODES[mode]
    if restart:
        save["restart_marker_blocks"] = restart
    return jpeg(photo(rng, h, w, 1 if mode == "L" else 3), **save)


def fuzz_file(k):
    """Small Pillow-written file k of the seeded fuzz: (description, bytes)."""
    rng = np.random.default_rng([FUZZ_SEED, k])
    w, h = int(rng.integers(1, 70)), int(rng.integers(1, 70))
    mode = list(MODES)[int(rng.integers(4))]
    save = {"quality": int(rng.choice([1, 10, 35, 75, 90, 100])), "optimize": bool(rng.integers(2))}
    if MODES[mode] is not None:
        save["subsampling"] = MODES[mode]
    r = int(rng.integers(4))
    if r == 1:
        save["restart_marker_blocks"] = int(rng.integers(1, 12))
    elif r == 2:
        save["restart_marker_rows"] = 1
    kind = int(rng.integers(3))
    c = 1 if mode == "L" else 3
    if kind == 0:
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    elif kind == 1:
        a = photo(rng, h, w, c).reshape(h, w, c)
    else:                                                    # hard edges between saturated colours
        a = (rng.integers(0, 2, (-(-h // 5), -(-w // 3), c), dtype=np.uint8) * 255).repeat(5, axis=0).repeat(3, axis=1)[:h, :w]
    a = np.ascontiguousarray(a[:, :, 0] if c == 1 else a)
    return f"fuzz {k} {w}x{h} {mode} {save}", jpeg(a, **save)


# ---------------------------------------------------------------------------------------------------------------------
# hand-built files whose dequantised coefficients, intermediate sums or outputs leave their ordinary range
# ---------------------------------------------------------------------------------------------------------------------
def _build(w, h, mode, coefs, qts, pq=0, ri=0):
    sampling = W.SAMPLING[mode]
    hts = W.tables_for(coefs, sampling, ri, w, h, (0, 1, 2), (0, 1, 2))
    return W.write(w, h, sampling, coefs, qts, hts, tq=(0, 1, 2), td=(0, 1, 2), ta=(0, 1, 2), pq=pq, ri=ri)


def _nblocks(w, h, mode):
    mcux, mcuy, layout = W.geometry(w, h, W.SAMPLING[mode])
    return mcux * mcuy * len(layout)


EXTREME_KINDS = ("huge q255", "huge q1", "32767 q1", "small q16bit", "row 0 only", "rows 0 and 4", "column 4", "DC q255", "DC q16bit",
                 "DC q65535", "moderate q60", "row 0 and one more")


@functools.lru_cache(maxsize=None)
def extreme(kind, mode):
    """40 x 24 file of one kind of extreme block in every component.  "huge q1": dense blocks of dequantised coefficients up
    to +-1023 -- they fit 11 bits signed, the class no decoder may leave out, and the outputs leave 0-255 by far."""
    w, h = 40, 24
    n = _nblocks(w, h, mode)
    rng = np.random.default_rng([EXTREME_SEED, EXTREME_KINDS.index(kind), list(MODES).index(mode)])
    q8 = lambda: {t: [int(x) for x in rng.integers(1, 256, 64)] for t in range(3)}          # noqa: E731
    q16 = lambda: {t: [int(x) for x in rng.integers(1, 65536, 64)] for t in range(3)}       # noqa: E731
    one = {t: [1] * 64 for t in range(3)}
    dc = rng.integers(-1023, 1024, n)
    c = np.zeros((n, 64), np.int64)
    if kind == "huge q255":
        return _build(w, h, mode, rng.integers(-1023, 1024, (n, 64)), q8())
    if kind == "huge q1":
        return _build(w, h, mode, rng.integers(-1023, 1024, (n, 64)), one)
    if kind == "32767 q1":
        c = rng.choice([-32767, -16384, 16384, 32767, 0, 5, -300], (n, 64))
        c[:, 0] = dc
        return _build(w, h, mode, c, one)
    if kind == "small q16bit":
        return _build(w, h, mode, rng.integers(-3, 4, (n, 64)), q16(), pq=1)
    if kind == "row 0 only":                                 # the 4 x 4 short cut with AC terms in row 0
        c[:, :8] = rng.integers(-1023, 1024, (n, 8))
        return _build(w, h, mode, c, q8())
    if kind == "rows 0 and 4":                               # row 4 is not looked at: still the short cut
        c[:, :8] = rng.integers(-1023, 1024, (n, 8))
        c[:, 32:40] = rng.integers(-1023, 1024, (n, 8))
        return _build(w, h, mode, c, q8())
    if kind == "column 4":                                   # column 4 is looked at: not the short cut, in every second block
        c[:, 0] = dc
        c[::2, 4::8] = rng.integers(-1023, 1024, (len(c[::2]), 8))
        return _build(w, h, mode, c, q8())
    if kind == "DC q255":
        c[:, 0] = dc
        return _build(w, h, mode, c, q8())
    if kind == "DC q16bit":
        c[:, 0] = dc
        return _build(w, h, mode, c, q16(), pq=1)
    if kind == "DC q65535":                                  # 1 x 1 reads the quantiser as a signed 16-bit number
        c[:, 0] = dc // 100
        return _build(w, h, mode, c, {t: [65535] * 64 for t in range(3)}, pq=1)
    if kind == "moderate q60":
        c = rng.integers(-40, 41, (n, 64)) * (rng.random((n, 64)) < .3)
        c[:, 0] = rng.integers(-200, 200, n)
        return _build(w, h, mode, c, {t: [int(x) for x in rng.integers(1, 61, 64)] for t in range(3)})
    assert kind == "row 0 and one more"
    c[:, 0] = dc
    c[:, 3] = -1000
    c[:, 8 * int(rng.integers(1, 8))] = 900
    return _build(w, h, mode, c, q8())
