"""The fixed list of seeded pictures whose encode_png bytes are pinned by SHA-256 in tests/golden/png_encode_digests.json
(tests/test_gpu_png_digests.py asserts them; tests/golden/PNG_DIGESTS.md says how the file was recorded).  encode_png's compressed
bytes are its own, not zlib's, so only a recording of an earlier build can say that a change to the segment coder left them
alone.

    python tests/png_digest_cases.py --record tests/golden/png_encode_digests.json      (needs the device)
"""
import hashlib
import json
import sys

import numpy as np

SEED = 20261019
MODES = {"L": 1, "RGB": 3, "RGBA": 4, "P": 1}
SHAPES = [(1, 1), (37, 53), (300, 500)]
# one-sample pictures whose filtered stream, h * (w + 1) bytes, is 32767, 32768, 32769 and 65536 bytes long: the segment border
BORDER = [(217, 150), (256, 127), (99, 330), (512, 127)]
CONTENT = ("random", "flat", "smooth")


def picture(mode, h, w, content, seed):
    c = MODES[mode]
    rng = np.random.default_rng(seed)
    top = 200 if mode == "P" else 256
    if content == "random":
        a = rng.integers(0, top, (h, w, c))
    elif content == "flat":
        a = np.full((h, w, c), 77)
    else:                               # a slope with a little noise: dynamic blocks with long and short codes
        y, x = np.mgrid[0:h, 0:w]
        a = ((3 * x + 5 * y)[..., None] // (1 + np.arange(c)) + rng.integers(0, 3, (h, w, c))) % top
    a = a.astype(np.uint8)
    return a[..., 0] if c == 1 else a


def cases():
    """[(name, array, palette or None)] in a fixed order."""
    out, k = [], 0
    for mode in MODES:
        for h, w in SHAPES + (BORDER if mode in ("L", "P") else []):
            for content in CONTENT:
                k += 1
                pal = np.random.default_rng(SEED - k).integers(0, 256, (200, 4)).astype(np.uint8) if mode == "P" else None
                out.append((f"{mode}-{h}x{w}-{content}", picture(mode, h, w, content, SEED + k), pal))
    return out


def digests():
    import lars_image_processing_amd as lars
    return {name: hashlib.sha256(lars.encode_png(a, palette=pal)).hexdigest() for name, a, pal in cases()}


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    import os
    sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    with open(sys.argv[2], "w") as f:
        json.dump(digests(), f, indent=1, sort_keys=True)
        f.write("\n")
