#!/usr/bin/env python3
"""PNG files of index pictures: the device encoder (api.encode_png, csrc/png.hip) next to Pillow's zlib writer, which
ends every picture of the batch driver (backend-process.py:49-73) and of the ZIP export (process-images.py:567-617).

Pictures: 4096 x 4096 RGBA RdYlGn colormaps (lars.colorize_index) of seeded 1/f^beta fields, smooth (beta 1.5) and
rough (beta 1.0).  Per picture: the host call time of encode_png (upload, kernels, length read, file download), Pillow
at compress_level=1 (what the driver uses) and 6 (Pillow's default), the file sizes; every device file is decoded once
and compared with the picture.  ``--matching`` adds, in the same run, every leg with the tuning knob ``deflate_matching`` at 1
(``lars.deflate_matching()``: string matching in the Deflate coder) and the pictures it is for: a two-class mask as a palette
picture, a five-class picture as RGBA, a flat picture.

    python tools/pngbench.py [--edge 4096] [--reps 5] [--gpu-only] [--matching] [--json out.json]

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/pngbench.py --gpu-only
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lars_image_processing_amd as lars  # noqa: E402
from lars_image_processing_amd import _ffi  # noqa: E402


def field_1f(n, beta, seed):
    rng = np.random.default_rng(seed)
    fy = np.fft.fftfreq(n)[:, None]
    fx = np.fft.rfftfreq(n)[None, :]
    f = np.sqrt(fx * fx + fy * fy)
    f[0, 0] = 1.0
    spec = (rng.normal(size=f.shape) + 1j * rng.normal(size=f.shape)) / f ** beta
    spec[0, 0] = 0
    x = np.fft.irfft2(spec, s=(n, n))
    return (x / np.abs(x).max()).astype(np.float32)


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def pillow(a, level, palette=None):
    buf = io.BytesIO()
    if palette is None:
        im = Image.fromarray(a, "RGBA" if a.ndim == 3 else "L")
    else:
        im = Image.fromarray(a, "P")
        im.putpalette(palette.tobytes(), rawmode="RGBA")
    im.save(buf, "PNG", compress_level=level)
    return buf.getvalue()


CLASS_COLOURS = np.array([[0, 0, 0, 0], [200, 40, 30, 255], [240, 220, 60, 255], [60, 180, 70, 255], [20, 90, 200, 255]], np.uint8)


def pictures(edge, matching):
    """(name, picture, palette or None)"""
    for name, beta in (("smooth", 1.5), ("rough", 1.0)):
        yield name, lars.colorize_index(field_1f(edge, beta, 7), "NDVI"), None
    if matching:
        f = field_1f(edge, 1.5, 7)
        yield "mask", (f > 0.05).astype(np.uint8), CLASS_COLOURS[[0, 3]]
        yield "classes", CLASS_COLOURS[np.digitize(f, [-0.3, -0.05, 0.1, 0.35]).astype(np.uint8)], None
        yield "flat", np.full((edge, edge), 90, np.uint8), None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--edge", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="skip the Pillow legs (for a kernel trace)")
    ap.add_argument("--matching", action="store_true", help='also every leg under the knob "deflate_matching" = 1, and the mask, class and flat pictures')
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    print("device:", _ffi.device_name(), flush=True)
    out = {"edge": args.edge, "pictures": {}}
    for name, a, palette in pictures(args.edge, args.matching):
        b = lars.encode_png(a, palette)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(b))), a), "device file does not decode to the picture"
        row = {"raw_bytes": int(a.nbytes), "device_bytes": len(b), "device_ms": median_ms(lambda: lars.encode_png(a, palette), args.reps)}
        if args.matching:
            with lars.deflate_matching():
                b = lars.encode_png(a, palette)
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(b))), a), "device file (matching) does not decode to the picture"
                row["matching_bytes"] = len(b)
                row["matching_ms"] = median_ms(lambda: lars.encode_png(a, palette), args.reps)
            row["matching_size_vs_device"] = row["matching_bytes"] / row["device_bytes"]
        if not args.gpu_only:
            for level in (1, 6):
                row[f"pillow_l{level}_bytes"] = len(pillow(a, level, palette))
                row[f"pillow_l{level}_ms"] = median_ms(lambda: pillow(a, level, palette), max(1, args.reps // 2))
            row["speedup_vs_l1"] = row["pillow_l1_ms"] / row["device_ms"]
            row["size_vs_l1"] = row["device_bytes"] / row["pillow_l1_bytes"]
            if args.matching:
                row["matching_speedup_vs_l1"] = row["pillow_l1_ms"] / row["matching_ms"]
                row["matching_size_vs_l1"] = row["matching_bytes"] / row["pillow_l1_bytes"]
        out["pictures"][name] = row
        print(name, " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
