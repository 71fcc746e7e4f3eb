#!/usr/bin/env python3
"""The gallery page (process-images.py:1344-1375): 12 stored images of 2048 x 1536, each turned into a 400 x 400 LANCZOS
thumbnail (process-images.py:186-189) -- ``thumbnail`` on the GPU next to Pillow's ``Image.thumbnail``, whose resampler runs
on one host core.

Three sources: RGB ndarrays, PNG-backed and JPEG-backed PIL images (a file-backed image is opened afresh for every call,
as load_image_from_db does, so its decode -- and for JPEG the draft at reduced scale -- is part of both sides).  The
upload line is ``lars_memcpy_h2d`` of the same 9.4 MB pageable ndarray: the floor of a host-to-device call at this size.
Every GPU leg ends in a device synchronise.

    python tools/thumbbench.py [--reps 5] [--gpu-only] [--json out.json]

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/thumbbench.py --gpu-only
"""
import argparse
import ctypes as C
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

N_IMAGES, W, H, SIZE = 12, 2048, 1536, (400, 400)


def gallery(seed=7):
    """12 RGB images with some structure (a JPEG of pure noise decodes unlike a photograph)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for k in range(N_IMAGES):
        base = np.stack([np.sin(xx / (37 + 5 * k) + c) * np.cos(yy / (53 + 3 * k) - c) for c in (0.0, 1.0, 2.0)], axis=-1)
        img = (127.5 + 100 * base + rng.normal(0, 12, (H, W, 3))).clip(0, 255).astype(np.uint8)
        out.append(img)
    return out


def encode(arrs, fmt):
    blobs = []
    for a in arrs:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, fmt, **({"quality": 90} if fmt == "JPEG" else {}))
        blobs.append(buf.getvalue())
    return blobs


def per_call_ms(fn, items, reps):
    """Median over reps of (time for one pass over the gallery) / len(items), after one warm-up pass."""
    for it in items:
        fn(it)
    _ffi.call("lars_synchronize", None)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for it in items:
            fn(it)
        _ffi.call("lars_synchronize", None)
        ts.append((time.perf_counter() - t0) / len(items))
    return float(np.median(ts)) * 1e3


def pillow_ms(fn, items, reps):
    for it in items:
        fn(it)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for it in items:
            fn(it)
        ts.append((time.perf_counter() - t0) / len(items))
    return float(np.median(ts)) * 1e3


def pil_thumb(img):
    img.thumbnail(SIZE, Image.Resampling.LANCZOS)
    return img


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="skip the Pillow legs (for a kernel trace)")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    if _ffi.device_count() < 1:
        sys.exit("thumbbench: needs a gfx950 GPU (no CPU fallback)")
    arrs = gallery()
    pngs, jpgs = encode(arrs, "PNG"), encode(arrs, "JPEG")
    res = {"device": _ffi.device_name(), "images": N_IMAGES, "shape": [H, W, 3], "size": list(SIZE), "reps": args.reps}

    # bit-exactness first: a fast wrong answer is no answer
    for a, j in zip(arrs[:2], jpgs[:2]):
        assert np.array_equal(lars.thumbnail(a), np.asarray(pil_thumb(Image.fromarray(a))))
        assert np.array_equal(np.asarray(lars.thumbnail(Image.open(io.BytesIO(j)))), np.asarray(pil_thumb(Image.open(io.BytesIO(j)))))

    dev = _ffi.DeviceBuffer(arrs[0].nbytes)
    res["upload_ms"] = per_call_ms(lambda a: _ffi.call("lars_memcpy_h2d", C.c_void_p(dev.ptr), _ffi.ptr(a), a.nbytes), arrs, args.reps)
    dev.free()
    res["gpu_ndarray_ms"] = per_call_ms(lars.thumbnail, arrs, args.reps)
    res["gpu_png_ms"] = per_call_ms(lambda b: lars.thumbnail(Image.open(io.BytesIO(b))), pngs, args.reps)
    res["gpu_jpeg_ms"] = per_call_ms(lambda b: lars.thumbnail(Image.open(io.BytesIO(b))), jpgs, args.reps)
    if not args.gpu_only:
        res["decode_png_ms"] = pillow_ms(lambda b: Image.open(io.BytesIO(b)).load(), pngs, args.reps)
        res["pillow_ndarray_ms"] = pillow_ms(lambda a: pil_thumb(Image.fromarray(a)), arrs, args.reps)
        res["pillow_png_ms"] = pillow_ms(lambda b: pil_thumb(Image.open(io.BytesIO(b))), pngs, args.reps)
        res["pillow_jpeg_ms"] = pillow_ms(lambda b: pil_thumb(Image.open(io.BytesIO(b))), jpgs, args.reps)

    print(f"device: {res['device']}   gallery: {N_IMAGES} x {W}x{H} RGB -> thumbnail{SIZE}, per call (median of {args.reps})")
    print(f"  upload of one 9.4 MB ndarray (lars_memcpy_h2d)  {res['upload_ms']:8.3f} ms")
    for src in ("ndarray", "png", "jpeg"):
        line = f"  {src:8s}  GPU thumbnail {res[f'gpu_{src}_ms']:8.3f} ms"
        if not args.gpu_only:
            line += f"   Pillow thumbnail {res[f'pillow_{src}_ms']:8.3f} ms   x{res[f'pillow_{src}_ms'] / res[f'gpu_{src}_ms']:.1f}"
        print(line)
    if not args.gpu_only:
        print(f"  PNG decode alone (Image.open + load)            {res['decode_png_ms']:8.3f} ms")
        print(f"  gallery page of {N_IMAGES} from ndarrays: GPU {N_IMAGES * res['gpu_ndarray_ms']:.1f} ms, "
              f"Pillow {N_IMAGES * res['pillow_ndarray_ms']:.1f} ms")
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
