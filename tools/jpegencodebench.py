#!/usr/bin/env python3
"""JPEG encoding for the camera path (process-rgn.py:47 with :72-73, process-images.py:247): ``encode_jpeg`` on the GPU next to
Pillow's ``Image.fromarray(a).save(BytesIO(), "JPEG")`` on one host core, in the same run on the same host.

Pictures: seeded 1/f fields (tools/pngbench.py's ``field_1f``), the gallery picture 2048 x 1536 RGB and 4096 x 4096 RGB, at
the default quality and subsampling.  Per picture, host array in and the file's bytes out, ending in a device synchronise: the
median over ``--files`` different pictures after a warm-up pass.  Every file is checked against Pillow's first.  ``--split``
adds the parts of one call (upload, the kernels from a resident picture into a resident file, download of the file).

    python tools/jpegencodebench.py [--files 20] [--split] [--gpu-only] [--json out.json]

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/jpegencodebench.py --gpu-only
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_image_processing_amd as lars  # noqa: E402
from lars_image_processing_amd import _ffi  # noqa: E402
from jpegdecodebench import pictures  # noqa: E402

KINDS = {"gallery_2048x1536_rgb": (1536, 2048), "rgb_4096x4096": (4096, 4096)}


def pil_jpeg(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=75, subsampling="4:2:0")
    return b.getvalue()


def per_picture_ms(fn, arrays, gpu):
    """Median over the pictures of the time of one call, after a warm-up pass over all of them."""
    for a in arrays:
        fn(a)
    ts = []
    for a in arrays:
        if gpu:
            _ffi.call("lars_synchronize", None)
        t0 = time.perf_counter()
        fn(a)
        if gpu:
            _ffi.call("lars_synchronize", None)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def split_ms(a, reps=20):
    """The parts of one encode_jpeg call, each timed on its own (median): upload of the picture, the kernels from a resident
    picture into a resident file (lars_d_encode_jpeg_u8), download of the file's bytes."""
    lib = _ffi.load()
    h, w, c = a.shape
    cap, need = lib.lars_jpeg_bound(h, w, c, 2), lib.lars_jpeg_encode_scratch_bytes(h, w, c, 2)

    def med(fn):
        fn()
        ts = []
        for _ in range(reps):
            _ffi.call("lars_synchronize", None)
            t0 = time.perf_counter()
            fn()
            _ffi.call("lars_synchronize", None)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    d_in, d_out, d_scratch, d_len = (C.c_void_p() for _ in range(4))
    _ffi.call("lars_malloc", C.byref(d_in), a.nbytes)
    _ffi.call("lars_malloc", C.byref(d_out), cap)
    _ffi.call("lars_malloc", C.byref(d_scratch), need)
    _ffi.call("lars_malloc", C.byref(d_len), 8)
    try:
        upload = med(lambda: _ffi.call("lars_memcpy_h2d", d_in, _ffi.ptr(a), a.nbytes))
        device = med(lambda: _ffi.call("lars_d_encode_jpeg_u8", d_in, h, w, c, 75, 2, d_out, cap, d_len, d_scratch, None))
        n = np.zeros(1, np.int64)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(n), d_len, 8)
        out = np.empty(int(n[0]), np.uint8)
        download = med(lambda: _ffi.call("lars_memcpy_d2h", _ffi.ptr(out), d_out, out.size))
    finally:
        for p in (d_in, d_out, d_scratch, d_len):
            _ffi.call("lars_free", p)
    assert out.tobytes() == pil_jpeg(a)
    return {"upload_ms": upload, "device_encode_ms": device, "download_ms": download}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=20, help="pictures per kind (each timed once after the warm-up)")
    ap.add_argument("--gpu-only", action="store_true", help="skip the Pillow leg (for a kernel trace)")
    ap.add_argument("--split", action="store_true", help="also time the parts of one call")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    if _ffi.device_count() < 1:
        sys.exit("jpegencodebench: needs a gfx950 GPU (no CPU fallback)")
    import PIL
    res = {"device": _ffi.device_name(), "pillow": PIL.__version__, "files": args.files, "quality": 75, "subsampling": "4:2:0", "kinds": {}}
    for name, shape in KINDS.items():
        arrays = pictures(shape, args.files, seed=11)
        files = [lars.encode_jpeg(a) for a in arrays]
        for a, b in list(zip(arrays, files))[:2]:             # a fast wrong answer is no answer
            assert b == pil_jpeg(a)
        r = {"files": len(arrays), "mean_file_bytes": int(np.mean([len(b) for b in files])), "shape": [shape[0], shape[1], 3],
             "encode_jpeg_ms": per_picture_ms(lars.encode_jpeg, arrays, True)}
        if not args.gpu_only:
            r["pillow_save_ms"] = per_picture_ms(pil_jpeg, arrays, False)
            r["encode_speedup"] = r["pillow_save_ms"] / r["encode_jpeg_ms"]
        if args.split:
            r["split"] = split_ms(arrays[0])
        res["kinds"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
