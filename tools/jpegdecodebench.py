#!/usr/bin/env python3
"""JPEG decoding for load_image_from_db (process-images.py:181-193): ``decode_jpeg`` and ``thumbnail_jpeg`` on the GPU next
to Pillow's ``Image.open(...).load()`` and ``Image.open(...)`` + ``.thumbnail(size, LANCZOS)`` on one host core, in the same
run on the same host.

Files, written by Pillow at its default quality and subsampling from seeded 1/f fields (tools/pngbench.py's ``field_1f``):
the gallery file, 2048 x 1536 RGB with the thumbnail box 800 x 800, and a 4096 x 4096 RGB file.  ``draft`` leaves the first
at full scale; for the second the box is 1100 x 1100, the smallest round one for which it does, because ``thumbnail_jpeg``
refuses the others.  Per file, host bytes in and host array out, ending in a device synchronise: the median over
``--files`` different files after a warm-up pass.  Every result is checked against Pillow's first.  ``--split`` adds the
parts of one call (host parse, upload, decode on the device, download); ``--sweep`` the "jpeg_subseq_bits" sweep.

The gallery legs (``GALLERY``) are what ``load_image_from_db(..., thumbnail=True)`` runs: ``thumbnail_jpeg(b, box,
scaled=True)`` against Pillow's ``thumbnail(box, LANCZOS)``, which lets ``draft`` decode at the scale ``jpeg_draft_scale``
names -- on the same files, in the same run.  The box of the application is 400 x 400: that is full scale for the 2048 x 1536
files (their short side is below 4 x 400) and 1/4 for the 4096 x 4096 ones; 350 x 350 and 200 x 200 add 1/2 and 1/8.

    python tools/jpegdecodebench.py [--files 20] [--split] [--sweep] [--gpu-only] [--only-gallery] [--json out.json]

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/jpegdecodebench.py --gpu-only
(with ``--only-gallery`` for the scaled decoder's kernels alone)
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
from pngbench import field_1f  # noqa: E402

KINDS = {"gallery_2048x1536_rgb": ((1536, 2048), (800, 800)), "rgb_4096x4096": ((4096, 4096), (1100, 1100))}
GALLERY = {"gallery_2048x1536_rgb": [((400, 400), 1), ((350, 350), 2)], "rgb_4096x4096": [((400, 400), 4), ((200, 200), 8)]}   # (box, draft scale)


def pictures(shape, n, seed):
    """n RGB pictures of 1/f content: three fields cut out of one square field each."""
    h, w = shape
    out = []
    for k in range(n):
        planes = [field_1f(max(h, w), 1.0, seed + 3 * k + c)[:h, :w] for c in range(3)]
        out.append(np.dstack([(127.5 + 127.5 * p).astype(np.uint8) for p in planes]))
    return out


def pil_jpeg(a):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG")
    return b.getvalue()


def pil_decode(b):
    im = Image.open(io.BytesIO(b))
    im.load()
    return im


def pil_thumb(b, size):
    im = Image.open(io.BytesIO(b))
    im.thumbnail(size, Image.Resampling.LANCZOS)
    return im


def per_file_ms(fn, files, gpu):
    """Median over the files of the time of one call, after a warm-up pass over all of them."""
    for b in files:
        fn(b)
    ts = []
    for b in files:
        if gpu:
            _ffi.call("lars_synchronize", None)
        t0 = time.perf_counter()
        fn(b)
        if gpu:
            _ffi.call("lars_synchronize", None)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def split_ms(b, reps=20):
    """The parts of one decode_jpeg call, each timed on its own (median): host parse, upload of the file, the decode on
    the device from a resident file into a resident array (lars_d_decode_jpeg_u8), download of the array."""
    lib = _ffi.load()
    file = np.frombuffer(b, np.uint8)
    info = _ffi.JpegInfo.array()

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

    parse = med(lambda: lib.lars_jpeg_info(_ffi.ptr(file), file.size, info))
    i = _ffi.JpegInfo(*info)
    nbytes = int(i.width * i.height * i.components)
    out = np.empty(nbytes, np.uint8)
    d_file, d_out, d_scratch, d_status = (C.c_void_p() for _ in range(4))
    _ffi.call("lars_malloc", C.byref(d_file), file.size)
    _ffi.call("lars_malloc", C.byref(d_out), nbytes)
    _ffi.call("lars_malloc", C.byref(d_scratch), lib.lars_jpeg_decode_scratch_bytes(info))
    _ffi.call("lars_malloc", C.byref(d_status), 8)
    try:
        upload = med(lambda: _ffi.call("lars_memcpy_h2d", d_file, _ffi.ptr(file), file.size))
        device = med(lambda: _ffi.call("lars_d_decode_jpeg_u8", d_file, _ffi.ptr(file), info, d_out, d_status, d_scratch, None))
        download = med(lambda: _ffi.call("lars_memcpy_d2h", _ffi.ptr(out), d_out, nbytes))
    finally:
        for p in (d_file, d_out, d_scratch, d_status):
            _ffi.call("lars_free", p)
    assert out.tobytes() == np.asarray(pil_decode(b)).tobytes()
    return {"host_parse_ms": parse, "upload_ms": upload, "device_decode_ms": device, "download_ms": download}


def gallery_legs(name, shape, files, gpu_only):
    """thumbnail_jpeg(b, box, scaled=True) and decode_jpeg(b, scale) against Pillow's thumbnail (draft and all) per box."""
    out = {}
    for box, scale in GALLERY[name]:
        assert lars.jpeg_draft_scale((shape[1], shape[0]), box) == scale
        for b in files[:2]:
            im = pil_thumb(b, box)
            assert (im.decoderconfig[0] if im.decoderconfig else 1) == scale
            assert lars.thumbnail_jpeg(b, box, scaled=True).tobytes() == np.asarray(im).tobytes()
        r = {"draft_scale": scale,
             "thumbnail_jpeg_scaled_ms": per_file_ms(lambda b: lars.thumbnail_jpeg(b, box, scaled=True), files, True),
             "decode_jpeg_at_scale_ms": per_file_ms(lambda b: lars.decode_jpeg(b, scale), files, True)}
        if not gpu_only:
            r["pillow_thumbnail_ms"] = per_file_ms(lambda b: pil_thumb(b, box), files, False)
            r["thumbnail_speedup"] = r["pillow_thumbnail_ms"] / r["thumbnail_jpeg_scaled_ms"]
        out["%dx%d" % box] = r
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=20, help="files per kind (each timed once after the warm-up)")
    ap.add_argument("--gpu-only", action="store_true", help="skip the Pillow legs (for a kernel trace)")
    ap.add_argument("--split", action="store_true", help="also time the parts of one call")
    ap.add_argument("--sweep", action="store_true", help='also sweep "jpeg_subseq_bits"')
    ap.add_argument("--only-gallery", action="store_true", help="only the gallery legs (scaled=True against Pillow's draft)")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    if _ffi.device_count() < 1:
        sys.exit("jpegdecodebench: needs a gfx950 GPU (no CPU fallback)")
    import PIL
    res = {"device": _ffi.device_name(), "pillow": PIL.__version__, "files": args.files, "jpeg_subseq_bits": _ffi.get_tuning("jpeg_subseq_bits"),
           "kinds": {}}
    for name, (shape, size) in KINDS.items():
        files = [pil_jpeg(a) for a in pictures(shape, args.files, seed=11)]
        assert lars.jpeg_draft_scale((shape[1], shape[0]), size) == 1
        if args.only_gallery:
            r = {"files": len(files), "shape": [shape[0], shape[1], 3], "gallery": gallery_legs(name, shape, files, args.gpu_only)}
            res["kinds"][name] = r
            print(name, json.dumps(r), flush=True)
            continue
        for b in files[:2]:                                   # a fast wrong answer is no answer
            assert lars.decode_jpeg(b).tobytes() == np.asarray(pil_decode(b)).tobytes()
            assert lars.thumbnail_jpeg(b, size).tobytes() == np.asarray(pil_thumb(b, size)).tobytes()
        r = {"files": len(files), "mean_file_bytes": int(np.mean([len(b) for b in files])), "shape": [shape[0], shape[1], 3],
             "thumbnail_box": list(size),
             "decode_jpeg_ms": per_file_ms(lars.decode_jpeg, files, True),
             "thumbnail_jpeg_ms": per_file_ms(lambda b: lars.thumbnail_jpeg(b, size), files, True)}
        if not args.gpu_only:
            r["pillow_load_ms"] = per_file_ms(pil_decode, files, False)
            r["pillow_thumbnail_ms"] = per_file_ms(lambda b: pil_thumb(b, size), files, False)
            r["decode_speedup"] = r["pillow_load_ms"] / r["decode_jpeg_ms"]
            r["thumbnail_speedup"] = r["pillow_thumbnail_ms"] / r["thumbnail_jpeg_ms"]
        r["gallery"] = gallery_legs(name, shape, files, args.gpu_only)
        lars.decode_jpeg(files[0])
        r["sync_rounds_first_file"] = _ffi.get_tuning("jpeg_last_rounds")
        if args.split:
            r["split"] = split_ms(files[0])
        if args.sweep:
            r["sweep_decode_jpeg_ms"] = {}
            for v in (64, 128, 256, 512, 1024, 2048, 4096):
                with _ffi.tuning(jpeg_subseq_bits=v):
                    r["sweep_decode_jpeg_ms"][str(v)] = per_file_ms(lars.decode_jpeg, files, True)
        res["kinds"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
