#!/usr/bin/env python3
"""TIFF encoding for the batch job's primary output (backend-process.py:57, ``<name>_wb.tif``): ``encode_tiff`` on the GPU next
to Pillow's ``Image.fromarray(a).save(BytesIO(), format="TIFF", compression="tiff_lzw")`` on one host core, in the same run on
the same host.

Pictures: seeded 1/f fields (tools/pngbench.py's ``field_1f``), the gallery picture 2048 x 1536 RGB and 4096 x 4096 RGB, with
and without the horizontal predictor.  ``--files`` pictures per kind: four different fields, the others the same fields rolled
by odd steps in both directions (other strips, the same statistics).  Per picture, host array in and the file's bytes out,
ending in a device synchronise: the median over the pictures after a warm-up pass, the smaller of ``--runs`` such medians.
Every file is read back first.  ``--split`` adds the parts of one call (upload, the kernels from a resident picture into a
resident file, download of the file), ``--sweep`` the knob "tiff_strip_bytes" at 8192 .. 262144.

The float leg (``--legs float`` alone, ``--legs all`` with the pictures): the float32 NDVI plane of the same 1/f pictures at
4096 x 4096 and 2048 x 1536, computed by the library, through ``encode_tiff_f32`` with and without the floating-point
predictor next to Pillow's ``Image.fromarray(plane).save(format="TIFF", compression="tiff_lzw", tiffinfo={317: 3})`` (and without
the tag), file sizes of both; and ``process_image(want_tiff=...)``, where the planes never leave the device, next to the same
call with ``want_arrays=True`` followed by ``encode_tiff_f32`` on the three host planes, in the same process.

``--compression deflate`` runs every leg with ``compression="deflate"`` (``want_tiff="deflate+predictor"``) next to Pillow's
``compression="tiff_adobe_deflate"`` instead, ``--compression both`` the LZW legs and then the Deflate legs in the same run, by
the same rules; the Deflate entries carry ``_deflate`` in their names.

``--matching`` adds to every Deflate entry, in the same run, the file size and the time with the tuning knob ``deflate_matching``
at 1 (``lars.deflate_matching()``: string matching in the Deflate coder), and a leg of its own with the rasters it is for: a
two-class mask and a flat raster, uint8 4096 x 4096, knob 0 and 1 next to Pillow's ``tiff_adobe_deflate``.

    python tools/tiffencodebench.py [--legs picture] [--compression lzw] [--files 20] [--runs 2] [--split] [--sweep] [--matching] [--gpu-only] [--json out.json]

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/tiffencodebench.py --gpu-only
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
from lars_image_processing_amd import _ffi, tiffio  # noqa: E402
from jpegdecodebench import pictures  # noqa: E402

KINDS = {"gallery_2048x1536_rgb": (1536, 2048), "rgb_4096x4096": (4096, 4096)}
SWEEP = (8192, 16384, 32768, 65536, 131072, 262144)
DISTINCT = 4


def many_pictures(shape, n, seed):
    base = pictures(shape, min(n, DISTINCT), seed)
    return [np.ascontiguousarray(np.roll(base[k % len(base)], (97 * (k // len(base)), 131 * (k // len(base))), (0, 1))) for k in range(n)]


PILLOW = {"lzw": "tiff_lzw", "deflate": "tiff_adobe_deflate"}


def pil_tiff(a, predictor=False, compression="lzw"):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="TIFF", compression=PILLOW[compression], **({"tiffinfo": {317: 2}} if predictor else {}))
    return b.getvalue()


def per_picture_ms(fn, arrays, gpu, runs):
    """The smaller of ``runs`` medians over the pictures of the time of one call, after a warm-up pass over all of them."""
    for a in arrays:
        fn(a)
    best = []
    for _ in range(runs):
        ts = []
        for a in arrays:
            if gpu:
                _ffi.call("lars_synchronize", None)
            t0 = time.perf_counter()
            fn(a)
            if gpu:
                _ffi.call("lars_synchronize", None)
            ts.append(time.perf_counter() - t0)
        best.append(float(np.median(ts)) * 1e3)
    return min(best)


def split_ms(a, predictor, reps=20, compression="lzw"):
    """The parts of one encode_tiff call, each timed on its own (median): upload of the picture, the kernels from a resident
    picture into a resident file (lars_d_encode_tiff), download of the file's bytes."""
    lib = _ffi.load()
    h, w, c = a.shape
    mid = "_deflate" if compression == "deflate" else ""
    cap = getattr(lib, f"lars_tiff{mid}_bound")(h, w, c, 1, 0)
    need = getattr(lib, f"lars_tiff{mid}_encode_scratch_bytes")(h, w, c, 1, 0)

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

    d_in, d_out, d_scratch, d_ans = (C.c_void_p() for _ in range(4))
    _ffi.call("lars_malloc", C.byref(d_in), a.nbytes)
    _ffi.call("lars_malloc", C.byref(d_out), cap)
    _ffi.call("lars_malloc", C.byref(d_scratch), need)
    _ffi.call("lars_malloc", C.byref(d_ans), 16)
    try:
        upload = med(lambda: _ffi.call("lars_memcpy_h2d", d_in, _ffi.ptr(a), a.nbytes))
        device = med(lambda: _ffi.call("lars_d_encode_tiff" + mid, d_in, h, w, c, 1, 0, int(predictor), d_out, cap, d_ans, C.c_void_p(d_ans.value + 8),
                                       d_scratch, None))
        n = np.zeros(2, np.int64)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(n), d_ans, 16)
        assert n[1] == 0, "device status"
        out = np.empty(int(n[0]), np.uint8)
        download = med(lambda: _ffi.call("lars_memcpy_d2h", _ffi.ptr(out), d_out, out.size))
    finally:
        for p in (d_in, d_out, d_scratch, d_ans):
            _ffi.call("lars_free", p)
    assert np.array_equal(tiffio.read_tiff(out.tobytes()), a)
    return {"upload_ms": upload, "device_encode_ms": device, "download_ms": download}


def pil_float_tiff(a, predictor=False, compression="lzw"):
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="TIFF", compression=PILLOW[compression], **({"tiffinfo": {317: 3}} if predictor else {}))
    return b.getvalue()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def float_leg(args, res, comp="lzw"):
    """encode_tiff_f32 on NDVI planes, and process_image(want_tiff=...) against planes that come back and go up again."""
    deflate = comp == "deflate"
    tag = "_deflate" if deflate else ""

    def decode(b):
        return lars.decode_tiff(b, deflate=True) if deflate else lars.decode_tiff(b)

    for name, shape in (("ndvi_4096x4096_f32", (4096, 4096)), ("ndvi_2048x1536_f32", (1536, 2048))):
        rgb = many_pictures(shape, min(args.files, DISTINCT), seed=11)
        planes = [lars.calculate_index(a, "NDVI") for a in rgb]
        for predictor in (False, True):
            files = [lars.encode_tiff_f32(a, predictor=predictor, compression=comp) for a in planes[:2]]
            for a, b in zip(planes, files):                    # a fast wrong answer is no answer
                assert same_bits(tiffio.read_tiff(b), a) and same_bits(np.asarray(Image.open(io.BytesIO(b))), a) and same_bits(decode(b), a)
            r = {"files": len(planes), "mean_file_bytes": int(np.mean([len(b) for b in files])), "shape": list(shape), "plane_bytes": planes[0].nbytes,
                 "strips": len(tiffio._read_ifd(memoryview(files[0]), "<")[tiffio.STRIP_OFFSETS]),
                 "encode_tiff_f32_ms": per_picture_ms(lambda a: lars.encode_tiff_f32(a, predictor=predictor, compression=comp), planes, True,
                                                      args.runs)}
            if args.matching and deflate:
                with lars.deflate_matching():
                    files = [lars.encode_tiff_f32(a, predictor=predictor, compression=comp) for a in planes[:2]]
                    assert all(same_bits(tiffio.read_tiff(b), a) for a, b in zip(planes, files))
                    r["matching_mean_file_bytes"] = int(np.mean([len(b) for b in files]))
                    r["encode_tiff_f32_matching_ms"] = per_picture_ms(lambda a: lars.encode_tiff_f32(a, predictor=predictor, compression=comp), planes,
                                                                      True, args.runs)
            if not args.gpu_only:
                pil = pil_float_tiff(planes[0], predictor, comp)
                r["pillow_file_bytes"] = len(pil)
                r["pillow_strips"] = len(tiffio._read_ifd(memoryview(pil), "<")[tiffio.STRIP_OFFSETS])
                r["same_strips_as_pillow"] = bool(tiffio._read_ifd(memoryview(pil), "<")[tiffio.STRIP_BYTE_COUNTS] ==
                                                  tiffio._read_ifd(memoryview(files[0]), "<")[tiffio.STRIP_BYTE_COUNTS])
                r["pillow_save_ms"] = per_picture_ms(lambda a: pil_float_tiff(a, predictor, comp), planes, False, args.runs)
                r["encode_speedup"] = r["pillow_save_ms"] / r["encode_tiff_f32_ms"]
            key = name + tag + ("_predictor3" if predictor else "")
            res["kinds"][key] = r
            print(key, json.dumps(r), flush=True)
        # the three index planes of one picture as files: on the device all the way, or down as arrays and up again
        mode = "deflate+predictor" if deflate else "predictor"

        def on_device(a):
            return lars.process_image(a, want_arrays=False, want_tiff=mode)

        def through_host(a):
            got = lars.process_image(a, want_arrays=True)
            return {t: lars.encode_tiff_f32(got["indices"][t]["index"], predictor=True, compression=comp) for t in got["indices"]}

        one, two = on_device(rgb[0]), through_host(rgb[0])
        assert all(one["indices"][t]["tiff"] == two[t] for t in two)
        r = {"shape": list(shape), "indices": 3, "file_bytes": {t: len(b) for t, b in two.items()},
             "process_image_want_tiff_ms": per_picture_ms(on_device, rgb, True, args.runs),
             "process_image_arrays_then_encode_ms": per_picture_ms(through_host, rgb, True, args.runs)}
        r["speedup"] = r["process_image_arrays_then_encode_ms"] / r["process_image_want_tiff_ms"]
        res["kinds"][name + tag + "_process_image"] = r
        print(name + tag + "_process_image", json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=20, help="pictures per kind (each timed once per run after the warm-up)")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--gpu-only", action="store_true", help="skip the Pillow leg (for a kernel trace)")
    ap.add_argument("--split", action="store_true", help="also time the parts of one call")
    ap.add_argument("--sweep", action="store_true", help='also sweep "tiff_strip_bytes"')
    ap.add_argument("--legs", choices=["picture", "float", "all"], default="picture",
                    help="picture: the RGB pictures through encode_tiff; float: NDVI planes through encode_tiff_f32; all: both")
    ap.add_argument("--compression", choices=["lzw", "deflate", "both"], default="lzw",
                    help="lzw: the LZW legs; deflate: the same legs with compression=\"deflate\"; both: one after the other in the same run")
    ap.add_argument("--matching", action="store_true",
                    help='Deflate legs also under the knob "deflate_matching" = 1, and the mask and flat rasters (with --compression deflate or both)')
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    if _ffi.device_count() < 1:
        sys.exit("tiffencodebench: needs a gfx950 GPU (no CPU fallback)")
    import PIL
    res = {"device": _ffi.device_name(), "pillow": PIL.__version__, "files": args.files, "runs": args.runs,
           "tiff_strip_bytes": _ffi.get_tuning("tiff_strip_bytes"), "kinds": {}}
    for comp in ("lzw", "deflate") if args.compression == "both" else (args.compression,):
        picture_and_float_legs(args, res, comp)
        if args.matching and comp == "deflate":
            mask_leg(args, res)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def mask_leg(args, res):
    """The rasters string matching is for, uint8 4096 x 4096 through encode_tiff(compression="deflate"): knob 0, knob 1, Pillow."""
    from pngbench import field_1f
    f = field_1f(4096, 1.5, 7)
    for name, a in (("mask_4096x4096_deflate", (f > 0.05).astype(np.uint8)), ("flat_4096x4096_deflate", np.full((4096, 4096), 90, np.uint8))):
        arrays = [a, np.ascontiguousarray(np.roll(a, (97, 131), (0, 1)))]
        r = {"shape": list(a.shape), "raw_bytes": int(a.nbytes)}
        for key, block in (("", lars.deflate_matching(False)), ("matching_", lars.deflate_matching())):
            with block:
                b = lars.encode_tiff(a, compression="deflate")
                assert np.array_equal(tiffio.read_tiff(b), a)
                r[key + "file_bytes"] = len(b)
                r[key + "encode_tiff_ms"] = per_picture_ms(lambda x: lars.encode_tiff(x, compression="deflate"), arrays, True, max(args.runs, 3))
        if not args.gpu_only:
            r["pillow_file_bytes"] = len(pil_tiff(a, False, "deflate"))
            r["pillow_save_ms"] = per_picture_ms(lambda x: pil_tiff(x, False, "deflate"), arrays, False, args.runs)
        res["kinds"][name] = r
        print(name, json.dumps(r), flush=True)


def picture_and_float_legs(args, res, comp):
    deflate = comp == "deflate"
    if args.legs in ("float", "all"):
        float_leg(args, res, comp)
    for name, shape in KINDS.items() if args.legs in ("picture", "all") else ():
        arrays = many_pictures(shape, args.files, seed=11)
        for predictor in (False, True):
            files = [lars.encode_tiff(a, predictor=predictor, compression=comp) for a in arrays[:DISTINCT]]
            for a, b in list(zip(arrays, files))[:2]:          # a fast wrong answer is no answer
                assert np.array_equal(tiffio.read_tiff(b), a) and np.array_equal(np.asarray(Image.open(io.BytesIO(b))), a)
            r = {"files": len(arrays), "mean_file_bytes": int(np.mean([len(b) for b in files])), "shape": [shape[0], shape[1], 3],
                 "strips": len(tiffio._read_ifd(memoryview(files[0]), "<")[tiffio.STRIP_OFFSETS]),
                 "encode_tiff_ms": per_picture_ms(lambda a: lars.encode_tiff(a, predictor=predictor, compression=comp), arrays, True, args.runs)}
            if args.matching and deflate:
                with lars.deflate_matching():
                    files = [lars.encode_tiff(a, predictor=predictor, compression=comp) for a in arrays[:DISTINCT]]
                    assert all(np.array_equal(tiffio.read_tiff(b), a) for a, b in list(zip(arrays, files))[:2])
                    r["matching_mean_file_bytes"] = int(np.mean([len(b) for b in files]))
                    r["encode_tiff_matching_ms"] = per_picture_ms(lambda a: lars.encode_tiff(a, predictor=predictor, compression=comp), arrays, True,
                                                                  args.runs)
            if not args.gpu_only:
                pil = pil_tiff(arrays[0], predictor, comp)
                r["pillow_file_bytes"] = len(pil)
                r["pillow_strips"] = len(tiffio._read_ifd(memoryview(pil), "<")[tiffio.STRIP_OFFSETS])
                r["pillow_save_ms"] = per_picture_ms(lambda a: pil_tiff(a, predictor, comp), arrays, False, args.runs)
                r["encode_speedup"] = r["pillow_save_ms"] / r["encode_tiff_ms"]
            if args.split:
                r["split"] = split_ms(arrays[0], predictor, compression=comp)
            if args.sweep:
                r["sweep_encode_tiff_ms"] = {}
                for v in SWEEP:
                    with _ffi.tuning(tiff_strip_bytes=v):
                        r["sweep_encode_tiff_ms"][str(v)] = per_picture_ms(lambda a: lars.encode_tiff(a, predictor=predictor, compression=comp),
                                                                           arrays[:DISTINCT + 1], True, args.runs)
            key = name + ("_deflate" if deflate else "") + ("_predictor" if predictor else "")
            res["kinds"][key] = r
            print(key, json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
