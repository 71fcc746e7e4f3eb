#!/usr/bin/env python3
"""TIFF decoding for the first accepted extension (process-images.py:1237, :183): ``decode_tiff`` and ``thumbnail_tiff`` on
the GPU next to Pillow's ``Image.open(...).load()`` (libtiff) where Pillow reads the file, ``tiffio.read_tiff`` (the host
thread pool) on every file, and an uncompressed copy of each file (the assembly stage's floor).

File sets: 20 gallery pictures (2048 x 1536 RGB, 8 bit, LZW with Pillow's defaults), 4096 x 4096 RGB 8-bit LZW with
predictor from Pillow, and three-sample uint16 files with LZW and predictor from ``write_tiff`` plus the test encoder
(``--side16``, 768 by default: the encoder is Python).  The Deflate legs (``decode_tiff(..., deflate=True)``, in the same
run and by the same rules): the gallery pictures as Pillow writes them with ``tiff_adobe_deflate``, the 4096 x 4096 file with
predictor, the uint16 file from ``write_tiff(deflate=True, predictor=True)``, and one 1024 x 1024 RGB file written as a
single strip, which one lane decodes.  The float legs (``f32_*``): the float32 NDVI plane of the 1/f pictures of
``tiffencodebench.py`` at 4096 x 4096 and 2048 x 1536, computed by the library and written by Pillow with ``tiff_lzw``, with
and without the floating-point predictor (317: 3); no thumbnails there.  Per file kind, after a warm-up pass: the median over reps of the
per-file time, host bytes in and host array out, each call ending in a device synchronise.  Every result is checked
against ``read_tiff`` first.  Each kind runs in a child process of its own under a time limit.

    python tools/tiffdecodebench.py [--reps 5] [--gpu-only] [--json out.json]

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/tiffdecodebench.py --kind gallery_rgb_lzw --gpu-only
"""
import argparse
import io
import json
import os
import subprocess
import sys
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KINDS = ("gallery_rgb_lzw", "rgb_4096_lzw_predictor", "u16x3_lzw_predictor",
         "gallery_rgb_deflate", "rgb_4096_deflate_predictor", "u16x3_deflate_predictor", "rgb_1024_deflate_one_strip",
         "f32_4096_lzw", "f32_4096_lzw_predictor3", "f32_2048x1536_lzw", "f32_2048x1536_lzw_predictor3")
LIMIT_S = 420


def pil_tiff(a, **save):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "TIFF", **save)
    return b.getvalue()


def files_of(kind, side16):
    """[(file, uncompressed copy, Pillow reads it)]"""
    from thumbbench import gallery
    import tiff_cases as tc
    scheme = "tiff_adobe_deflate" if "deflate" in kind else "tiff_lzw"
    if kind.startswith("f32_"):
        import lars_image_processing_amd as lars
        from jpegdecodebench import pictures
        planes = [lars.calculate_index(a, "NDVI") for a in pictures((4096, 4096) if "4096_" in kind else (1536, 2048), 2, seed=11)]
        extra = {"tiffinfo": {317: 3}} if kind.endswith("predictor3") else {}
        return [(pil_tiff(a, compression=scheme, **extra), pil_tiff(a), True) for a in planes]
    if kind in ("gallery_rgb_lzw", "gallery_rgb_deflate"):
        pics = (gallery(7) + gallery(8))[:20]
        return [(pil_tiff(a, compression=scheme), pil_tiff(a), True) for a in pics]
    if kind == "rgb_1024_deflate_one_strip":
        a = np.ascontiguousarray(gallery(7)[0][:1024, :1024])
        return [(tc.written(a, deflate=True, rows_per_strip=1024), tc.written(a, rows_per_strip=1024), True)]
    if kind in ("rgb_4096_lzw_predictor", "rgb_4096_deflate_predictor"):
        rng = np.random.default_rng(5)
        y, x = np.mgrid[0:4096, 0:4096].astype(np.float32)
        out = []
        for k in range(3):
            base = np.stack([np.sin(x / (61 + 7 * k) + c) * np.cos(y / (47 + 5 * k) - c) for c in (0.0, 1.0, 2.0)], axis=-1)
            a = (127.5 + 100 * base + rng.normal(0, 6, base.shape)).clip(0, 255).astype(np.uint8)
            out.append((pil_tiff(a, compression=scheme, tiffinfo={317: 2}), pil_tiff(a), True))
        return out
    rng = np.random.default_rng(6)
    y, x = np.mgrid[0:side16, 0:side16].astype(np.float32)
    base = np.stack([np.sin(x / 61 + c) * np.cos(y / 47 - c) for c in (0.0, 1.0, 2.0)], axis=-1)
    a = (32768 + 25000 * base + rng.normal(0, 300, base.shape)).clip(0, 65535).astype(np.uint16)
    rps = max(1, 65536 // (side16 * 6))
    packed = tc.written(a, rows_per_strip=rps, predictor=True, deflate=True) if "deflate" in kind else tc.lzw_tiff(a, rows_per_strip=rps, predictor=True)
    return [(packed, tc.written(a, rows_per_strip=rps, predictor=True), False)]


def host_ms(fn, items, reps):
    for it in items:
        fn(it)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for it in items:
            fn(it)
        ts.append((time.perf_counter() - t0) / len(items))
    return float(np.median(ts)) * 1e3


def run_kind(kind, args):
    import lars_image_processing_amd as lars
    from lars_image_processing_amd import _ffi, tiffio
    if _ffi.device_count() < 1:
        sys.exit("tiffdecodebench: needs a gfx950 GPU (no CPU fallback)")

    def gpu_ms(fn, items):
        for it in items:
            fn(it)
        _ffi.call("lars_synchronize", None)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for it in items:
                fn(it)
                _ffi.call("lars_synchronize", None)
            ts.append((time.perf_counter() - t0) / len(items))
        return float(np.median(ts)) * 1e3

    deflate = "deflate" in kind
    decode = (lambda f: lars.decode_tiff(f, deflate=True)) if deflate else lars.decode_tiff
    thumbnail = (lambda f: lars.thumbnail_tiff(f, deflate=True)) if deflate else lars.thumbnail_tiff
    sets = files_of(kind, args.side16)
    files, raws, pillow = [f for f, _r, _p in sets], [r for _f, r, _p in sets], sets[0][2]
    for f, r in zip(files[:2], raws[:2]):                      # a fast wrong answer is no answer
        want = tiffio.read_tiff(f)
        for got in (decode(f), lars.decode_tiff(r)):
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    info = lars.tiff_info(files[0], deflate=deflate)
    out_bytes = int(np.prod(info["shape"])) * info["dtype"].itemsize
    dev = _ffi.DeviceBuffer(max(out_bytes, max(len(f) for f in files)))
    first = np.frombuffer(files[0], dtype=np.uint8)
    r = {"kind": kind, "device": _ffi.device_name(), "files": len(files), "reps": args.reps, "shape": list(info["shape"]),
         "dtype": str(info["dtype"]), "chunks": info["chunks"], "mean_file_bytes": int(np.mean([len(f) for f in files])),
         "decode_tiff_ms": gpu_ms(decode, files), "decode_tiff_uncompressed_ms": gpu_ms(lars.decode_tiff, raws),
         "upload_ms": gpu_ms(lambda a: dev.upload(a), [first]), "download_ms": gpu_ms(lambda n: dev.download(np.uint8, (n,)), [out_bytes])}
    r["kernels_and_host_ms"] = r["decode_tiff_ms"] - r["upload_ms"] - r["download_ms"]
    thumbs = pillow and info["bits"] == 8
    if thumbs:
        r["thumbnail_tiff_ms"] = gpu_ms(thumbnail, files)
    if not args.gpu_only:
        r["read_tiff_ms"] = host_ms(tiffio.read_tiff, files, args.reps)
        r["speedup_over_read_tiff"] = r["read_tiff_ms"] / r["decode_tiff_ms"]
        if pillow:
            def pil_load(b):
                im = Image.open(io.BytesIO(b))
                im.load()
                return im

            def pil_thumb(b):
                im = Image.open(io.BytesIO(b))
                im.thumbnail((400, 400), Image.Resampling.LANCZOS)
                return im
            r["pillow_load_ms"] = host_ms(pil_load, files, args.reps)
            r["speedup_over_pillow"] = r["pillow_load_ms"] / r["decode_tiff_ms"]
            if thumbs:
                r["pillow_thumbnail_ms"] = host_ms(pil_thumb, files, args.reps)
                r["thumbnail_speedup"] = r["pillow_thumbnail_ms"] / r["thumbnail_tiff_ms"]
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--side16", type=int, default=768, help="side of the three-sample uint16 file")
    ap.add_argument("--gpu-only", action="store_true", help="skip the host legs (for a kernel trace)")
    ap.add_argument("--kind", choices=KINDS, help="run this kind in this process (what the parent starts per kind)")
    ap.add_argument("--only", help="the parent runs only the kinds whose names start with this (f32: the float legs)")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    if args.kind:
        return run_kind(args.kind, args)
    res = {"reps": args.reps, "kinds": {}}
    for kind in [k for k in KINDS if k.startswith(args.only or "")]:    # one child per kind, each under its own time limit; stop at the first that fails
        cmd = [sys.executable, os.path.abspath(__file__), "--kind", kind, "--reps", str(args.reps), "--side16", str(args.side16)]
        out = subprocess.run(cmd + (["--gpu-only"] if args.gpu_only else []), capture_output=True, text=True, timeout=LIMIT_S)
        if out.returncode != 0:
            sys.exit(f"tiffdecodebench: {kind} ended with status {out.returncode}\n{out.stderr[-2000:]}")
        r = json.loads(out.stdout.strip().splitlines()[-1])
        res["kinds"][kind] = r
        print(kind, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
