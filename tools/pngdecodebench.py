#!/usr/bin/env python3
"""PNG decoding for load_image_from_db (process-images.py:181-193): ``decode_png`` and ``thumbnail_png`` on the GPU next to
Pillow's ``Image.open(...).load()`` and ``Image.open(...)`` + ``.thumbnail((400, 400), LANCZOS)`` on one host core.

Files: the 12 gallery pictures of tools/thumbbench.py (2048 x 1536 RGB) saved by Pillow at its default level, and
4096 x 4096 RGBA colormap pictures written by Pillow ``compress_level=1`` and by ``encode_png``.  Per file kind, after a
warm-up pass: the median over reps of the per-file time, host bytes in and host array out.  Every result is checked
against Pillow's first.

    python tools/pngdecodebench.py [--reps 5] [--gpu-only] [--json out.json]

``--variants`` measures ``decode_png(..., extended=True)`` instead, by the same rules (file bytes in, array out, median per
file after a warm-up pass, every pass ending in a device synchronise, Pillow's open + load in the same run): 2048 x 1536 RGB
interlaced, 2048 x 1536 I;16, 2048 x 1536 16-bit RGB and 4096 x 4096 palette at 4 bits, written by tests/png_variant_writer.py
(Pillow writes neither interlaced nor 16-bit RGB files), and the 8-bit gallery leg next to them.  ``--gallery-only`` is that
last leg alone: it needs nothing of the extended decoder, so it also runs against an older build of the library.

Kernel times come from a separate run:  rocprofv3 --kernel-trace --stats -- python tools/pngdecodebench.py --gpu-only
"""
import argparse
import io
import json
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lars_image_processing_amd as lars  # noqa: E402
from lars_image_processing_amd import _ffi  # noqa: E402
from thumbbench import SIZE, gallery, per_call_ms, pillow_ms  # noqa: E402


def colormap_pictures(n=2, side=4096, seed=3):
    """RGBA colormap pictures of smooth index fields (what the batch driver writes)."""
    rng = np.random.default_rng(seed)
    lut = lars.colormap_lut("RdYlGn")
    out = []
    for k in range(n):
        y, x = np.mgrid[0:side, 0:side].astype(np.float32) / side
        f = np.sin(6 * x + k) * np.cos(5 * y - k) + 0.1 * rng.standard_normal((side, side)).astype(np.float32)
        idx = np.clip((f + 1.2) / 2.4 * 255, 0, 255).astype(np.uint8)
        out.append(np.ascontiguousarray(lut[idx]))
    return out


def pil_png(a, **save):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG", **save)
    return b.getvalue()


def pil_decode(b):
    im = Image.open(io.BytesIO(b))
    im.load()
    return im


def pil_thumb(b):
    im = Image.open(io.BytesIO(b))
    im.thumbnail(SIZE, Image.Resampling.LANCZOS)
    return im


def variant_files():
    """{kind: (files, colour type, depth)} of the variants leg."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import png_variant_writer as W
    rng = np.random.default_rng(11)
    pics = gallery()[:4]
    wide = [(a.astype(np.uint16) << 8) | rng.integers(0, 256, a.shape, dtype=np.uint16) for a in pics]       # noisy low bytes, as a sensor's
    side = 4096
    y, x = np.mgrid[0:side, 0:side].astype(np.float32) / side
    pal = [np.clip((np.sin(6 * x + k) * np.cos(5 * y - k) + 1.0) * 8, 0, 15).astype(np.uint8) for k in range(2)]
    # Paeth on every row for samples of a byte or more, none for the packed palette rows (libpng's own choice for those)
    return {
        "rgb_2048x1536_interlaced": [W.write_png(a, 2, 8, True, filters=4) for a in pics],
        "i16_2048x1536": [W.write_png(a[:, :, 1], 0, 16, False, filters=4) for a in wide],
        "rgb16_2048x1536": [W.write_png(a, 2, 16, False, filters=4) for a in wide],
        "palette4_4096x4096": [W.write_png(a, 3, 4, False, filters=0) for a in pal],
    }


def gallery_leg(args):
    files = [pil_png(a) for a in gallery()]
    for b in files[:2]:
        assert lars.decode_png(b).tobytes() == np.asarray(Image.open(io.BytesIO(b))).tobytes()
    r = {"files": len(files), "mean_file_bytes": int(np.mean([len(b) for b in files])),
         "decode_png_ms": [per_call_ms(lars.decode_png, files, args.reps) for _ in range(2)]}                 # two runs: their spread
    if not args.gpu_only:
        r["pillow_load_ms"] = pillow_ms(pil_decode, files, args.reps)
    print("gallery_rgb_pillow_default", json.dumps(r), flush=True)
    return r


def variants(args):
    res = {"device": _ffi.device_name(), "reps": args.reps, "kinds": {"gallery_rgb_pillow_default": gallery_leg(args)}}
    if not args.gallery_only:
        def decode(b):
            return lars.decode_png(b, extended=True)
        for name, files in variant_files().items():
            for b in files[:2]:                               # a fast wrong answer is no answer
                want = np.asarray(Image.open(io.BytesIO(b)))
                got = decode(b)
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
            r = {"files": len(files), "mean_file_bytes": int(np.mean([len(b) for b in files])), "shape": list(want.shape),
                 "dtype": str(want.dtype), "decode_png_extended_ms": per_call_ms(decode, files, args.reps)}
            if not args.gpu_only:
                r["pillow_load_ms"] = pillow_ms(pil_decode, files, args.reps)
                r["decode_speedup"] = r["pillow_load_ms"] / r["decode_png_extended_ms"]
            res["kinds"][name] = r
            print(name, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="skip the Pillow legs (for a kernel trace)")
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--variants", action="store_true", help="the extended decoder's leg: interlaced, 16-bit and 4-bit files, and the 8-bit gallery")
    ap.add_argument("--gallery-only", action="store_true", help="of --variants, the 8-bit gallery leg alone")
    args = ap.parse_args()
    if _ffi.device_count() < 1:
        sys.exit("pngdecodebench: needs a gfx950 GPU (no CPU fallback)")
    if args.variants or args.gallery_only:
        return variants(args)
    maps = colormap_pictures()
    kinds = {
        "gallery_rgb_pillow_default": [pil_png(a) for a in gallery()],
        "colormap_4096_rgba_pillow_level1": [pil_png(a, compress_level=1) for a in maps],
        "colormap_4096_rgba_encode_png": [lars.encode_png(a) for a in maps],
    }
    res = {"device": _ffi.device_name(), "reps": args.reps, "size": list(SIZE), "kinds": {}}
    for name, files in kinds.items():
        for b in files[:2]:                                   # a fast wrong answer is no answer
            assert lars.decode_png(b).tobytes() == np.asarray(Image.open(io.BytesIO(b))).tobytes()
            assert lars.thumbnail_png(b).tobytes() == np.asarray(pil_thumb(b)).tobytes()
        r = {"files": len(files), "mean_file_bytes": int(np.mean([len(b) for b in files])),
             "shape": list(np.asarray(Image.open(io.BytesIO(files[0]))).shape),
             "decode_png_ms": per_call_ms(lars.decode_png, files, args.reps),
             "thumbnail_png_ms": per_call_ms(lars.thumbnail_png, files, args.reps)}
        if not args.gpu_only:
            r["pillow_load_ms"] = pillow_ms(pil_decode, files, args.reps)
            r["pillow_thumbnail_ms"] = pillow_ms(pil_thumb, files, args.reps)
            r["decode_speedup"] = r["pillow_load_ms"] / r["decode_png_ms"]
            r["thumbnail_speedup"] = r["pillow_thumbnail_ms"] / r["thumbnail_png_ms"]
        res["kinds"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
