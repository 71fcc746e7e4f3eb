#!/usr/bin/env python3
"""Zone margins (process_image_zones(img, Shrunk(zones, m)), csrc/zone_margin.hip) next to the call without a margin and next to what a caller
did before: labels down, one distance transform per zone on the host, labels up again.

Pictures and rules are tools/zonebench.py's: seeded vegetation-like uint8 RGNir images of 2048 x 1536 and 4096 x 4096, the three
indices with their statistics and float32 planes and the corrected image plus one row per zone and index, host arrays in and out,
every call returns after a device synchronise.  Zone layouts, as polygons packed once beforehand: ``plots`` 2000 rotated four-vertex
plots on about 60 % of the raster, ``large`` 40 rotated zones, ``one`` a single zone over the whole raster.  Margins 2, 8, 32, 128
and 254 pixels.  Per size, layout and margin, after a warm-up call, the median over ``--reps`` host call times, the legs alternating
``--rounds`` times in one process (median of the rounds' medians, the rounds kept), of

  margin      process_image_zones(img, Shrunk(polygons, m))
  plain       process_image_zones(img, polygons): margin / plain is the cost of the feature
  host        rasterize_zones(polygons, shape), then scipy.ndimage.distance_transform_edt of each zone on the host -- done well: on
              the zone's box with floor(m) + 1 pixels around it, the raster's edge no border, a zone that fills its box left alone --
              then process_image_zones(img, eroded raster): what a caller does today.  ``--host-reps`` calls a round, no warm-up of
              their own.
  shrink      shrink_zones(polygons, m, shape) alone (labels downloaded), for the share of the two kernels

The eroded raster of ``host`` is held against ``shrink_zones``'s before anything is timed.  ``--parent-lib PATH`` measures the calls
without a margin (process_image, process_image_masked, process_image_zones with a label raster and with polygons) in fresh child
processes, alternating between this build's library and the parent commit's.

    python tools/marginbench.py [--sizes 2048x1536,4096x4096] [--margins 2,8,32,128,254] [--layouts plots,large,one] [--reps 7]
                                [--rounds 3] [--host-reps 1] [--parent-lib PATH] [--json out.json]

Kernel times come from a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/marginbench.py --margin-only --sizes 4096x4096
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zonebench as zb  # noqa: E402
from lars_image_processing_amd import _ffi  # noqa: E402

LAYOUTS = ("plots", "large", "one")
DEFAULT_CALLS = ("unmasked", "masked", "zones", "polygons")


def polygons_of(layout, h, w):
    if layout == "one":
        return [np.array([(-1.0, -1.0), (w + 1.0, -1.0), (w + 1.0, h + 1.0), (-1.0, h + 1.0)])]
    return zb.polygons_of(layout, h, w)


def host_shrink(labels, margin):
    """What a caller does today, done well: one exact distance transform per zone, on the zone's box and what the margin can reach."""
    from scipy.ndimage import distance_transform_edt, find_objects
    pad = int(margin) + 1
    h, w = labels.shape
    out = labels.copy()
    for z, box in enumerate(find_objects(labels), start=1):
        if box is None:
            continue
        rows = slice(max(0, box[0].start - pad), min(h, box[0].stop + pad))
        cols = slice(max(0, box[1].start - pad), min(w, box[1].stop + pad))
        inside = labels[rows, cols] == z
        if inside.all():                                           # nothing differs within reach: the transform has no zero to measure from
            continue
        away = distance_transform_edt(inside)
        out[rows, cols][inside & (away <= margin)] = 0
    return out


def host_ms(fn, reps):
    """The median of ``reps`` calls without a warm-up of their own: the device is warm from the other legs, and the host's share
    takes seconds."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def child(args):
    """The calls without a margin alone, on the library LARS_HIP_LIB names; what that library does not export is not bound (the
    parent's lacks the margin entry points)."""
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in [n for n in _ffi.SIGNATURES if not hasattr(lib, n)]:
        del _ffi.SIGNATURES[name]
    import lars_image_processing_amd as lars
    out = {}
    for w, h in zb.sizes_of(args.sizes):
        img = zb.picture(h, w)
        ones = np.ones((h, w), dtype=bool)
        lab, nz = zb.labels("plots", h, w)
        packed = lars.Polygons(polygons_of("plots", h, w))
        out[f"{w}x{h}"] = {"unmasked": zb.median_ms(lambda: lars.process_image(img), args.reps),
                           "masked": zb.median_ms(lambda: lars.process_image_masked(img, valid=ones), args.reps),
                           "zones": zb.median_ms(lambda: lars.process_image_zones(img, lab, n_zones=nz), args.reps),
                           "polygons": zb.median_ms(lambda: lars.process_image_zones(img, packed), args.reps)}
    print("CHILD " + json.dumps(out), flush=True)


def run_child(lib, args):
    env = dict(os.environ)
    if lib:
        env["LARS_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--sizes", args.sizes, "--reps", str(args.reps)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"child ({lib or 'this build'}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2048x1536,4096x4096", help="WIDTHxHEIGHT, comma separated")
    ap.add_argument("--margins", default="2,8,32,128,254", help="pixels, comma separated")
    ap.add_argument("--layouts", default=",".join(LAYOUTS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1, help="calls of the host leg per round (it takes seconds)")
    ap.add_argument("--parent-lib", help="liblars_hip.so built from the parent commit")
    ap.add_argument("--margin-only", action="store_true", help="the margin call alone, twice per case after a warm-up (for a kernel trace)")
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import lars_image_processing_amd as lars
    print("device:", _ffi.device_name(), flush=True)
    margins = [float(m) for m in args.margins.split(",")]
    out = {"device": _ffi.device_name(), "reps": args.reps, "rounds": args.rounds, "host_reps": args.host_reps,
           "request": "three indices, statistics, float32 planes, corrected image; one row per zone and index", "sizes": {}}
    for w, h in zb.sizes_of(args.sizes):
        img = zb.picture(h, w)
        size_row = {"pixels": h * w, "layouts": {}}
        for layout in args.layouts.split(","):
            packed = lars.Polygons(polygons_of(layout, h, w))
            nz = len(packed)
            raster = lars.rasterize_zones(packed, (h, w))
            layout_row = {"zones": nz, "label_type": str(raster.dtype), "covered": float(np.count_nonzero(raster) / raster.size), "margins": {}}
            for m in margins:
                if args.margin_only:
                    for _ in range(3):
                        lars.process_image_zones(img, lars.Shrunk(packed, m))
                    continue
                shrunk = lars.shrink_zones(packed, m, shape=(h, w))
                assert host_shrink(raster, m).tobytes() == shrunk.tobytes(), (layout, m)       # the two ways agree before they are timed
                row = {"kept": float(np.count_nonzero(shrunk) / max(1, np.count_nonzero(raster)))}

                def host():
                    return lars.process_image_zones(img, host_shrink(lars.rasterize_zones(packed, (h, w)), m), n_zones=nz)
                legs = {"margin": lambda: lars.process_image_zones(img, lars.Shrunk(packed, m)),
                        "plain": lambda: lars.process_image_zones(img, packed),
                        "shrink": lambda: lars.shrink_zones(packed, m, shape=(h, w))}
                times = {name: [] for name in (*legs, "host")}
                for _ in range(args.rounds):
                    for name, fn in legs.items():
                        times[name].append(zb.median_ms(fn, args.reps))
                    times["host"].append(host_ms(host, args.host_reps))
                for name, rounds in times.items():
                    row[name] = zb.summary(rounds)
                row["margin_over_plain"] = row["margin"]["ms"] / row["plain"]["ms"]
                row["host_over_margin"] = row["host"]["ms"] / row["margin"]["ms"]
                a, b = lars.process_image_zones(img, lars.Shrunk(packed, m)), lars.process_image_zones(img, shrunk, n_zones=nz)   # the timed calls agree
                assert np.array_equal(a["zones"]["pixels"], b["zones"]["pixels"])
                for t in ("NDVI", "GNDVI", "NDWI"):
                    assert np.array_equal(a["zones"][t]["median"], b["zones"][t]["median"], equal_nan=True)
                del a, b
                layout_row["margins"][f"{m:g}"] = row
                print(f"{w}x{h} {layout} margin {m:g}", json.dumps(row), flush=True)
            size_row["layouts"][layout] = layout_row
        out["sizes"][f"{w}x{h}"] = size_row
    if args.parent_lib and not args.margin_only:
        rounds = {"this_lib": [], "parent_lib": []}
        for _ in range(args.rounds):
            rounds["this_lib"].append(run_child(None, args))
            rounds["parent_lib"].append(run_child(os.path.abspath(args.parent_lib), args))
        for key, size_row in out["sizes"].items():
            cmp_row = {}
            for call in DEFAULT_CALLS:
                for which, runs in rounds.items():
                    cmp_row[f"{which}_{call}"] = zb.summary([r[key][call] for r in runs])
                cmp_row[f"this_over_parent_{call}"] = cmp_row[f"this_lib_{call}"]["ms"] / cmp_row[f"parent_lib_{call}"]["ms"]
            size_row["default_calls"] = cmp_row
            print(key, "default calls", json.dumps(cmp_row), flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
