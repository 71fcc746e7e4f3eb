#!/usr/bin/env python3
"""Zonal statistics (process_image_zones, csrc/zonal.hip) next to the calls without zones.

Pictures: seeded vegetation-like uint8 RGNir images (oracle.index_oracle.synth_tile_u8) of 2048 x 1536 and 4096 x 4096.  Zone
layouts: ``plots`` 2000 rectangular plots (50 x 40) that cover about 60 % of the raster, uint16 labels; ``large`` 40 zones (8 x
5) that cover all of it, uint8; ``one`` a single zone everywhere, uint8.  Request: the three indices with their statistics and
float32 planes and the corrected image, plus one row per zone and index.  Per size and layout, after a warm-up call, the median
over ``--reps`` host call times (upload, kernels, downloads; every call returns after a device synchronise), the legs
alternating ``--rounds`` times in one process (median of the rounds' medians, the rounds kept), of

  zones       process_image_zones(img, labels)
  masked      process_image_masked(img, valid=all ones): the same route without zones -- zones / masked is the cost of the feature
  unmasked    process_image(img)
  numpy       the NumPy model done well (tests/zonal_model.py: one stable argsort of the labels, then a split), the zone part
              alone on planes that already exist, once
  loop        ``plots`` at 2048 x 1536 only: process_image_masked(valid=labels == z) for 20 of the plots, times Z / 20 --
              an extrapolation, labelled as such (and the wrong white balance: the plot's, not the picture's)

``--sweep`` times the zones call on ``large`` and ``one`` with the knob zone_split_pixels at every power of two from 2^10 to
2^24 and at 2^30 (no zone is split), the same alternation, and reports per layout each value's time over the best and the spread
of the rounds.  ``--parent-lib PATH`` measures process_image, process_image_masked and process_image_zones with a label raster
(``plots``) in fresh child processes, alternating between this build's library and the parent commit's.

``--polygons`` times the zones made from outlines (csrc/zone_raster.hip) instead, by the same rules.  Layouts: ``plots`` 2000 rotated
four-vertex plots on about 60 % of the raster, ``large`` 40 rotated zones, ``outline`` one polygon of 10 000 vertices over most of the
raster.  Legs:

  polygons    process_image_zones(img, polygons): the list is checked and packed on the host in every call
  packed      process_image_zones(img, Polygons(polygons)) with the packing done once beforehand, as a time series would
  labels      process_image_zones(img, labels) with the labels made beforehand: the call before this feature, and a floor that
              polygons cannot beat by more than the saved upload
  pillow      what a caller without GDAL does today: an ImageDraw.polygon loop into an I;16 image, then ``labels``.  Timing only:
              Pillow paints the edge pixels of both neighbours, its raster is not the definition's
  rasterize   rasterize_zones(polygons, shape) alone (labels downloaded), for the share of the rasteriser

``--layouts ring_thin`` / ``ring_full`` (with ``--zones-only``, under the kernel trace) give the share of the label writes in k_zr_fill.

    python tools/zonebench.py [--sizes 2048x1536,4096x4096] [--reps 7] [--rounds 3] [--sweep] [--polygons] [--parent-lib PATH] [--json out.json]

Kernel times come from a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/zonebench.py --zones-only --sizes 4096x4096
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lars_image_processing_amd import _ffi  # noqa: E402

POLYGON_SYMBOLS = ("lars_zone_rasterize_scratch_bytes", "lars_d_zone_rasterize", "lars_d_zone_labels_narrow", "lars_h_rasterize_zones",
                   "lars_h_zonal_stats_polygons_f32", "lars_h_process_image_zones_polygons")
LAYOUTS = ("plots", "large", "one")
POLYGON_LAYOUTS = ("plots", "large", "outline")
SWEEP = [2 ** k for k in range(10, 25)] + [2 ** 30]


def picture(h, w):
    from oracle import index_oracle as orc
    return np.ascontiguousarray(orc.synth_tile_u8(99, 0, h, w, profile="vegetation"))


def labels(layout, h, w):
    y, x = np.mgrid[0:h, 0:w]
    if layout == "plots":
        ny, nx, side = 40, 50, 0.6 ** 0.5
        cy, cx = y * ny // h, x * nx // w
        inside = ((y - cy * h / ny) < side * h / ny) & ((x - cx * w / nx) < side * w / nx)
        return np.where(inside, cy * nx + cx + 1, 0).astype(np.uint16), ny * nx
    if layout == "large":
        return ((y * 5 // h) * 8 + x * 8 // w + 1).astype(np.uint8), 40
    return np.ones((h, w), dtype=np.uint8), 1


def rotated_grid(ny, nx, h, w, fill, angle):
    """``ny * nx`` rectangles of ``fill`` of their cell's area, turned by ``angle`` about the raster's centre (some end up cut by the border)."""
    side = fill ** 0.5
    cy, cx = np.mgrid[0:ny, 0:nx]
    y0, x0 = cy.ravel() * h / ny, cx.ravel() * w / nx
    corners = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)])
    x = x0[:, None] + corners[:, 0] * side * w / nx - w / 2
    y = y0[:, None] + corners[:, 1] * side * h / ny - h / 2
    c, s = np.cos(angle), np.sin(angle)
    return list(np.stack((x * c - y * s + w / 2, x * s + y * c + h / 2), axis=2))


def polygons_of(layout, h, w):
    if layout == "plots":
        return rotated_grid(40, 50, h, w, 0.6, np.radians(7.0))
    if layout == "large":
        return rotated_grid(5, 8, h, w, 0.9, np.radians(7.0))
    k = np.arange(10000)                                       # a wavy outline over most of the raster
    a = k * (2 * np.pi / 10000)
    r = 0.46 + 0.03 * np.sin(37 * a)
    outline = np.stack((w / 2 + r * w * np.cos(a), h / 2 + r * h * np.sin(a)), axis=1)
    if layout == "outline":
        return [outline]
    # the outline with a hole: the same edges, rows and words for the kernel, but few (ring_thin) or nearly all (ring_full) of the
    # pixels written -- the difference of their kernel times is the time of the atomicMax writes
    scale = {"ring_thin": 0.98, "ring_full": 0.02}[layout]
    centre = np.array((w / 2, h / 2))
    return [[outline, centre + (outline - centre) * scale]]


def pillow_labels(polygons, h, w):
    from PIL import Image, ImageDraw
    im = Image.new("I;16", (w, h), 0)
    draw = ImageDraw.Draw(im)
    for k, p in enumerate(polygons):
        draw.polygon([tuple(v) for v in p], fill=k + 1)
    return np.asarray(im)


def polygon_legs(lars, args, out):
    for w, h in sizes_of(args.sizes):
        img = picture(h, w)
        size_row = {"pixels": h * w, "layouts": {}}
        for layout in (args.layouts.split(",") if args.layouts else POLYGON_LAYOUTS):
            polys = polygons_of(layout, h, w)
            packed = lars.Polygons(polys)
            lab = lars.rasterize_zones(packed, (h, w))
            nz = len(polys)
            row = {"zones": nz, "vertices": int(len(packed.verts)), "label_type": str(lab.dtype), "covered": float(np.count_nonzero(lab) / lab.size)}
            if args.zones_only:
                for _ in range(2):
                    lars.process_image_zones(img, packed)
                size_row["layouts"][layout] = row
                continue
            legs = {"polygons": lambda: lars.process_image_zones(img, polys),
                    "packed": lambda: lars.process_image_zones(img, packed),
                    "labels": lambda: lars.process_image_zones(img, lab, n_zones=nz),
                    "pillow": lambda: lars.process_image_zones(img, pillow_labels(polys, h, w), n_zones=nz),
                    "rasterize": lambda: lars.rasterize_zones(packed, (h, w))}
            for name, rounds in alternate(legs, args.reps, args.rounds).items():
                row[name] = summary(rounds)
            row["polygons_over_labels"] = row["polygons"]["ms"] / row["labels"]["ms"]
            row["packed_over_labels"] = row["packed"]["ms"] / row["labels"]["ms"]
            row["pillow_over_polygons"] = row["pillow"]["ms"] / row["polygons"]["ms"]
            row["pillow_differs_in_pixels"] = int(np.count_nonzero(pillow_labels(polys, h, w) != lab))
            a, b = lars.process_image_zones(img, packed), lars.process_image_zones(img, lab, n_zones=nz)     # the timed calls agree
            assert np.array_equal(a["zones"]["pixels"], b["zones"]["pixels"])
            for t in ("NDVI", "GNDVI", "NDWI"):
                assert np.array_equal(a["zones"][t]["median"], b["zones"][t]["median"], equal_nan=True)
            del a, b
            size_row["layouts"][layout] = row
            print(f"{w}x{h} polygons {layout}", json.dumps(row), flush=True)
        out["sizes"][f"{w}x{h}"] = size_row


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def alternate(legs, reps, rounds):
    """{name: [one median per round]}: the legs take turns, so none of them always runs on the colder heap; no result is kept
    alive while another call is timed."""
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(median_ms(fn, reps))
    return times


def sizes_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",")]


def child(args):
    """The calls that exist on both sides alone, on the library LARS_HIP_LIB names (the parent's lacks the polygon entry points)."""
    if args.child == "parent":
        for name in POLYGON_SYMBOLS:
            _ffi.SIGNATURES.pop(name, None)
    import lars_image_processing_amd as lars
    out = {}
    for w, h in sizes_of(args.sizes):
        img = picture(h, w)
        ones = np.ones((h, w), dtype=bool)
        lab, nz = labels("plots", h, w)
        out[f"{w}x{h}"] = {"unmasked": median_ms(lambda: lars.process_image(img), args.reps),
                           "masked": median_ms(lambda: lars.process_image_masked(img, valid=ones), args.reps),
                           "zones": median_ms(lambda: lars.process_image_zones(img, lab, n_zones=nz), args.reps)}
    print("CHILD " + json.dumps(out), flush=True)


def run_child(which, lib, args):
    env = dict(os.environ)
    if lib:
        env["LARS_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--sizes", args.sizes, "--reps", str(args.reps)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"child ({which}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])


def summary(rounds):
    return {"ms": float(np.median(rounds)), "rounds": rounds, "spread": (max(rounds) - min(rounds)) / float(np.median(rounds))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2048x1536,4096x4096", help="WIDTHxHEIGHT, comma separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", action="store_true", help="also time zone_split_pixels at every power of two on the layouts large and one")
    ap.add_argument("--polygons", action="store_true", help="the legs of the zones made from polygons instead of the label-raster layouts")
    ap.add_argument("--layouts", help="with --polygons: these layouts only, comma separated (also ring_thin, ring_full: see polygons_of)")
    ap.add_argument("--parent-lib", help="liblars_hip.so built from the parent commit")
    ap.add_argument("--zones-only", action="store_true", help="the zones call alone, once per layout after a warm-up (for a kernel trace)")
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--child", choices=["this", "parent"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import lars_image_processing_amd as lars
    import masked_model as mm
    import zonal_model as zm
    print("device:", _ffi.device_name(), flush=True)
    out = {"device": _ffi.device_name(), "reps": args.reps, "rounds": args.rounds, "zone_split_pixels": _ffi.get_tuning("zone_split_pixels"),
           "request": "three indices, statistics, float32 planes, corrected image; one row per zone and index", "sizes": {}}
    if args.polygons:
        polygon_legs(lars, args, out)
    for w, h in ([] if args.polygons else sizes_of(args.sizes)):
        img = picture(h, w)
        ones = np.ones((h, w), dtype=bool)
        size_row = {"pixels": h * w, "layouts": {}}
        for layout in LAYOUTS:
            lab, nz = labels(layout, h, w)
            row = {"zones": nz, "label_type": str(lab.dtype), "covered": float(np.count_nonzero(lab) / lab.size)}
            if args.zones_only:
                for _ in range(2):
                    lars.process_image_zones(img, lab, n_zones=nz)
                size_row["layouts"][layout] = row
                continue
            legs = {"zones": lambda: lars.process_image_zones(img, lab, n_zones=nz),
                    "masked": lambda: lars.process_image_masked(img, valid=ones),
                    "unmasked": lambda: lars.process_image(img)}
            for name, rounds in alternate(legs, args.reps, args.rounds).items():
                row[name] = summary(rounds)
            row["zones_over_masked"] = row["zones"]["ms"] / row["masked"]["ms"]
            res = lars.process_image_zones(img, lab, n_zones=nz, want_hist=True)
            planes = {t: res["indices"][t]["index"] for t in mm.INDEX_NAMES}
            t0 = time.perf_counter()
            want = {t: zm.zonal_model(planes[t], lab, t, None, nz) for t in mm.INDEX_NAMES}
            row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            row["numpy_over_zone_part"] = row["numpy_ms"] / max(row["zones"]["ms"] - row["masked"]["ms"], 1e-3)
            for t in mm.INDEX_NAMES:                     # the timed call computes the model's numbers
                zm.check_zone_figures({"zone": res["zones"]["zone"], "pixels": res["zones"]["pixels"], **res["zones"][t]}, want[t], t)
            del res, want, planes
            if layout == "plots" and (w, h) == (2048, 1536):
                some = np.linspace(1, nz, 20).astype(int)
                t0 = time.perf_counter()
                for z in some:
                    lars.process_image_masked(img, valid=lab == z)
                row["loop_20_plots_ms"] = (time.perf_counter() - t0) * 1e3
                row["loop_extrapolated_ms"] = row["loop_20_plots_ms"] * nz / 20
                row["loop_extrapolated_over_zones"] = row["loop_extrapolated_ms"] / row["zones"]["ms"]
            size_row["layouts"][layout] = row
            print(f"{w}x{h} {layout}", json.dumps(row), flush=True)
        if args.sweep and not args.zones_only:
            sweep = {}
            for layout in ("large", "one"):
                lab, nz = labels(layout, h, w)
                times = {v: [] for v in SWEEP}
                for _ in range(args.rounds):
                    for v in SWEEP:
                        with _ffi.tuning(zone_split_pixels=v):
                            times[v].append(median_ms(lambda: lars.process_image_zones(img, lab, n_zones=nz), args.reps))
                best = min(float(np.median(r)) for r in times.values())
                sweep[layout] = {str(v): {**summary(r), "over_best": float(np.median(r)) / best} for v, r in times.items()}
                print(f"{w}x{h} sweep {layout}", {v: round(s["ms"], 2) for v, s in sweep[layout].items()}, flush=True)
            size_row["sweep"] = sweep
        out["sizes"][f"{w}x{h}"] = size_row
    if args.parent_lib and not args.zones_only:
        rounds = {"this_lib": [], "parent_lib": []}
        for _ in range(args.rounds):
            rounds["this_lib"].append(run_child("this", None, args))
            rounds["parent_lib"].append(run_child("parent", os.path.abspath(args.parent_lib), args))
        for key, size_row in out["sizes"].items():
            cmp_row = {}
            for call in ("unmasked", "masked", "zones"):
                for which, runs in rounds.items():
                    cmp_row[f"{which}_{call}"] = summary([r[key][call] for r in runs])
                cmp_row[f"this_over_parent_{call}"] = cmp_row[f"this_lib_{call}"]["ms"] / cmp_row[f"parent_lib_{call}"]["ms"]
            size_row["default_calls"] = cmp_row
            print(key, "default calls", json.dumps(cmp_row), flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
