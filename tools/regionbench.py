#!/usr/bin/env python3
"""Zones from regions (label_regions and Regions, csrc/regions.hip) next to scipy.ndimage.label on the host.

Masks, per size (2048 x 1536 and 4096 x 4096): ``field`` a 1/f random field above its mean (blobs of every size, half the raster),
``grid`` 2000 rectangular plots on about 60 % of the raster, ``noise`` independent pixels at density 0.05.  The picture of the
picture legs is the seeded vegetation-like uint8 RGNir image of tools/zonebench.py; its zones are the patches of NDVI above 0.2 with
64 pixels or more (the speckle below that is tens of thousands of regions nobody wants a row for).

Three groups of legs alternate ``--rounds`` times in one process; every timed call returns after a device synchronise, a time is
the median over ``--reps`` calls after a warm-up call, a figure the median of the rounds' medians with the rounds kept:

  label      label_regions(mask)  next to  scipy.ndimage.label(mask, ones((3, 3))) on the same mask: upload, kernels and the labels'
             download on one side, the host's serial pass on the other.  The two label rasters are compared before they are timed.
  picture    process_image_zones(img, Regions(index="NDVI", above=0.2, min_pixels=64))  next to  the same call on a label raster
             made beforehand: what making the labels on the device costs on top of a call that gets them for nothing
  chain      process_image(img), then scipy's labelling of NDVI > 0.2 with the small regions dropped, then
             process_image_zones(img, labels): what a caller does today, next to ``picture``'s first leg

``--hard`` adds, per size, the ``label`` legs on masks built to be hard for the device -- ``full`` (one region, every seam joins the
same two roots), ``serpentine`` (one region that winds through every tile row), ``comb`` (teeth that merge in the last row) and
``checkerboard`` (under connectivity 4 every foreground pixel a region of its own: half the raster in table rows) -- under both
connectivities.

    python tools/regionbench.py [--sizes 2048x1536,4096x4096] [--reps 5] [--rounds 3] [--hard] [--json profiles/regions.json]

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/regionbench.py --label-only --sizes 4096x4096
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lars_image_processing_amd import _ffi  # noqa: E402

MASKS = ("field", "grid", "noise")
HARD_MASKS = ("full", "serpentine", "comb", "checkerboard")
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
MIN_PIXELS = 64
FULL = np.ones((3, 3), dtype=int)


def picture(h, w):
    from oracle import index_oracle as orc
    return np.ascontiguousarray(orc.synth_tile_u8(99, 0, h, w, profile="vegetation"))


def mask_of(kind, h, w):
    import regions_cases as gc
    if kind == "field":
        return gc.thresholded_field(h, w)
    if kind == "noise":
        return gc.random_mask(h, w, 0.05, 17)
    if kind == "full":
        return np.ones((h, w), dtype=bool)
    if kind in ("serpentine", "comb"):
        return getattr(gc, kind)(h, w)
    if kind == "checkerboard":
        y, x = np.mgrid[0:h, 0:w]
        return (x + y) % 2 == 0
    y, x = np.mgrid[0:h, 0:w]                                          # zonebench's plots
    ny, nx, side = 40, 50, 0.6 ** 0.5
    cy, cx = y * ny // h, x * nx // w
    return ((y - cy * h / ny) < side * h / ny) & ((x - cx * w / nx) < side * w / nx)


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def alternate(legs, reps, rounds):
    times = {name: [] for name in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(median_ms(fn, reps))
    return times


def summary(rounds):
    return {"ms": float(np.median(rounds)), "rounds": rounds, "spread": (max(rounds) - min(rounds)) / float(np.median(rounds))}


def host_labels(plane, ndimage):
    """scipy's labels of NDVI > 0.2 with the regions below MIN_PIXELS dropped and the rest renumbered in order."""
    lab, n = ndimage.label(plane > np.float32(0.2), structure=FULL)
    keep = np.bincount(lab.ravel(), minlength=n + 1)[1:] >= MIN_PIXELS
    remap = np.concatenate(([0], np.cumsum(keep) * keep)).astype(np.int32)
    return remap[lab], int(keep.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2048x1536,4096x4096", help="WIDTHxHEIGHT, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hard", action="store_true", help="also the label legs on the masks built to be hard, under both connectivities")
    ap.add_argument("--label-only", action="store_true", help="label_regions alone, twice per mask after a warm-up (for a kernel trace)")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    import lars_image_processing_amd as lars
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    print("device:", _ffi.device_name(), flush=True)
    out = {"device": _ffi.device_name(), "reps": args.reps, "rounds": args.rounds, "scipy": ndimage is not None, "min_pixels_of_the_picture_legs": MIN_PIXELS,
           "sizes": {}}
    for w, h in [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]:
        size_row = {"pixels": h * w, "label": {}}
        for kind in MASKS:
            mask = mask_of(kind, h, w)
            got = lars.label_regions(mask)
            row = {"n_regions": got["n_regions"], "foreground": float(mask.mean()), "label_type": str(got["labels"].dtype)}
            if args.label_only:
                for _ in range(2):
                    lars.label_regions(mask)
                size_row["label"][kind] = row
                continue
            legs = {"device": lambda: lars.label_regions(mask)}
            if ndimage is not None:
                want, n = ndimage.label(mask, structure=FULL)
                assert n == got["n_regions"] and np.array_equal(got["labels"], want)      # the timed calls agree
                del want
                legs["scipy"] = lambda: ndimage.label(mask, structure=FULL)
            del got
            for name, rounds in alternate(legs, args.reps, args.rounds).items():
                row[name] = summary(rounds)
            if ndimage is not None:
                row["scipy_over_device"] = row["scipy"]["ms"] / row["device"]["ms"]
            size_row["label"][kind] = row
            print(f"{w}x{h} label {kind}", json.dumps(row), flush=True)
        for kind, connectivity in [(k, c) for k in HARD_MASKS for c in (8, 4)] if args.hard and not args.label_only else []:
            mask = mask_of(kind, h, w)
            got = lars.label_regions(mask, connectivity=connectivity)
            row = {"n_regions": got["n_regions"], "label_type": str(got["labels"].dtype)}
            legs = {"device": lambda: lars.label_regions(mask, connectivity=connectivity)}
            if ndimage is not None:
                structure = FULL if connectivity == 8 else CROSS
                want, n = ndimage.label(mask, structure=structure)
                assert n == got["n_regions"] and np.array_equal(got["labels"], want)
                del want
                legs["scipy"] = lambda: ndimage.label(mask, structure=structure)
            del got
            for name, rounds in alternate(legs, args.reps, args.rounds).items():
                row[name] = summary(rounds)
            if ndimage is not None:
                row["scipy_over_device"] = row["scipy"]["ms"] / row["device"]["ms"]
            size_row.setdefault("hard", {})[f"{kind}-{connectivity}"] = row
            print(f"{w}x{h} hard {kind} connectivity {connectivity}", json.dumps(row), flush=True)
        if not args.label_only:
            img = picture(h, w)
            regions = lars.Regions(index="NDVI", above=0.2, min_pixels=MIN_PIXELS, max_regions=65535)
            made = lars.process_image_zones(img, lars.Regions(index="NDVI", above=0.2, min_pixels=MIN_PIXELS, max_regions=65535, want_labels=True))
            lab, nz = made["zones"]["labels"], len(made["zones"]["zone"])
            row = {"n_regions": nz, "label_type": str(lab.dtype)}
            legs = {"regions": lambda: lars.process_image_zones(img, regions),
                    "labels": lambda: lars.process_image_zones(img, lab, n_zones=nz)}
            if ndimage is not None:
                host, n = host_labels(made["indices"]["NDVI"]["index"], ndimage)
                assert n == nz and np.array_equal(host, lab)                               # the chain computes the same zones

                def chain():
                    first = lars.process_image(img)
                    mine, count = host_labels(first["indices"]["NDVI"]["index"], ndimage)
                    return lars.process_image_zones(img, mine, n_zones=count)
                legs["chain"] = chain
                del host
            del made
            for name, rounds in alternate(legs, args.reps, args.rounds).items():
                row[name] = summary(rounds)
            row["regions_over_labels"] = row["regions"]["ms"] / row["labels"]["ms"]
            if ndimage is not None:
                row["chain_over_regions"] = row["chain"]["ms"] / row["regions"]["ms"]
            size_row["picture"] = row
            print(f"{w}x{h} picture", json.dumps(row), flush=True)
        out["sizes"][f"{w}x{h}"] = size_row
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
