#!/usr/bin/env python3
"""Region outlines (region_outlines, csrc/outlines.hip) next to label_regions, by the rules of tools/regionbench.py: host arrays in and
out, the legs alternate ``--rounds`` times in one process, a time is the median over ``--reps`` calls after a warm-up call, every call
returns after a device synchronise, a figure is the median of the rounds' medians with the rounds kept.

Masks: regionbench's three ordinary ones per size (``field``, ``grid``, ``noise``) and, with ``--hard``, its four hard ones under both
connectivities.  The checkerboard under connectivity 4 (every other pixel a region: at 4096 x 4096 8.4 M rings, 33 M vertices) is left out
unless ``--checkerboard-4`` asks for it.

  outlines   region_outlines(mask)  next to  label_regions(mask) on the same mask: what the outlines cost on top of the labels.  The
             traced rings are rasterised again (rasterize_zones) and compared with the labels before anything is timed, where the regions
             are 65535 or fewer and the vertices 2**24 or fewer.
  contourpy  timing only, on the ordinary masks, where contourpy is installed: its lines at level 0.5 of the foreground of the same labels.  Its
             contours run between pixel centres, cut corners and know no labels: another shape, what a caller without a crack tracer has.
  default    with ``--parent-lib PATH`` (a liblars_hip.so built from the parent commit): label_regions(mask) on the field mask and
             process_image_zones(img, Regions(index="NDVI", above=0.2, min_pixels=64)) through this library and through that one, the
             same Python above both: the calls that existed before must not have moved.  Twice ``--rounds`` rounds, the order of the
             legs reversed in every other one, so that neither library always follows the other's work.

    python tools/outlinebench.py [--sizes 2048x1536,4096x4096] [--reps 5] [--rounds 3] [--hard] [--parent-lib PATH] [--json profiles/outlines.json]

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/outlinebench.py --outlines-only --sizes 4096x4096
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lars_image_processing_amd import _ffi  # noqa: E402
from regionbench import HARD_MASKS, MASKS, MIN_PIXELS, alternate, mask_of, median_ms, picture, summary  # noqa: E402


def parent_library(path):
    """The parent commit's library beside the loaded one: its own symbols first (it calls its own entry points, not this library's),
    the prototypes of every entry point it has."""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def through(lib, fn):
    """``fn`` with the package bound to ``lib`` for the call."""
    def call():
        mine = _ffi._lib
        _ffi._lib = lib
        try:
            return fn()
        finally:
            _ffi._lib = mine
    return call


def outline_row(lars, mask, connectivity, args, with_contourpy=False):
    got = lars.region_outlines(mask, connectivity=connectivity)
    row = {"n_regions": got["n_regions"], "n_rings": got["n_rings"], "n_vertices": got["n_vertices"], "foreground": float(mask.mean())}
    if 0 < got["n_regions"] <= 65535 and got["n_vertices"] <= 1 << 24:             # what rasterize_zones takes
        assert np.array_equal(lars.rasterize_zones(got["outlines"], mask.shape), got["labels"])        # the rings are the labels' own
        row["rasterised_back"] = True
    if args.outlines_only:
        for _ in range(2):
            lars.region_outlines(mask, connectivity=connectivity)
        return row
    legs = {"outlines": lambda: lars.region_outlines(mask, connectivity=connectivity),
            "labels": lambda: lars.label_regions(mask, connectivity=connectivity)}
    try:
        import contourpy
    except ImportError:
        contourpy = None
    if with_contourpy and contourpy is not None:
        z = (got["labels"] > 0).astype(np.float64)
        legs["contourpy"] = lambda: contourpy.contour_generator(z=z, line_type=contourpy.LineType.Separate).lines(0.5)
    del got
    for name, rounds in alternate(legs, args.reps, args.rounds).items():
        row[name] = summary(rounds)
    row["outlines_over_labels"] = row["outlines"]["ms"] / row["labels"]["ms"]
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2048x1536,4096x4096", help="WIDTHxHEIGHT, comma separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hard", action="store_true", help="also the masks built to be hard, under both connectivities (without the checkerboard under 4)")
    ap.add_argument("--checkerboard-4", action="store_true", help="also the checkerboard under connectivity 4: every other pixel a ring")
    ap.add_argument("--no-ordinary", action="store_true", help="leave the three ordinary masks out")
    ap.add_argument("--outlines-only", action="store_true", help="region_outlines alone, twice per mask after a first call (for a kernel trace)")
    ap.add_argument("--parent-lib", help="a liblars_hip.so of the parent commit: the calls that existed before, through both libraries in turn")
    ap.add_argument("--json", help="also write the figures to this file")
    args = ap.parse_args()
    import lars_image_processing_amd as lars
    print("device:", _ffi.device_name(), flush=True)
    out = {"device": _ffi.device_name(), "reps": args.reps, "rounds": args.rounds, "sizes": {}}
    for w, h in [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]:
        size_row = {"pixels": h * w, "outlines": {}}
        for kind in () if args.no_ordinary else MASKS:
            size_row["outlines"][kind] = outline_row(lars, mask_of(kind, h, w), 8, args, with_contourpy=True)
            print(f"{w}x{h} outlines {kind}", json.dumps(size_row["outlines"][kind]), flush=True)
        hard = [(k, c) for k in HARD_MASKS for c in (8, 4) if (k, c) != ("checkerboard", 4)] if args.hard else []
        for kind, connectivity in hard + ([("checkerboard", 4)] if args.checkerboard_4 else []):
            row = outline_row(lars, mask_of(kind, h, w), connectivity, args)
            size_row.setdefault("hard", {})[f"{kind}-{connectivity}"] = row
            print(f"{w}x{h} hard {kind} connectivity {connectivity}", json.dumps(row), flush=True)
        if args.parent_lib:
            here, parent = _ffi.load(), parent_library(args.parent_lib)
            mask, img = mask_of("field", h, w), picture(h, w)
            regions = lars.Regions(index="NDVI", above=0.2, min_pixels=MIN_PIXELS, max_regions=65535)
            a = lars.label_regions(mask)
            b = through(parent, lambda: lars.label_regions(mask))()
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)              # the same bytes through both
            legs = {"label_regions": through(here, lambda: lars.label_regions(mask)),
                    "label_regions_parent": through(parent, lambda: lars.label_regions(mask)),
                    "picture": through(here, lambda: lars.process_image_zones(img, regions)),
                    "picture_parent": through(parent, lambda: lars.process_image_zones(img, regions))}
            times = {name: [] for name in legs}
            for k in range(2 * args.rounds):
                for name in list(legs)[::1 if k % 2 == 0 else -1]:
                    times[name].append(median_ms(legs[name], args.reps))
            row = {name: summary(rounds) for name, rounds in times.items()}
            for name in ("label_regions", "picture"):
                row[name + "_over_parent"] = row[name]["ms"] / row[name + "_parent"]["ms"]
            size_row["default"] = row
            print(f"{w}x{h} default", json.dumps(row), flush=True)
        out["sizes"][f"{w}x{h}"] = size_row
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
