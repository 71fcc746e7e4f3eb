#!/usr/bin/env python3
"""Nodata-aware processing (process_image_masked(valid=...), csrc/masked.hip) next to the call without a mask.

Pictures: seeded vegetation-like uint8 RGNir images (oracle.index_oracle.synth_tile_u8) of 2048 x 1536 and 4096 x 4096 with a
black frame that holds a quarter of the raster, and that frame as the mask.  Request: the three indices with their
statistics, histograms and float32 planes, and the corrected image.  Per size, after a warm-up call, the median over
``--reps`` host call times (upload, kernels, downloads; every call returns after a device synchronise), the masked and the
unmasked leg alternating ``--rounds`` times (median of the rounds' medians), of

  masked      process_image_masked(img, want_hist=True, valid=mask)
  unmasked    process_image(img, want_hist=True) on the same picture in the same process
  this_lib / parent_lib
              the unmasked call in fresh child processes, alternating between this build's library and ``--parent-lib`` (the
              library built from the parent commit): the default route launches the same kernels in both, so the two columns
              differ by the run-to-run scatter of the session, which the rounds show
  numpy       the NumPy model of the definition (tests/masked_model.py) on the host, once

    python tools/maskbench.py [--sizes 2048x1536,4096x4096] [--reps 7] [--parent-lib PATH] [--json out.json]

Kernel times come from a separate run:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/maskbench.py --masked-only --sizes 4096x4096
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

MASKED_SYMBOLS = ("lars_d_valid_mask", "lars_d_masked_channel_hist", "lars_d_masked_fused", "lars_h_valid_mask", "lars_h_process_image_masked")


def picture(h, w):
    from oracle import index_oracle as orc
    img = orc.synth_tile_u8(99, 0, h, w, profile="vegetation")
    by, bx = int(round(h * (1 - 0.75 ** 0.5) / 2)), int(round(w * (1 - 0.75 ** 0.5) / 2))
    valid = np.zeros((h, w), dtype=bool)
    valid[by:h - by, bx:w - bx] = True
    img = np.ascontiguousarray(img)
    img[~valid] = 0
    return img, valid


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def sizes_of(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",")]


def child(args):
    """The unmasked call alone, on the library LARS_HIP_LIB names (the parent's lacks the masked entry points)."""
    if args.child == "parent":
        for name in MASKED_SYMBOLS:
            _ffi.SIGNATURES.pop(name, None)
    import lars_image_processing_amd as lars
    out = {}
    for w, h in sizes_of(args.sizes):
        img, _ = picture(h, w)
        out[f"{w}x{h}"] = median_ms(lambda: lars.process_image(img, want_hist=True), args.reps)[0]
    print("CHILD " + json.dumps(out), flush=True)


def run_child(which, lib, args):
    env = dict(os.environ)
    if lib:
        env["LARS_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--sizes", args.sizes, "--reps", str(args.reps)],
                       env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"child ({which}) failed with {p.returncode}:\n{p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1]
    return json.loads(line[6:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2048x1536,4096x4096", help="WIDTHxHEIGHT, comma separated")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the masked and the unmasked leg, and of the two child processes")
    ap.add_argument("--parent-lib", help="liblars_hip.so built from the parent commit")
    ap.add_argument("--masked-only", action="store_true", help="the masked call alone (for a kernel trace)")
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--child", choices=["this", "parent"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import lars_image_processing_amd as lars
    import masked_model as mm
    print("device:", _ffi.device_name(), flush=True)
    out = {"device": _ffi.device_name(), "reps": args.reps, "request": "three indices, statistics, histograms, float32 planes, corrected image",
           "sizes": {}}
    for w, h in sizes_of(args.sizes):
        img, valid = picture(h, w)
        row = {"pixels": h * w, "valid_pixels": int(valid.sum())}
        # No result is kept while a call is timed: fresh result arrays are what the host API pays most for (first-touch page
        # faults), and whether the allocator hands back mapped pages depends on what else is alive.  The
        # two legs alternate, so neither is the one that runs on the colder heap.
        legs = {"masked": lambda: lars.process_image_masked(img, want_hist=True, valid=valid)}
        if not args.masked_only:
            legs["unmasked"] = lambda: lars.process_image(img, want_hist=True)
        times = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, fn in legs.items():
                times[name].append(median_ms(fn, args.reps))
        for name, runs in times.items():
            row[f"{name}_ms_rounds"] = [r[0] for r in runs]
            row[f"{name}_ms"], row[f"{name}_min_ms"], row[f"{name}_max_ms"] = float(np.median([r[0] for r in runs])), min(r[1] for r in runs), max(r[2] for r in runs)
        if not args.masked_only:
            row["masked_over_unmasked"] = row["masked_ms"] / row["unmasked_ms"]
            t0 = time.perf_counter()
            want = mm.masked_model(img, valid)
            row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            row["numpy_over_masked"] = row["numpy_ms"] / row["masked_ms"]
            res = lars.process_image_masked(img, want_hist=True, valid=valid)
            assert res["valid_pixels"] == row["valid_pixels"]
            mm.check_result(res, want, mm.INDEX_NAMES, want_rgba=False)          # the timed call computes the model's numbers
            del res, want
        out["sizes"][f"{w}x{h}"] = row
        print(f"{w}x{h}", " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in row.items()), flush=True)
    if args.parent_lib and not args.masked_only:
        rounds = {"this_lib": [], "parent_lib": []}
        for _ in range(args.rounds):
            rounds["this_lib"].append(run_child("this", None, args))
            rounds["parent_lib"].append(run_child("parent", os.path.abspath(args.parent_lib), args))
        for key, row in out["sizes"].items():
            for which, runs in rounds.items():
                row[f"{which}_unmasked_ms_rounds"] = [r[key] for r in runs]
                row[f"{which}_unmasked_ms"] = float(np.median([r[key] for r in runs]))
            row["this_over_parent"] = row["this_lib_unmasked_ms"] / row["parent_lib_unmasked_ms"]
            print(key, "this", row["this_lib_unmasked_ms_rounds"], "parent", row["parent_lib_unmasked_ms_rounds"], flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
