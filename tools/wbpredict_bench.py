"""The headline step (white-balance tables + three planes + statistics) under the wb_predict settings, on one resident batch in one
process and one output arena: milliseconds of the pre-pass and of the launches per step, the per-launch cost of the verifying kernel
against the plain one, and how many tiles the predictor was confident about and how many of those a verified launch had to repair.

    python tools/wbpredict_bench.py --profile vegetation --tiles 1024 --sixteenths 2,3,4
    python tools/wbpredict_bench.py --profile natural --tiles 256            # tools/jointbench.py's hand-made contents
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lars_image_processing_amd as lars  # noqa: E402
from lars_image_processing_amd import _ffi  # noqa: E402

INDICES = ("NDVI", "GNDVI", "NDWI")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", default="vegetation")
    ap.add_argument("--settings", default="0,1,2", help="wb_predict settings to alternate")
    ap.add_argument("--sixteenths", default="2", help="sampled sixteenths to time under wb_predict = 1")
    ap.add_argument("--k", type=int, default=3)
    args = ap.parse_args()
    if args.profile in ("uniform", "vegetation"):
        b = lars.TileBatch.synthetic(args.tiles, args.tile, args.tile, seed=1234, profile=args.profile)
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import jointbench
        b = jointbench.make_batch(args.profile, args.tiles, args.tile)
    with _ffi.tuning(wb_predict=0):
        b.compute_wb_tables()
        outs = b.make_outputs(indices=INDICES, index=True, ring=args.ring, arena="plain")
    stats = b.new_stats()
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        _ffi.call("lars_event_create", C.byref(e))
    variants = []
    for s in map(int, args.settings.split(",")):
        for f in (map(int, args.sixteenths.split(",")) if s == 1 else [2]):
            variants.append((s, f))
    times = {v: [] for v in variants}
    reports = {}
    for _ in range(args.rounds + 1):
        for v in variants:
            with _ffi.tuning(wb_predict=v[0], wb_predict_sixteenths=v[1], wb_predict_k=args.k):
                _ffi.call("lars_event_record", ev[0], None)
                b.compute_wb_tables()
                _ffi.call("lars_event_record", ev[1], None)
                n = b.run_fused_chunks(INDICES, True, stats, False, outs)
                _ffi.call("lars_event_record", ev[2], None)
                ms = C.c_float(0)
                _ffi.call("lars_event_elapsed_ms", ev[0], ev[1], C.byref(ms))
                pre = float(ms.value)
                _ffi.call("lars_event_elapsed_ms", ev[1], ev[2], C.byref(ms))
                times[v].append((pre, float(ms.value), n))
                reports[v] = b.wb_predict_report()
    out = {"profile": args.profile, "tiles": args.tiles, "tile": args.tile, "ring": args.ring, "k": args.k, "variants": {}}
    for v, t in times.items():
        t = np.array(t[1:])
        out["variants"][f"wb_predict={v[0]} sixteenths={v[1]}"] = {
            "pre_pass_ms": round(float(np.median(t[:, 0])), 3), "launches_ms": round(float(np.median(t[:, 1])), 3),
            "per_launch_ms": round(float(np.median(t[:, 1] / t[:, 2])), 4), "step_ms": round(float(np.median(t[:, 0] + t[:, 1])), 3),
            "confident": reports[v][0], "missed": reports[v][1]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
