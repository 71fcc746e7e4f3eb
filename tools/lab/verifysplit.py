#!/usr/bin/env python3
"""Where does the verifying form of the headline launch (k_fused_u8c3, VERIFY) spend its time over the plain form?

Laboratory build of the library (make -C lars_image_processing_amd/csrc labverify), in which LARS_LAB_VERIFY_FORM names the form a
verified launch of three planes + basic statistics runs -- the kernel alone, no repair launches behind it:

    0  the plain form (16 quads per step, byte table)
    2  the plain form with 12 quads per step
    3  form 2 with the dword table and the packed add, counters kept alive but never reduced
    4  form 3 with the reduction and twelve atomics per workgroup: the verifying body in a kernel of its own
    1  the product's kernel: a block takes the verifying body (form 4's) for a tile that carries a prediction, the plain body
       (form 0's) for any other
   -1  the product's whole verified launch (kernel + gated exact pass + repair launch + memset)

(the VERIFY values of k_fused_u8c3 in csrc/fused.hip; the forms tried and dropped -- three-operand adds, 16 quads with two unpacks, the
table alone, the reduction without atomics, 64-bit atomics -- are described with their numbers in profiles/wb_lean_verify_split.txt.)

One process, one resident batch, one arena, the forms alternating pass by pass (a pass = the batch's launches), the tables
predicted again before every pass; per-launch medians over the rounds.

    LARS_HIP_LIB=build/labverify/liblars_verify.so python tools/lab/verifysplit.py --tiles 1024 --rounds 3
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import lars_image_processing_amd as lars  # noqa: E402
from lars_image_processing_amd import _ffi  # noqa: E402

INDICES = ("NDVI", "GNDVI", "NDWI")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forms", default="0,2,3,4,1,-1,0")
    ap.add_argument("--arena", default="auto", choices=["auto", "plain"], help="auto: the searched arena bench.py runs in")
    args = ap.parse_args()
    forms = [int(f) for f in args.forms.split(",")]
    b = lars.TileBatch.synthetic(args.tiles, args.tile, args.tile, seed=1234, profile="vegetation")
    with _ffi.tuning(wb_predict=0):
        b.compute_wb_tables()
        outs = b.make_outputs(indices=INDICES, index=True, ring=args.ring, arena=args.arena)
    stats = b.new_stats()
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        _ffi.call("lars_event_create", C.byref(e))
    times = {i: [] for i in range(len(forms))}
    for _ in range(args.rounds + 1):
        for i, form in enumerate(forms):
            os.environ["LARS_LAB_VERIFY_FORM"] = str(form)
            with _ffi.tuning(wb_predict=1):
                b.compute_wb_tables()
                _ffi.call("lars_event_record", ev[0], None)
                n = b.run_fused_chunks(INDICES, True, stats, False, outs)
                _ffi.call("lars_event_record", ev[1], None)
            ms = C.c_float(0)
            _ffi.call("lars_event_elapsed_ms", ev[0], ev[1], C.byref(ms))
            times[i].append(float(ms.value) / n)
    os.environ.pop("LARS_LAB_VERIFY_FORM", None)
    out = {"tiles": args.tiles, "tile": args.tile, "ring": args.ring, "rounds": args.rounds,
           "arena": args.arena, "arena_probe_ms": (outs.arena_report or {}).get("chosen_ms"), "per_launch_ms": []}
    for i, form in enumerate(forms):
        t = np.array(times[i][1:])
        out["per_launch_ms"].append({"form": form, "median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4),
                                     "max": round(float(t.max()), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
