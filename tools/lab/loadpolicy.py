#!/usr/bin/env python3
"""The hot path's tile loads under each cache policy (lars_d_probe kinds 200..247, csrc/lab/probe.hip, csrc/stream_load.h).

Three conditions: read-only, the headline's 12 B : 48 B write mix, and the two-reader arrangement of sharedprobe.py.  The
variants of a condition ALTERNATE launch by launch in one process, and the plain policy runs twice in every rotation: the
difference between its two columns is the spread against which the other columns are read.

    python tools/lab/loadpolicy.py [--tiles 256] [--reps 7] [--blocks 16,64] [--isa build/isa/probe.s] [--out profiles/load_policy_probe.txt]

--isa: the probe's device assembly, from which the table quotes every variant's load instruction -- csrc/lab/probe.hip compiled with the
Makefile's flags and ``-S --cuda-device-only -o build/isa/probe.s``.
"""
import argparse, ctypes as C, os, re, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lablib
from lars_image_processing_amd import _ffi

POLICIES = ("plain", "nt", "sc1", "nt sc1")
SHAPES = {0: ("12 B per lane (b96)", 12), 1: ("16 B + 8 B per lane (b128 + b64)", 24), 2: ("16 B per lane (b128)", 16)}
QT = 4194304                                         # vectors per chunk: a 4096 x 4096 tile's quads


def isa_lines(path):
    """Per probe instantiation the distinct `buffer_load` forms of its assembly (hipcc -S / --save-temps), registers blanked."""
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w*k_probe_(?:policy|shared)\w*):", line)
        if m:
            name = m.group(1)
            out[name] = set()
        elif name and "s_endpgm" in line:
            name = None
        elif name and "buffer_load" in line:
            out[name].add(re.sub(r"v\[\d+:\d+\], v\d+, s\[\d+:\d+\], \S+", "v[..], v, s[..], soff", line.strip()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", default="16,64", help="workgroups of 256 threads per chunk (read-only and mix)")
    ap.add_argument("--isa", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    src = _ffi.DeviceBuffer(a.tiles * QT * 24)
    slots = min(a.tiles, 64)
    dst = _ffi.DeviceBuffer(slots * 4 * QT * 12)
    lablib.probe(3, 1, 8192, None, src.ptr, src.nbytes - src.nbytes % 16)
    e0, e1 = C.c_void_p(), C.c_void_p()
    _ffi.call("lars_event_create", C.byref(e0)); _ffi.call("lars_event_create", C.byref(e1))

    def timed(kind, unroll, blocks, nbytes):
        _ffi.call("lars_event_record", e0, None)
        lablib.probe_policy(*kind, unroll, blocks, src.ptr, dst.ptr, nbytes)
        _ffi.call("lars_event_record", e1, None)
        ms = C.c_float(0); _ffi.call("lars_event_elapsed_ms", e0, e1, C.byref(ms))
        return ms.value

    def rotation(title, cond, shape, unroll, blocks, nbytes, moved):
        cols = [0, 1, 2, 3, 0]                                      # plain, nt, sc1, nt sc1, plain again
        ts = [[] for _ in cols]
        for rep in range(2 + a.reps):                               # two warm-up rotations
            for j, pol in enumerate(cols):
                t = timed((cond, shape, pol), unroll, blocks, nbytes)
                if rep >= 2:
                    ts[j].append(t)
        med = [float(np.median(t)) for t in ts]
        mn = [float(np.min(t)) for t in ts]
        spread = abs(med[0] - med[4]) / min(med[0], med[4]) * 100
        say(title)
        for j, pol in enumerate(cols):
            name = POLICIES[pol] + (" (again)" if j == 4 else "")
            say(f"    {name:16s} median {med[j]:8.4f} ms  min {mn[j]:8.4f} ms   {moved / med[j] / 1e6:7.0f} GB/s (median)   "
                f"{(med[0] / med[j] - 1) * 100:+6.2f} % against plain")
        say(f"    spread of the two plain columns: {spread:.2f} %")

    say(f"load-policy probe: {a.tiles} chunks of {QT} vectors per shape, {a.reps} timed launches after 2 warm-up, variants alternating")
    for shape, (name, vb) in SHAPES.items():
        for blocks in [int(x) for x in a.blocks.split(",")]:
            nbytes = a.tiles * QT * vb
            rotation(f"read-only, {name}, {blocks} workgroups per chunk", 0, shape, 1, blocks, nbytes, nbytes)
    for blocks in [int(x) for x in a.blocks.split(",")]:
        nbytes = a.tiles * QT * 12
        rotation(f"12 B read : 48 B written, 12 B per lane (b96), {blocks} workgroups per chunk, {slots} output slots", 1, 0, slots, blocks,
                 nbytes, nbytes * 5)
    for shape in (0, 2):
        name, vb = SHAPES[shape]
        nbytes = a.tiles * QT * vb
        for readers in (1, 2):
            rotation(f"shared readers, {name}, 1024 chunks, {readers} reader(s) per chunk on one XCD (rate = bytes once)", 2, shape, readers,
                     1024, nbytes, nbytes)
    if a.isa:
        say()
        say("ISA of each variant (distinct buffer_load forms per instantiation, registers blanked):")
        for name, forms in sorted(isa_lines(a.isa).items()):
            say(f"  {name}")
            for f in sorted(forms):
                say(f"      {f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
