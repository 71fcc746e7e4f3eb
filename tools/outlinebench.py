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

  simplify   with ``--simplify``: region_outlines(mask, simplify=t) (a) next to region_outlines(mask) (b) and to (b) followed by a host
             simplification this tool brings itself (c: the rounds of the device in NumPy int64, ``host_simplify`` below -- no library;
             checked equal to the model of the definition on the first rings and to (a) on all of them before anything is timed; timed
             once a round, without a warm-up), for the tolerances of ``--tolerances`` on the ordinary masks and, at the sizes of
             ``--corner-sizes``, on the slow corners: the checkerboard under connectivity 8 and a comb of growing teeth across the full
             width, whose depth is linear in its teeth.  Per mask and tolerance: vertices traced and kept, rounds, rings kept as
             traced, bytes down.  With ``--parent-lib`` also (d): region_outlines without the keyword, label_regions and
             process_image_zones(img, Regions(...)) through the parent's library and this one in turn.

    python tools/outlinebench.py [--sizes 2048x1536,4096x4096] [--reps 5] [--rounds 3] [--hard] [--parent-lib PATH] [--json profiles/outlines.json]
    python tools/outlinebench.py --simplify [--tolerances 0.5,1,2,8] [--parent-lib PATH] [--json profiles/outline_simplify.json]

Kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/outlinebench.py --outlines-only --sizes 4096x4096
    bash tools/ktrace.sh outline_simplify tools/outlinebench.py --simplify --simplify-only --masks field --sizes 4096x4096 --tolerances 1 --corner-sizes ''
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def growing_comb(h, w):
    """A spine along the top and a tooth in every other column, each a little longer than the one before: Douglas-Peucker takes them
    off one or two a level, so the depth is about twice the teeth."""
    mask = np.zeros((h, w), dtype=bool)
    mask[0, :] = True
    teeth = w // 2
    for i in range(teeth):
        mask[1:2 + i * (h - 3) // teeth, 2 * i] = True
    return mask


def host_simplify(ring_starts, xy, tq):
    """Douglas-Peucker as csrc/outline_simplify.hip runs it, in NumPy int64 on the host: ``ring_starts`` int32 [Q + 1] and ``xy`` float64
    [V, 2] (x, y) of a Polygons -> (ring_starts, xy, ring_area2, rounds, rings kept as traced) of the simplified rings."""
    count = np.diff(ring_starts).astype(np.int64)
    start = ring_starts[:-1].astype(np.int64)
    q = len(count)
    sbase = np.cumsum(count + 1) - (count + 1)
    n = int((count + 1).sum())
    ring = np.repeat(np.arange(q), count + 1)
    pos = np.arange(n) - sbase[ring]
    closing = pos == count[ring]
    at = start[ring] + np.where(closing, 0, pos)
    r, c = xy[at, 1].astype(np.int64), xy[at, 0].astype(np.int64)
    a, b = sbase[ring].copy(), (sbase + count)[ring].copy()
    kept = (pos == 0) | closing
    inside = np.flatnonzero(~kept)
    rounds, tq2 = 0, tq * tq
    best_m, best_k = np.zeros(n, dtype=np.int64), np.full(n, n, dtype=np.int64)
    while inside.size:
        s = inside
        sa, sb = a[s], b[s]
        abr, abc, apr, apc = r[sb] - r[sa], c[sb] - c[sa], r[s] - r[sa], c[s] - c[sa]
        len2, ap2, dot = abr * abr + abc * abc, apr * apr + apc * apc, apr * abr + apc * abc
        bp2 = (r[s] - r[sb]) ** 2 + (c[s] - c[sb]) ** 2
        cross = abr * apc - abc * apr
        m = np.where(len2 == 0, ap2, np.where(dot <= 0, ap2 * len2, np.where(dot >= len2, bp2 * len2, cross * cross)))
        best_m[sa] = 0
        np.maximum.at(best_m, sa, m)
        mine = (m == best_m[sa]) & (m > ((tq2 * np.where(len2 == 0, 1, len2)) >> 8))
        best_k[sa] = n
        np.minimum.at(best_k, sa[mine], s[mine])
        k = best_k[sa]
        split = k < n
        if not split.any():
            break
        rounds += 1
        kept[s[split & (s == k)]] = True
        left, right = split & (s < k), split & (s > k)
        b[s[left]] = k[left]
        a[s[right]] = k[right]
        inside = s[left | right]
    nxt = np.where(np.append(kept[1:], True), np.arange(n) + 1, np.append(b[1:], n))
    live, plain = kept & ~closing, ~closing
    kc = np.bincount(ring[live], minlength=q)
    karea, own = np.zeros(q, dtype=np.int64), np.zeros(q, dtype=np.int64)
    np.add.at(karea, ring[live], c[live] * r[nxt[live]] - c[nxt[live]] * r[live])
    after = np.flatnonzero(plain) + 1
    np.add.at(own, ring[plain], c[plain] * r[after] - c[after] * r[plain])
    back = (kc < 3) | (karea == 0) | ((karea > 0) != (own > 0))
    written = plain & (back[ring] | kept)
    out_count = np.where(back, count, kc)
    starts = np.concatenate(([0], np.cumsum(out_count))).astype(np.int32)
    return starts, np.stack((c[written], r[written]), axis=-1).astype(np.float64), np.where(back, own, karea), rounds, int(back.sum())


def check_host_simplify(plain, tq, most=20000):
    """``host_simplify`` is the model of the definition (tests/outline_simplify_model.py) on the first rings, ``most`` vertices of them."""
    import outline_simplify_model as sm
    p = plain["outlines"]
    q = max(1, int(np.searchsorted(p.ring_starts, most, side="right")) - 1)
    starts, verts = p.ring_starts[:q + 1], p.verts[:p.ring_starts[q]]
    traced = {"verts": verts[:, ::-1].astype(np.int32), "ring_start": starts[:-1], "ring_count": np.diff(starts), "ring_area2": plain["ring_area2"][:q],
              "n_rings": q, "n_vertices": len(verts), "ring_label": np.zeros(q, dtype=np.int32), "ring_key": np.zeros(q, dtype=np.int32), "n_edges": 0}
    want = sm.simplify(traced, tq)
    got = host_simplify(starts, verts, tq)
    assert np.array_equal(got[0][:-1], want["ring_start"]) and np.array_equal(got[1], want["verts"][:, ::-1]) and np.array_equal(got[2], want["ring_area2"])
    return q


def simplify_row(lars, mask, connectivity, tolerances, args):
    """The legs (a), (b), (c) on one mask for every tolerance."""
    plain = lars.region_outlines(mask, connectivity=connectivity)
    p = plain["outlines"]
    row = {"n_regions": plain["n_regions"], "n_rings": plain["n_rings"], "n_vertices": plain["n_vertices"], "tolerances": {}}
    ring_bytes, vert_bytes = _ffi.RING_DTYPE.itemsize, 8
    for t in tolerances:
        tq = int(np.floor(t * 16 + 0.5))
        got = lars.region_outlines(mask, connectivity=connectivity, simplify=t)
        if args.simplify_only:
            for _ in range(2):
                lars.region_outlines(mask, connectivity=connectivity, simplify=t)
            row["tolerances"][str(t)] = {"kept": got["n_vertices"]}
            continue
        model_rings = check_host_simplify(plain, tq)
        t0 = time.perf_counter()
        starts, xy, area2, rounds, restored = host_simplify(p.ring_starts, p.verts, tq)
        host_ms = (time.perf_counter() - t0) * 1e3
        g = got["outlines"]
        assert np.array_equal(starts, g.ring_starts) and np.array_equal(xy, g.verts) and np.array_equal(area2, got["ring_area2"])     # (c) is (a), byte for byte
        assert got["n_vertices_traced"] == plain["n_vertices"]
        legs = {"simplified": lambda: lars.region_outlines(mask, connectivity=connectivity, simplify=t),
                "plain": lambda: lars.region_outlines(mask, connectivity=connectivity)}
        out = {name: summary(rounds_) for name, rounds_ in alternate(legs, args.reps, args.rounds).items()}
        host = []
        for _ in range(args.host_rounds):
            t0 = time.perf_counter()
            again = lars.region_outlines(mask, connectivity=connectivity)
            host_simplify(again["outlines"].ring_starts, again["outlines"].verts, tq)
            host.append((time.perf_counter() - t0) * 1e3)
        out["plain_then_host"] = summary(host)
        out.update({"tq": tq, "traced": plain["n_vertices"], "kept": got["n_vertices"], "rounds": rounds, "rings_kept_as_traced": restored,
                    "host_simplify_alone_ms": host_ms, "model_checked_rings": model_rings,
                    "bytes_down": plain["n_rings"] * ring_bytes + got["n_vertices"] * vert_bytes,
                    "bytes_down_plain": plain["n_rings"] * ring_bytes + plain["n_vertices"] * vert_bytes,
                    "simplified_over_plain": out["simplified"]["ms"] / out["plain"]["ms"],
                    "simplified_over_plain_then_host": out["simplified"]["ms"] / out["plain_then_host"]["ms"]})
        row["tolerances"][str(t)] = out
    return row


def unchanged_row(lars, parent_path, h, w, args):
    """(d): the calls that existed before, through the parent's library and this one, alternating, the order reversed every other round."""
    here, parent = _ffi.load(), parent_library(parent_path)
    mask, img = mask_of("field", h, w), picture(h, w)
    regions = lars.Regions(index="NDVI", above=0.2, min_pixels=MIN_PIXELS, max_regions=65535)
    a = lars.region_outlines(mask)
    b = through(parent, lambda: lars.region_outlines(mask))()
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if k != "outlines")          # the same bytes through both
    assert all(getattr(a["outlines"], k).tobytes() == getattr(b["outlines"], k).tobytes() for k in ("verts", "ring_starts", "poly_starts"))
    calls = {"region_outlines": lambda: lars.region_outlines(mask), "label_regions": lambda: lars.label_regions(mask),
             "picture": lambda: lars.process_image_zones(img, regions)}
    legs = {}
    for name, fn in calls.items():
        legs[name], legs[name + "_parent"] = through(here, fn), through(parent, fn)
    times = {name: [] for name in legs}
    for k in range(2 * args.rounds):
        for name in list(legs)[::1 if k % 2 == 0 else -1]:
            times[name].append(median_ms(legs[name], args.reps))
    row = {name: summary(rounds) for name, rounds in times.items()}
    for name in calls:
        row[name + "_over_parent"] = row[name]["ms"] / row[name + "_parent"]["ms"]
    return row


def simplify_main(lars, args):
    tolerances = [float(v) for v in args.tolerances.split(",")]
    out = {"device": _ffi.device_name(), "reps": args.reps, "rounds": args.rounds, "host_rounds": args.host_rounds, "tolerances": tolerances, "sizes": {}}
    corner_sizes = set(args.corner_sizes.split(",")) if args.corner_sizes else set()
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        size_row = {"pixels": h * w, "masks": {}}
        cases = [] if args.no_ordinary else [(kind, 8, lambda kind=kind: mask_of(kind, h, w)) for kind in MASKS if kind in args.masks.split(",")]
        if size in corner_sizes:
            cases += [("checkerboard-8", 8, lambda: mask_of("checkerboard", h, w)), ("growing-comb", 8, lambda: growing_comb(h, w))]
        for name, connectivity, make in cases:
            size_row["masks"][name] = simplify_row(lars, make(), connectivity, tolerances, args)
            print(f"{size} simplify {name}", json.dumps(size_row["masks"][name]), flush=True)
        if args.parent_lib and not args.simplify_only:
            size_row["unchanged"] = unchanged_row(lars, args.parent_lib, h, w, args)
            print(f"{size} unchanged", json.dumps(size_row["unchanged"]), flush=True)
        out["sizes"][size] = size_row
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


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
    ap.add_argument("--simplify", action="store_true", help="the legs of region_outlines(simplify=): see above")
    ap.add_argument("--tolerances", default="0.5,1,2,8", help="with --simplify: the tolerances in pixels, comma separated")
    ap.add_argument("--corner-sizes", default="2048x1536", help="with --simplify: the sizes (of --sizes) at which the slow corners run as well; empty for none")
    ap.add_argument("--masks", default=",".join(MASKS), help="with --simplify: which of the ordinary masks, comma separated")
    ap.add_argument("--host-rounds", type=int, default=1, help="with --simplify: how often leg (c), which takes seconds, is timed")
    ap.add_argument("--simplify-only", action="store_true", help="with --simplify: region_outlines(simplify=) alone, twice after a first call (for a kernel trace)")
    args = ap.parse_args()
    import lars_image_processing_amd as lars
    print("device:", _ffi.device_name(), flush=True)
    if args.simplify:
        return simplify_main(lars, args)
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
