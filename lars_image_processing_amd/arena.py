"""Where a batch's output planes live: the search behind ``TileBatch.make_outputs(arena="auto")``.

The float32 index planes (and RGBA8 planes) live in ONE allocation (an arena).  How fast the write-bound fused kernel runs
into a multi-GiB arena depends on WHERE its planes lie: device memory comes in two kinds that alternate along an allocation
in stretches of 6-16 GiB, and a launch whose write streams are split between the kinds runs 18 % faster than one whose planes
all lie in one kind (2.49-2.52 against 3.01-3.15 ms per 64-tile launch of the headline kernel;
profiles/r04_arena_two_kinds.txt).  Three 4 GiB planes packed into 12 GiB see a change of kind in three allocations of ten;
with room to spare inside the allocation a placement that does can be found in three of four.

The search, for arenas of ARENA_MIN_BYTES and more (``plan_arena`` decides whether it runs at all):
  1. ``within_allocations``: ONE allocation with up to ARENA_SPAN_BYTES of room beyond the first planes (24 GiB for three planes
     of 4 GiB, less if the device is short of memory), and the planes are tried in a handful of placements inside it
     (``arena_placements``) -- each timed with the batch's own launches (``TileBatch._probe_arena``).  If no placement is 7 %
     faster than another the allocation is of one kind throughout: another one is taken, up to ``trials``.
  2. ``across_pairs``: every allocation was of one kind (two fresh processes in ten on some boxes): the first half of the planes
     stays in one allocation and the rest goes to another, up to ARENA_CROSS_TRIALS pairs.  Such outputs keep BOTH allocations.
  3. ``extra_blocks``: ... and all of them of the SAME kind: up to ARENA_EXTRA_BLOCKS small allocations for the second half alone.
It ends as soon as both speed classes have been seen.  The fastest candidate is kept, every other allocation is freed and the
survivor is timed once more.  It is host logic around three effects -- allocate, ask how much device memory is free, time one
placement -- which it takes as arguments (tests/test_arena_search_cpu.py scripts them).

A placement is, per plane (index planes in the order of INDEX_NAMES, then the RGBA planes), ``(allocation, byte offset)``, the
allocation as its number among those the search took; ``BatchOutputs.adopt`` points the planes there.
"""
from __future__ import annotations

import time
from collections import namedtuple

import numpy as np

from ._ffi import LarsError

ARENA_MIN_BYTES = 2 << 30         # smaller arenas run alike wherever they land
ARENA_SPREAD_PLANE_BYTES = 2 << 30  # planes from this size on are worth a placement search (and its spare room)
ARENA_TRIALS = 4                  # allocations of the default search at most (each is tried with every placement of its planes)
ARENA_CLASS_GAP = 0.93            # the search ends once its best candidate is 7 % under its worst: both classes seen (they are ~18 % apart)
ARENA_WARM_MS = 30.0              # untimed launches before a candidate is timed: after an idle gap a fast arena needs ~22 ms to reach its level
ARENA_SPAN_BYTES = 20 << 30       # how far from the first planes the last ones may be placed inside an allocation (the memory changes kind every 6-16 GiB)
ARENA_SPAN_STEP = 4 << 30         # ... in steps of
ARENA_CROSS_TRIALS = 6            # pairs of allocations tried with the planes split between them when every allocation is of one kind
ARENA_EXTRA_BLOCKS = 24           # ... and after those, small allocations for the second half of the planes alone: stretches of one kind
                                  # reach 72 GiB in some processes (tools/lab/kindmap.py), and the allocations held so far have used most of one
ARENA_CALLER_HEADROOM = 8 << 30   # device memory the search leaves free for the caller: no further allocation below it
ARENA_SPREAD_HEADROOM = 16 << 30  # device memory left free when an allocation with room to spare is sized

ArenaPlan = namedtuple("ArenaPlan", "kind spread trials")   # kind: "none" (no planes), "packed" (one allocation, no timing) or "search"


def plan_arena(nplanes, plane_bytes, payload_bytes, arena="auto", placement_trials=None, pick="fastest"):
    """What ``TileBatch.make_outputs`` does for ``nplanes`` planes of ``plane_bytes`` (``payload_bytes``: slots x pixels x 4, a plane
    before its size is rounded up): nothing, one packed allocation as it comes, or a search over ``trials`` allocations at most --
    ``spread``: each with room to spare and the planes tried in several placements inside it."""
    if nplanes and arena not in ("auto", "plain"):
        raise ValueError("arena must be auto or plain")
    if pick not in ("fastest", "slowest"):
        raise ValueError("pick must be fastest or slowest")
    if not nplanes:
        return ArenaPlan("none", False, 0)
    # Room inside the allocation and several placements: only where it can pay -- two or more planes of ARENA_SPREAD_PLANE_BYTES
    # (2 GiB) or more each (planes of 1 GiB show no difference between placements: profiles/r04_arena_two_kinds.txt) -- and only
    # if the caller did not ask for one trial at most.  Such an arena KEEPS its spare room while the outputs live:
    # report["arena_bytes"] against the packed size (24 instead of 12 GiB for three planes of 4 GiB).
    spread = (arena == "auto" and nplanes * payload_bytes >= ARENA_MIN_BYTES and nplanes >= 2 and plane_bytes >= ARENA_SPREAD_PLANE_BYTES
              and (placement_trials is None or int(placement_trials) > 1))
    if placement_trials is None:
        # one plane: nothing to split -- sixteen 4 GiB single-plane arenas measured within 1 % of each other (profiles/r04_ndvi_plane_step_ways.txt)
        placement_trials = ARENA_TRIALS if spread else 0
    if placement_trials <= 1 and not spread:
        return ArenaPlan("packed", False, 0)
    return ArenaPlan("search", spread, max(1, int(placement_trials)))


def packed(nplanes, plane_bytes, start=0):
    return tuple(start + j * plane_bytes for j in range(nplanes))


def arena_placements(nplanes, plane_bytes, nbytes):
    """Byte offsets of ``nplanes`` planes of ``plane_bytes`` inside an allocation of ``nbytes`` that ``TileBatch.make_outputs`` tries:
    packed back to back, then the first ceil(n / 2) planes packed at the start and the rest packed from 8, 12, 16, 20 GiB on
    (every multiple of ARENA_SPAN_STEP beyond the first cluster up to ARENA_SPAN_BYTES that still fits).  Device memory changes kind
    every 6-16 GiB along an allocation and a launch is fast when its planes are split between the kinds (this module's docstring)."""
    # Two clusters: ceil(n / 2) planes at the start, the rest further out.  The other split of an odd number ((0, 16, 20) for three planes)
    # was measured too: 1 % slower than (0, 4, 16) although it balances the launch's four streams, the read included, more often -- and
    # the 28 GiB it needs came from one kind of memory throughout in three of six fresh processes, where the first 24 GiB of a fresh
    # process showed both classes in eleven of thirteen (profiles/r04_arena_fresh_processes.txt).
    n_first = (nplanes + 1) // 2
    first_bytes, second_bytes = n_first * plane_bytes, (nplanes - n_first) * plane_bytes
    out = [packed(nplanes, plane_bytes)]
    if nplanes < 2:
        return out
    start = ((first_bytes + ARENA_SPAN_STEP - 1) // ARENA_SPAN_STEP) * ARENA_SPAN_STEP
    for s0 in range(start, ARENA_SPAN_BYTES + 1, ARENA_SPAN_STEP):
        if s0 > first_bytes and s0 + second_bytes <= nbytes:
            out.append(packed(n_first, plane_bytes) + packed(nplanes - n_first, plane_bytes, s0))
    return out


def both_classes(best, worst):
    """Whether two timings are far enough apart to be the two speed classes."""
    return best <= ARENA_CLASS_GAP * worst


def allocations_of(placement):
    """The allocations a placement uses, in the order of its planes."""
    return list(dict.fromkeys(a for a, _ in placement))


class _Search:
    """What one search holds and has timed.  ``ended_by`` goes into the report."""

    def __init__(self, outs, plan, pick, alloc, free_bytes, probe):
        self.outs, self.spread, self.trials, self.pick = outs, plan.spread, plan.trials, pick
        self.alloc, self.free_bytes, self.probe = alloc, free_bytes, probe
        self.nplanes, self.plane_bytes = len(outs._index_ids) + len(outs._rgba_ids), outs.plane_bytes
        self.n_first = (self.nplanes + 1) // 2                             # planes of the first cluster; the rest form the second
        self.second_bytes = (self.nplanes - self.n_first) * self.plane_bytes
        self.buffers, self.malloc_ms = [], []                              # every allocation taken, in order
        self.cands = []                                                    # (ms, placement)
        self.ended_by = "placement_trials"
        self.started = time.perf_counter()

    def times(self):
        return [ms for ms, _ in self.cands]

    def take(self, nbytes):
        """One more allocation; False if the device has none of that size (the first one must exist: that error is the caller's)."""
        t0 = time.perf_counter()
        try:
            buf = self.alloc(nbytes)
        except LarsError:
            if not self.buffers:
                raise
            return False
        self.malloc_ms.append((time.perf_counter() - t0) * 1e3)
        self.buffers.append(buf)
        return True

    def time(self, placement, idle=False):
        """One more candidate.  ``idle``: the device has just waited for an allocation (the long warm-up: ``TileBatch._probe_arena``)."""
        self.outs.adopt(self.buffers, placement)
        self.cands.append((self.probe(placement, ARENA_WARM_MS if idle else 5.0), placement))
        return self.cands[-1][0]

    def split(self, i, j):
        """The first cluster packed at the start of allocation ``i``, the second at the start of allocation ``j``."""
        return (tuple((i, o) for o in packed(self.n_first, self.plane_bytes))
                + tuple((j, o) for o in packed(self.nplanes - self.n_first, self.plane_bytes)))


def within_allocations(s):
    """Phase 1: allocation after allocation, each with every placement of the planes inside it.  -> both classes seen."""
    packed_bytes = s.nplanes * s.plane_bytes
    while len(s.buffers) < s.trials:
        free, want = s.free_bytes(), packed_bytes
        if s.spread:
            want = max(packed_bytes, min(ARENA_SPAN_BYTES + s.second_bytes, free - ARENA_SPREAD_HEADROOM))
        if free < want + ARENA_CALLER_HEADROOM:
            if s.buffers:
                s.ended_by = "device memory"
                return False
            want = packed_bytes                                            # the first arena must exist whatever the headroom
        if not s.take(want):
            s.ended_by = "device memory"
            return False
        for k, offsets in enumerate(arena_placements(s.nplanes, s.plane_bytes, want)):
            s.time(tuple((len(s.buffers) - 1, o) for o in offsets), idle=k == 0)
        if len(s.cands) >= 2 and both_classes(min(s.times()), max(s.times())):
            s.ended_by = "both classes seen"
            return True
    return False


def across_pairs(s, slow):
    """Phase 2.  Every allocation of ONE kind throughout (no placement 7 % under another; seen for all four 24 GiB allocations of some
    processes: profiles/r05_arena_first_process.txt): allocations differ in kind among each other -- their slow levels do,
    3.01 against 3.09 ms -- so the first cluster of planes stays in one and the rest goes to another, tried from the pair
    whose levels lie furthest apart.  Both allocations are then kept.  ``slow``: the slowest candidate of phase 1, the level a
    split has to beat.  -> both classes seen."""
    n = len(s.buffers)
    level = [float(np.mean([ms for ms, p in s.cands if p[0][0] == j])) for j in range(n)]
    pairs = sorted(((abs(level[i] - level[j]), i, j) for i in range(n) for j in range(n) if i != j), reverse=True)
    for _, i, j in pairs[:ARENA_CROSS_TRIALS]:
        if both_classes(s.time(s.split(i, j)), slow):
            s.ended_by = "both classes seen: planes split between two allocations"
            return True
    return False


def extra_blocks(s, slow):
    """Phase 3.  ... and if all of them are of the SAME kind: small allocations for the second cluster alone (while the large ones
    are held they come from other memory), next to the first cluster in the first allocation.  -> both classes seen."""
    while len(s.buffers) < s.trials + ARENA_EXTRA_BLOCKS:
        if s.free_bytes() < s.second_bytes + ARENA_CALLER_HEADROOM or not s.take(s.second_bytes):
            return False
        if both_classes(s.time(s.split(0, len(s.buffers) - 1)), slow):
            s.ended_by = "both classes seen: second half of the planes in an allocation of its own"
            return True
    return False


def search(outs, plan, pick, alloc, free_bytes, probe, synchronize):
    """Run ``plan`` (a "search" of ``plan_arena``) for the planes of ``outs`` and leave them in the ``pick`` ("fastest" / "slowest")
    candidate; every other allocation is freed.  ``alloc(nbytes)`` -> a buffer (``nbytes``, ``free()``; LarsError when there is no
    memory), ``free_bytes()`` -> free device memory, ``probe(placement, warm_ms)`` -> milliseconds of the planes of ``outs`` where
    they point now (``placement``, for the record), ``synchronize()`` waits for the device.  -> the finished search, for ``report``.
    If anything raises, everything taken is freed and no plane of ``outs`` points anywhere."""
    s = _Search(outs, plan, pick, alloc, free_bytes, probe)
    try:
        if not within_allocations(s) and s.spread and pick == "fastest" and len(s.buffers) >= 2:
            slow = max(s.times())
            if not across_pairs(s, slow) and s.ended_by == "placement_trials":     # not when device memory ran short
                extra_blocks(s, slow)
        times = s.times()
        s.chosen_ms, s.chosen = s.cands[int(np.argmin(times) if pick == "fastest" else np.argmax(times))]
        outs.adopt(s.buffers, s.chosen)
        s.kept = allocations_of(s.chosen)
        for j, buf in enumerate(s.buffers):
            if j not in s.kept:
                buf.free()
        synchronize()
        # the survivor once more, now that the rejected allocations are gone: the figure the steps should reproduce
        s.post_free_ms = probe(s.chosen, ARENA_WARM_MS) if len(s.buffers) > 1 else float(s.chosen_ms)
    except BaseException:
        # a failed probe launch or allocation: nothing of the search may stay behind, and `outs` must not point into a freed arena
        synchronize()
        outs.forget_planes()
        for buf in s.buffers:
            buf.free()
        raise
    s.search_ms = (time.perf_counter() - s.started) * 1e3
    return s


def unsearched_report(plan):
    """``arena_report`` of outputs that needed no search."""
    if plan.kind == "none":
        return {"kind": "none"}
    return {"kind": "plain hipMalloc", "search_ms": 0.0, "chosen_ms": None, "post_free_ms": None, "rejected": 0}


def report(s):
    """(``placement_ms``, ``arena_report``) of a finished search."""
    gib = float(1 << 30)
    times = [float(ms) for ms in s.times()]
    kept_bytes = sum(s.buffers[j].nbytes for j in s.kept)

    def allocation(placement):                                             # a number, or the two a split lies in
        used = allocations_of(placement)
        return int(used[0]) if len(used) == 1 else used

    return {"arenas": times, "chosen": float(s.chosen_ms)}, {
        "kind": f"plain hipMalloc of {kept_bytes / gib:.1f} GiB{' in two allocations' if len(s.kept) > 1 else ''}, the {s.pick} of {len(s.cands)} "
                f"placements of the planes in {len(s.buffers)} allocation(s), timed with the batch's own launches (search ended by: {s.ended_by})",
        "search_ms": s.search_ms, "chosen_ms": float(s.chosen_ms), "post_free_ms": float(s.post_free_ms),
        "rejected": len(s.buffers) - len(s.kept), "candidate_ms": list(times), "malloc_ms": [float(x) for x in s.malloc_ms],
        "placements": [{"allocation": allocation(p), "offsets_gib": [round(o / gib, 3) for _, o in p], "ms": float(ms)} for ms, p in s.cands],
        "chosen_offsets_gib": [round(o / gib, 3) for _, o in s.chosen],
        "arena_bytes": int(kept_bytes), "packed_bytes": int(s.nplanes * s.plane_bytes), "allocations": len(s.buffers),
        "transient_bytes": int(sum(b.nbytes for b in s.buffers)),
        "probe": f">= {ARENA_WARM_MS:.0f} ms of untimed launches per allocation, then per placement one timed pass of launches over the batch's chunks"}
