"""The output-arena search of TileBatch.make_outputs (lars_image_processing_amd/arena.py) on a fake device: no GPU, no library.

The search is host logic around three effects -- allocate, ask how much device memory is free, time one placement of the
planes -- so a fake device can script every path of it, also those a real allocator shows once in ten processes.  Every
scenario asserts the whole trace (allocations, probes with the planes' placement and warm-up, frees, synchronisations, in
order), where the planes end up, and every key of ``arena_report`` / ``placement_ms`` but the wall-clock ones.

The expected values in tests/golden/arena_search_traces.json were NOT produced by the code under test: they were recorded
from ``make_outputs`` as it was before the search moved out of batch.py (commit 75bfb0a), by running this very file as a
script in a checkout of that commit (``python tests/test_arena_search_cpu.py > tests/golden/arena_search_traces.json``).
``run_make_outputs`` below is what recorded them and what ``test_make_outputs_follows_the_record`` runs today.  One
scenario kind differs on purpose: after a failed search (``raises`` in the record) that commit left ``outs.index`` pointing
into freed arenas; the expected end state here is "no plane points anywhere" (``test_a_failed_search_leaves_nothing_dangling``).
The trace of those scenarios is the recorded one.
"""
import contextlib
import itertools
import json
import os
import sys
from unittest import mock

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lars_image_processing_amd  # noqa: E402,F401  (does not load the library)
from lars_image_processing_amd import _ffi, batch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "arena_search_traces.json")
GIB = 1 << 30
TYPES = ("NDVI", "GNDVI", "NDWI")
FAILURES = {"LarsError": lambda: _ffi.LarsError(-2, "out of memory"), "KeyboardInterrupt": KeyboardInterrupt}


class FakeBuffer:
    def __init__(self, device, number, nbytes, ptr):
        self.device, self.number, self.nbytes, self.ptr = device, number, int(nbytes), ptr

    def free(self):
        if self.ptr:
            self.device.trace.append(["free", self.number])
            self.device.live -= self.nbytes
            self.ptr = None

    def upload(self, array):
        """Only colour tables are uploaded to (BatchOutputs makes them before any arena): not an allocation of the search."""
        assert self.device.trace.pop() == ["alloc", self.nbytes] and self.number == self.device.count - 1
        self.device.count -= 1
        self.number = "lut"


class FakeDevice:
    """Numbers its buffers, hands out addresses that do not overlap, fails the ``fail_alloc``-th allocation, answers the
    probes from ``ms`` (3.0 for ever when None) and raises ``probe_raises[1]`` on the ``probe_raises[0]``-th."""

    def __init__(self, free_gib=280, fail_alloc=None, ms=None, probe_raises=None):
        self.total, self.live, self.count, self.calls, self.next_ptr = int(free_gib * GIB), 0, 0, 0, 1 << 40
        self.fail_alloc, self.ms, self.probe_raises = fail_alloc, None if ms is None else list(ms), probe_raises
        self.trace, self.probes, self.outs = [], 0, None

    def alloc(self, nbytes):
        self.calls += 1
        if self.calls == self.fail_alloc:
            self.trace.append(["alloc", int(nbytes), "fails"])
            raise FAILURES["LarsError"]()
        self.trace.append(["alloc", int(nbytes)])
        buf = FakeBuffer(self, self.count, nbytes, self.next_ptr)
        self.count, self.live, self.next_ptr = self.count + 1, self.live + buf.nbytes, self.next_ptr + buf.nbytes + (1 << 21)
        return buf

    def stats(self):
        return FakeBuffer(self, "stats", 0, 1 << 30)

    def free_bytes(self):
        return self.total - self.live

    def synchronize(self):
        self.trace.append(["sync"])

    def probe(self, outs, warm_ms):
        """One timing of ``outs`` where its planes point now."""
        self.outs = outs
        self.probes += 1
        self.trace.append(["probe", planes_of(outs), float(warm_ms)])
        if self.probe_raises and self.probes == self.probe_raises[0]:
            raise FAILURES[self.probe_raises[1]]()
        return 3.0 if self.ms is None else self.ms.pop(0)


def planes_of(outs):
    """Per plane (index planes, then RGBA planes): [number of the allocation it lies in, byte offset], None for a plane that points nowhere."""
    planes = [outs.index[k] for k in outs._index_ids] + [outs.rgba[k] for k in outs._rgba_ids]
    return [None if p is None else [p.owner.number, p.ptr - p.owner.ptr] for p in planes]


def fake_batch(device, ntiles, h, w):
    b = object.__new__(batch.TileBatch)
    b.ntiles, b.h, b.w, b.channels, b.npix, b.table = ntiles, h, w, 3, h * w, None
    b.new_stats = device.stats
    b._probe_arena = lambda outs, indices, stats, warm_ms=30.0: device.probe(outs, warm_ms)
    return b


def flat(*levels, each=4):
    return [ms for level in levels for ms in [level] * each]


FOUR_FLAT = flat(3.00, 3.02, 3.05, 3.09)         # four allocations of one kind each, at distinct levels: the order of the pairs is determined
AFTER = [2.9]                                   # the survivor timed once more after the rejected allocations were freed
BIG = dict(ntiles=64, h=4096, w=4096)            # 64 slots of 4096 x 4096: planes of 4 GiB
SCENARIOS = {
    "1 the first allocation shows both classes": dict(BIG, ms=[3.0, 3.0, 2.5, 3.0]),
    "2 the second allocation shows a gap": dict(BIG, ms=flat(3.0) + [3.0, 2.5, 3.0, 3.0] + AFTER),
    "3 the third cross pair is fast": dict(BIG, ms=FOUR_FLAT + [3.0, 3.0, 2.5] + AFTER),
    "4 the third extra block is fast": dict(BIG, ms=FOUR_FLAT + [3.0] * 6 + [3.0, 3.0, 2.5] + AFTER),
    "4b the allocator fails on the second extra block": dict(BIG, ms=FOUR_FLAT + [3.0] * 6 + [3.0] + AFTER, fail_alloc=6),
    "5 nothing is ever fast": dict(BIG, ms=[3.0] * (16 + 6 + 24) + AFTER),
    "5b extra blocks until device memory is short": dict(BIG, ms=[3.0] * (16 + 6 + 6) + AFTER, free_gib=128),
    "6 device memory short from the start": dict(BIG, ms=[3.0], free_gib=30),
    "6b no headroom at all for the first arena": dict(BIG, ms=[3.0], free_gib=18),
    "7 the allocator fails on the third buffer": dict(BIG, ms=[3.0] * (8 + 2) + AFTER, fail_alloc=3),
    "8 pick slowest": dict(BIG, ms=flat(3.0, 3.0) + [3.0, 3.1, 3.0, 3.0] + flat(3.0) + AFTER, kw=dict(pick="slowest")),
    "8b pick slowest, both classes in the first allocation": dict(BIG, ms=[2.5, 3.0, 3.0, 3.0], kw=dict(pick="slowest")),
    "9 small planes, three packed allocations": dict(ntiles=8, h=512, w=512, ms=[1.0, 1.0, 1.0] + AFTER, kw=dict(ring=2, placement_trials=3)),
    "9b small planes, a gap at the second": dict(ntiles=8, h=512, w=512, ms=[1.0, 0.9] + AFTER, kw=dict(ring=2, placement_trials=3)),
    "9c plain arena of large planes with trials": dict(BIG, ms=[3.0, 3.0, 2.5] + AFTER, kw=dict(arena="plain", placement_trials=3)),
    "10 the probe raises on its third call": dict(BIG, ms=[3.0, 3.0], probe_raises=(3, "LarsError")),
    "10b interrupted in the sixth probe": dict(BIG, ms=[3.0] * 5, probe_raises=(6, "KeyboardInterrupt")),
    "10c the first allocation fails": dict(BIG, ms=[], fail_alloc=1),
    "11 two planes": dict(BIG, ms=[3.0, 3.0, 3.0, 2.5, 3.0], kw=dict(indices=("NDVI", "GNDVI"))),
    "11b six planes": dict(BIG, ms=[3.0, 2.5, 3.0], kw=dict(rgba=True)),
    "12 no search: plain": dict(BIG, ms=[], kw=dict(arena="plain")),
    "12b no search: one plane": dict(BIG, ms=[], kw=dict(indices=("NDWI",))),
    "12c no search: no trials": dict(BIG, ms=[], kw=dict(placement_trials=0)),
    "12d no search: one trial": dict(BIG, ms=[], kw=dict(placement_trials=1)),
    "12e no search: a small arena": dict(BIG, ms=[], kw=dict(ring=8)),
    "12f no search: planes of 1 GiB": dict(BIG, ms=[], kw=dict(ring=16)),
    "12g no search: no planes": dict(BIG, ms=[], kw=dict(index=False, wb=False)),
    "13 constants patched at run time": dict(ntiles=32, h=4096, w=4096, ms=[3.0] * (10 + 2 + 24) + AFTER, constants=dict(ARENA_CLASS_GAP=0.0, ARENA_TRIALS=2)),
}


def constants_home():
    """The module whose ARENA_* constants the search reads."""
    return getattr(lars_image_processing_amd, "arena", batch)


def run_make_outputs(ntiles, h, w, ms=None, kw=None, free_gib=280, fail_alloc=None, probe_raises=None, constants=None):
    """``TileBatch.make_outputs`` with the device behind it replaced: -> (device, outs or None, the exception or None)."""
    device = FakeDevice(free_gib, fail_alloc, ms, probe_raises)

    def call(name, *args):
        if name == "lars_mem_info":
            args[0]._obj.value, args[1]._obj.value = device.free_bytes(), device.total
        else:
            assert name == "lars_synchronize", name
            device.synchronize()

    outs = error = None
    with mock.patch.object(batch, "DeviceBuffer", device.alloc), mock.patch.object(_ffi, "call", call), \
            mock.patch.multiple(constants_home(), **constants) if constants else contextlib.nullcontext():
        try:
            outs = fake_batch(device, ntiles, h, w).make_outputs(**dict(dict(index=True), **(kw or {})))
        except BaseException as exc:                                   # KeyboardInterrupt is one of the scripted failures
            error = exc
    assert not device.ms, "the scenario scripts more timings than the search asked for"
    return device, outs, error


def summary(device, outs, error):
    """What a scenario is held to, as JSON would store it."""
    got = {"trace": device.trace, "raises": None if error is None else f"{type(error).__name__}: {error}"}
    if outs is not None:
        report = dict(outs.arena_report)
        if "malloc_ms" in report:                                      # wall-clock figures: their types, and how many
            assert all(isinstance(x, float) for x in report["malloc_ms"] + [report["search_ms"]])
            report["malloc_ms"] = len(report["malloc_ms"])
            report["search_ms"] = None
        got.update(planes=planes_of(outs), arena=getattr(outs.arena, "number", None), arena2=getattr(outs.arena2, "number", None),
                   plane_offsets=list(getattr(outs, "plane_offsets", [])) or None, arena_report=report,
                   placement_ms=getattr(outs, "placement_ms", None))
    return json.loads(json.dumps(got))


def canonical(value):
    """Text in which 3 and 3.0, or a list and a number, differ: the report's types are part of the record."""
    return json.dumps(value, sort_keys=True)


# -- the planner's grid ----------------------------------------------------------------------------------------------------
PLANES = {0: dict(index=False), 1: dict(indices=TYPES[:1]), 2: dict(indices=TYPES[:2]), 3: dict(), 4: dict(indices=TYPES[:2], rgba=True),
          6: dict(rgba=True)}                                          # five planes cannot be asked for
# (h, w, slots): planes of 4096 x 4096 slots are multiples of 64 MiB -- under, at and over 2 GiB per plane (32 slots) and per arena
# (16 slots x 2 planes, 8 x 4; 10 and 11 slots x 3 planes straddle it); 32 slots of 4095 x 4097 are 128 bytes short of 2 GiB and
# rounded up to it as a plane
SHAPES = [(4096, 4096, s) for s in (1, 8, 10, 11, 16, 31, 32, 33, 64)] + [(4095, 4097, 32)]


def grid():
    for pick, arena, trials, (nplanes, planes), shape in itertools.product(
            ("fastest", "slowest", "best"), ("auto", "plain", "assembled"), (None, 0, 1, 2, 4), PLANES.items(), SHAPES):
        yield pick, arena, trials, nplanes, planes, shape


def decision_of_make_outputs(pick, arena, trials, planes, shape):
    """What make_outputs decides, read off its effects: nothing allocated / one packed allocation / a search, with room to spare
    inside its allocations or not, of so many allocations when no candidate ever stands out (the first probe of each has the long warm-up)."""
    h, w, slots = shape
    kw = dict(planes, ring=slots, pick=pick, arena=arena, placement_trials=trials)
    device, outs, error = run_make_outputs(slots, h, w, kw=kw, free_gib=4096)
    if error is not None:
        return f"{type(error).__name__}: {error}"
    allocs = [e[1] for e in device.trace if e[0] == "alloc"]
    probes = [e for e in device.trace if e[0] == "probe"]
    if not probes:
        return "packed" if allocs else "none"
    packed = len(probes[0][1]) * outs.plane_bytes
    long_warm_ups = sum(1 for before, e in zip(device.trace, device.trace[1:]) if before[0] == "alloc" and e[0] == "probe" and e[2] == 30.0)
    return f"search spread={allocs[0] > packed} trials={long_warm_ups}"


def run_length(outcomes):
    return [[outcome, len(list(group))] for outcome, group in itertools.groupby(outcomes)]


def record():
    scenarios = {name: summary(*run_make_outputs(**sc)) for name, sc in SCENARIOS.items()}
    return {"scenarios": scenarios, "planner": run_length(decision_of_make_outputs(p, a, t, planes, shape) for p, a, t, _, planes, shape in grid())}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def expected_of(golden, name):
    want = dict(golden["scenarios"][name])
    if want["raises"]:
        assert "planes" not in want                                    # the call raised: the record holds no outputs
    return want


def test_the_record_covers_the_scenarios(golden):
    assert sorted(golden["scenarios"]) == sorted(SCENARIOS)
    ends = {name: (g.get("arena_report") or {}).get("kind", g["raises"]) for name, g in golden["scenarios"].items()}
    ended_by = lambda name: ends[name].split("search ended by: ")[-1].rstrip(")")
    assert ended_by("1 the first allocation shows both classes") == ended_by("2 the second allocation shows a gap") == "both classes seen"
    assert ended_by("3 the third cross pair is fast") == "both classes seen: planes split between two allocations"
    assert ended_by("4 the third extra block is fast") == "both classes seen: second half of the planes in an allocation of its own"
    assert ended_by("5 nothing is ever fast") == "placement_trials" and ended_by("7 the allocator fails on the third buffer") == "device memory"
    worst = golden["scenarios"]["5 nothing is ever fast"]["arena_report"]
    # today's worst case, documented, not blessed: 4 allocations of 24 GiB and 24 of 4 GiB held at once for 12 GiB of planes
    assert (worst["allocations"], worst["transient_bytes"], worst["arena_bytes"]) == (4 + 24, 192 * GIB, 24 * GIB)
    first = golden["scenarios"]["1 the first allocation shows both classes"]
    assert [p[1] for p in first["trace"] if p[0] == "probe"][2] == first["planes"] == [[0, 0], [0, 4 * GIB], [0, 16 * GIB]]
    assert first["arena_report"]["rejected"] == 0 and first["arena_report"]["allocations"] == 1
    assert golden["scenarios"]["3 the third cross pair is fast"]["arena2"] is not None
    assert all(ends[name] == "plain hipMalloc" for name in SCENARIOS if name.startswith("12") and "no planes" not in name)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_make_outputs_follows_the_record(golden, name):
    device, outs, error = run_make_outputs(**SCENARIOS[name])
    got, want = summary(device, outs, error), expected_of(golden, name)
    assert got["trace"] == want["trace"]
    assert canonical(got) == canonical(want)


@pytest.mark.parametrize("name", [n for n, sc in SCENARIOS.items() if sc.get("probe_raises") or sc.get("fail_alloc") == 1])
def test_a_failed_search_leaves_nothing_dangling(golden, name):
    """The exception propagates, everything the search took is freed after a synchronise (the recorded trace ends with them), and --
    unlike the recorded commit, which left the index planes pointing into the freed arenas -- no plane of ``outs`` points anywhere."""
    sc = SCENARIOS[name]
    device, outs, error = run_make_outputs(**sc)
    assert outs is None and type(error).__name__ in ("LarsError", "KeyboardInterrupt")
    allocated = [e for e in device.trace if e[0] == "alloc" and len(e) == 2]
    tail = device.trace[-(len(allocated) + 2):]
    assert tail == [["sync"]] + [["free", j] for j in range(len(allocated))] + [["free", "stats"]]
    assert device.live == 0
    if device.outs is not None:                                        # the outputs the probe saw
        assert planes_of(device.outs) == [None] * 3 and device.outs.index == [None] * 3 and device.outs.rgba == [None] * 3
        assert device.outs.arena is None and device.outs.arena2 is None


@pytest.mark.parametrize("name", [n for n, sc in SCENARIOS.items() if n[:2] not in ("12", "13")])
def test_the_search_takes_its_effects_as_arguments(golden, name):
    """arena.search driven directly -- an allocator, a free-memory figure, a probe that is told the placement, a synchronise -- with
    no module patched: the recorded trace (less the statistics buffer, which is make_outputs' own) and the recorded report."""
    from lars_image_processing_amd import arena
    sc = SCENARIOS[name]
    kw = dict(dict(indices=TYPES, index=True, rgba=False, ring=None, placement_trials=None, arena="auto", pick="fastest"), **sc.get("kw", {}))
    device = FakeDevice(sc.get("free_gib", 280), sc.get("fail_alloc"), sc["ms"], sc.get("probe_raises"))
    with mock.patch.object(batch, "DeviceBuffer", device.alloc):       # the colour tables of RGBA planes, not the search
        outs = batch.BatchOutputs(fake_batch(device, sc["ntiles"], sc["h"], sc["w"]), kw["indices"], kw["index"], False, kw["rgba"], kw["ring"], allocate=False)
    nplanes = len(outs._index_ids) + len(outs._rgba_ids)
    plan = arena.plan_arena(nplanes, outs.plane_bytes, outs.slots * outs.batch.npix * 4, kw["arena"], kw["placement_trials"], kw["pick"])
    assert plan.kind == "search"

    def probe(placement, warm_ms):
        assert [list(p) for p in placement] == planes_of(outs)        # the planes point where the search says before it times them
        return device.probe(outs, warm_ms)

    error = None
    try:
        found = arena.search(outs, plan, kw["pick"], alloc=device.alloc, free_bytes=device.free_bytes, probe=probe, synchronize=device.synchronize)
        outs.placement_ms, outs.arena_report = arena.report(found)
    except BaseException as exc:
        error = exc
    want = expected_of(golden, name)
    want["trace"] = [e for e in want["trace"] if e != ["free", "stats"]]
    assert canonical(summary(device, None if error else outs, error)) == canonical(want)


def test_the_planner_decides_what_make_outputs_decided(golden):
    """arena.plan_arena over the grid (planes 0-6, plane and arena sizes around the two 2 GiB thresholds, arena, placement_trials,
    pick) against what make_outputs of the recorded commit did with the same arguments, read off its effects on the fake device."""
    from lars_image_processing_amd import arena

    def decide(pick, arena_kind, trials, nplanes, shape):
        h, w, slots = shape
        plane_bytes = (slots * h * w * 4 + 255) & ~255
        try:
            plan = arena.plan_arena(nplanes, plane_bytes, slots * h * w * 4, arena_kind, trials, pick)
        except ValueError as exc:
            return f"ValueError: {exc}"
        return plan.kind if plan.kind != "search" else f"search spread={plan.spread} trials={plan.trials}"

    got = [decide(p, a, t, nplanes, shape) for p, a, t, nplanes, _, shape in grid()]
    assert run_length(got) == golden["planner"]
    assert {"none", "packed", "search spread=True trials=4", "search spread=True trials=2", "search spread=False trials=4",
            "ValueError: arena must be auto or plain", "ValueError: pick must be fastest or slowest"} <= set(got)
    # ... and make_outputs still decides the same from end to end (a sample of the grid: every seventh case)
    cases = list(grid())[::7]
    assert [decision_of_make_outputs(p, a, t, planes, shape) for p, a, t, _, planes, shape in cases] == got[::7]


if __name__ == "__main__":
    rec = record()                                                     # one scenario per line
    lines = [f' {json.dumps(name)}: {json.dumps(got, sort_keys=True)}' for name, got in sorted(rec["scenarios"].items())]
    print('{"planner": %s,\n"scenarios": {\n%s\n}}' % (json.dumps(rec["planner"]), ",\n".join(lines)))
