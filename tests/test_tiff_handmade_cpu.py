"""The model of decode_tiff's LZW kernel (tests/tiff_lzw_model.py) against the host decoder, the specification, on hand-built
streams (tests/tiff_handmade_cases.py) and on a seeded fuzz of streams that are valid but not greedy, before any such stream
reaches a GPU: a stream on which k_td_lzw would index out of range, read a byte that is not written yet or stand still fails
an assertion of the model here.  Each case also states, as claims on the model's event record, which path it is there for.
The last tests show that the table tells a slightly wrong decoder from the right one: one-line mutations of a copy of the
model each fail a named case, or are shown to be equivalent."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lzw_writer as lw  # noqa: E402
import tiff_cases as tc  # noqa: E402
import tiff_handmade_cases as C  # noqa: E402
import tiff_lzw_model as model  # noqa: E402
from test_tiffio import lzw_encode  # noqa: E402


def check(c, m=model):
    """One case: the model equals the host decoder (bytes and count, or being an error), the host decoder equals the writer's
    plaintext where there is one, and the model took the paths the case claims.  Returns the event record."""
    ev = m.new_events()
    got = m.decode(c["stream"], c["ndst"], ev)
    want = tc.host_lzw(c["stream"], c["ndst"])
    assert got[1] == want[1], f"host decoder: bad = {want[1]}, model: bad = {got[1]}"
    assert got[1] or got[0] == want[0], f"host decoder: {len(want[0])} bytes, model: {len(got[0])} bytes, or other bytes"
    if "plain" in c:
        assert want == (c["plain"][:c["ndst"]], 0), "the host decoder does not give the writer's plaintext"
    for key, value in c.get("claims", {}).items():
        if isinstance(value, set):
            assert value <= ev[key], f"{key}: {sorted(value - ev[key])} not seen"
        elif key.endswith("_min"):
            assert ev[key[:-4]] >= value, f"{key[:-4]}: {ev[key[:-4]]} < {value}"
        else:
            assert ev[key] == value, f"{key}: {ev[key]}, not {value}"
    return ev


# ---- the writer ------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_read_what_the_encoders_write():
    rng = np.random.default_rng(2)
    for data in (rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), bytes(30000), b"\x07", rng.integers(0, 3, 12000, dtype=np.uint8).tobytes()):
        enc = lzw_encode(data)
        codes = lw.unpack(enc)
        assert lw.pack(codes) == enc and lw.plaintext(codes) == data
        assert codes == lw.encode(data, clear_at=4094)            # the test encoder of test_tiffio.py is the policy 4094
        assert (lw.bit_length(codes) + 7) // 8 == len(enc)
    assert tc.pack is lw.pack and tc.unpack is lw.unpack
    assert [lw.width_of(i) for i in (0, 253, 254, 765, 766, 1789, 1790, 5000)] == [9, 9, 10, 10, 11, 11, 12, 12]
    assert all(lw.width_of(i) == model.width_of(i) for i in range(6000))


@pytest.mark.parametrize("policy", [dict(clear_at=None), dict(clear_at=4096), dict(clear_at=4095), dict(clear_at=4096, frozen_run=500),
                                    dict(clear_at=300), dict(clear_at=1000), dict(clear_at=None, leading_clear=False, eoi=False)],
                         ids=lambda p: " ".join(f"{k}={v}" for k, v in p.items()))
def test_the_encoder_keeps_its_clear_policy(policy):
    data = b"\x41" + np.random.default_rng(3).integers(0, 5, 40000, dtype=np.uint8).tobytes()
    codes = lw.encode(data, **policy)
    assert lw.plaintext(codes) == data and tc.host_lzw(lw.pack(codes), len(data)) == (data, 0)
    runs, i = [], 0                                               # data codes of every segment that a Clear ended
    for code in codes[1:] if policy.get("leading_clear", True) else codes:
        if code == lw.CLEAR:
            runs.append(i)
        i = 0 if code == lw.CLEAR else i + 1
    at = policy["clear_at"]
    if at is None:
        assert not runs and len(codes) > 5000
    else:                                                         # after k codes the encoder holds 258 + k codes
        assert len(runs) >= 2 and set(runs) == {at - lw.FIRST + policy.get("frozen_run", 0)}


def test_the_generator_is_valid_by_construction_and_not_greedy():
    rng = np.random.default_rng(5)
    greedy = 0
    for k in range(60):
        w = lw.Writer().random(rng, int(rng.integers(1, 900)), clears=(7, 300), p_clear=0.003, literals=int(rng.choice([2, 256]))).eoi()
        plain = w.plain()
        assert len(plain) == w.n and tc.host_lzw(w.stream(), len(plain)) == (plain, 0)
        assert lw.unpack(w.stream()) == w.codes and w.codes.count(lw.CLEAR) >= 1 + (len(w.codes) > 9)
        greedy += lw.encode(plain, clear_at=None) == w.codes
    assert greedy <= 3                                            # only the shortest streams are what a greedy matcher writes
    w = lw.Writer().lit(1, 2)
    with pytest.raises(AssertionError):
        w.entry(2)                                                # one above the fill level
    with pytest.raises(AssertionError):
        lw.plaintext(w.codes + [lw.FIRST + 2])
    assert lw.plaintext(w.put(lw.FIRST + 1).codes) == bytes([1, 2, 2, 2])


# ---- the table -------------------------------------------------------------------------------------------------------
def test_the_table_names_what_the_issue_lists():
    names = C.VALID + C.INVALID + C.SLOW
    assert len(names) == len(set(names)) == len(C.CASES) and len(C.SLOW) == 3
    for word in ("full table", "long strings", "batch", "clear", "width", "end", "encoder"):
        assert any(n.startswith(word + ":") for n in names), word


@pytest.mark.parametrize("name", C.VALID)
def test_model_equals_host_decoder_on_valid_streams(name):
    c = C.case(name)
    assert "plain" in c
    check(c)


@pytest.mark.parametrize("name", C.INVALID)
def test_model_equals_host_decoder_on_invalid_streams(name):
    c = C.case(name)
    check(c)
    assert tc.host_lzw(c["stream"], c["ndst"])[1] == 1 and "plain" not in c


@pytest.mark.parametrize("name", C.SLOW)
def test_model_equals_host_decoder_on_a_long_string_stream(name):
    """The zero chain costs the model about 5 s (7.4 MB, byte by byte), the chains to 2048 and 2049 bytes about 1.5 s each."""
    check(C.case(name))


def test_the_table_as_a_whole_reaches_every_path():
    ev = model.new_events()
    for name in C.VALID + C.INVALID:
        c = C.case(name)
        one = model.new_events()
        model.decode(c["stream"], c["ndst"], one)
        for key, value in one.items():
            ev[key] = ev[key] | value if isinstance(value, set) else max(ev[key], value)
    assert ev["dep_b"] == {"self", "none", "inside", "lane0"}
    assert ev["clear_lanes"] == set(range(64)) and {0, 1, 62, 63} <= ev["eoi_lanes"]
    assert {0, 63} <= ev["fill_lanes"] and {1, 63} <= ev["next_lanes"]
    assert ev["max_i"] >= 3839 + 200 and ev["pcap_batches"] >= 2 and ev["stage_full"] >= 1 and 4096 in ev["totals"]
    assert {253, 254, 765, 766, 1789, 1790} <= ev["first_at"] and ev["rounds"] >= 63


# ---- the seeded fuzz -------------------------------------------------------------------------------------------------
def test_seeded_fuzz_model_equals_host_decoder():
    cases = C.fuzz_cases()
    assert len(cases) == C.FUZZ_STREAMS == 2000
    kinds, old, bad, frozen, short = {}, 0, 0, 0, 0
    for k, (kind, stream, ndst, plain) in enumerate(cases):
        want = tc.host_lzw(stream, ndst)
        if C.old_style(stream):                                   # lars_tiff_info refuses it: the kernel never sees it
            assert want[1] == 1
            old += 1
            continue
        c = dict(stream=stream, ndst=ndst)
        if plain is not None:
            c["plain"] = plain
        try:
            ev = check(c)
        except AssertionError as e:
            raise AssertionError(f"stream {k} ({kind}, {stream.hex() if len(stream) < 400 else len(stream)}, ndst {ndst}): {e}") from e
        kinds[kind] = kinds.get(kind, 0) + 1
        bad += want[1]
        short += (not want[1]) and len(want[0]) < ndst
        frozen += ev["max_i"] >= 3839
    print(f"fuzz: {len(cases)} streams, {kinds}, old-style {old}, corrupt {bad}, short {short}, past the freeze {frozen}")
    assert set(kinds) == {"valid", "cut", "flip", "splice"} and kinds["valid"] == 500
    # one stream in 40 is long: of the 500 valid ones about 12, 6 in 7 of them with a chunk that is not halved
    assert bad >= 200 and short >= 200 and frozen >= 10 and old <= 20


# ---- the table tells a slightly wrong decoder from the right one -----------------------------------------------------
MUTATIONS = [
    ("PCAP 3838", "PCAP = 3840 ", "PCAP = 3838 ", "full table: codes 4094 and 4095 used after the freeze, in front of the batch and inside it"),
    ("STAGE 4095", "STAGE = 4096 ", "STAGE = 4095 ", "long strings: a batch of 64 codes whose inclusive sum is exactly 4096"),
    ("9 bits up to i = 254", "9 if i <= 253", "9 if i <= 254", "width: Clear at i = 254, the first code of its width"),
    ("9 bits up to i = 252", "9 if i <= 253", "9 if i <= 252", "width: Clear at i = 253, the last code of its width"),
    ("10 bits up to i = 764", "10 if i <= 765", "10 if i <= 764", "width: EOI at i = 765, the last code of its width"),
    ("10 bits up to i = 766", "10 if i <= 765", "10 if i <= 766", "width: EOI at i = 766, the first code of its width"),
    ("11 bits up to i = 1790", "11 if i <= 1789", "11 if i <= 1790", "width: Clear at i = 1790, the first code of its width"),
    ("11 bits up to i = 1788", "11 if i <= 1789", "11 if i <= 1788", "width: Clear at i = 1789, the last code of its width"),
    ("the code above the fill level passes", "code[lane] - FIRST > i - 1", "code[lane] - FIRST > i", "batch: a code one above the fill level at lane 63"),
    ("the same at i = 3837", "code[lane] - FIRST > i - 1", "code[lane] - FIRST > i", "full table: code 4095 at i = 3837 is above the table"),
    ("the fill-level code refused", "code[lane] - FIRST > i - 1", "code[lane] - FIRST > i - 2", "full table: code 4095 at i = 3838 is the fill level, the last entry"),
    ("the i == 0 stop rule dropped", " or (idx[lane] == 0 and start[lane] >= ndst)", "",
     "end: the literal that fills the chunk, then Clear, Clear, a literal and a corrupt code"),
    ("a first code stops like any other", "(idx[lane] >= 1 and end[lane] >= ndst)", "(end[lane] >= ndst)",
     "end: the literal that fills the chunk, then a code above the table"),
    ("the dep_b rule dropped", "dep_b = lane_b if (j + 1 >= seg_i and lane_b != lane) else -1", "dep_b = -1",
     "batch: an entry j with j + 1 == seg_i, seen from lanes 1 and 63"),
    ("the same inside a batch", "dep_b = lane_b if (j + 1 >= seg_i and lane_b != lane) else -1", "dep_b = -1", C.GOOD),
    ("seg_bit advanced without the Clear's own width", "seg_bit += bits_before(seg_i) + width_of(seg_i)", "seg_bit += bits_before(seg_i)",
     "clear: two and three Clears in a row, at the start, in the middle and before EOI"),
    ("the open-ended 12-bit branch capped", "d = 0 if i < 1790 else i - 1790", "d = 0 if i < 1790 else min(i - 1790, 2049)",
     "full table: 64 code(s) past i = 3839 without Clear"),
    ("a batch cut at the stage restarts the segment", "        seg_i += nproc\n", "        seg_i += nproc if nproc == ndata else 0\n",
     "long strings: a batch of 64 codes whose inclusive sum is 4097 at the last lane"),
]
# Argued equivalent in DESIGN.md: entry 258 + j exists for j <= 3837 and its length needs P[j + 1], so the highest slot read is
# P[3838] and P[] has one slot to spare.  PCAP 3839 alone, or `j + 1 < PCAP` as `j + 2 < PCAP` alone, changes no result; the two
# together, or PCAP 3838, lose entry 4095.
EQUIVALENT = [("PCAP 3839", [("PCAP = 3840 ", "PCAP = 3839 ")]), ("j + 2 < PCAP", [("and j + 1 < PCAP", "and j + 2 < PCAP")])]
BOTH = [("PCAP = 3840 ", "PCAP = 3839 "), ("and j + 1 < PCAP", "and j + 2 < PCAP")]
FULL_TABLE = [n for n in C.VALID + C.INVALID if n.startswith(("full table", "encoder"))]


def mutant(*pairs):
    src = Path(model.__file__).read_text()
    for old, new in pairs:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    spec = importlib.util.spec_from_loader("tiff_lzw_model_mutant", loader=None)
    mod = importlib.util.module_from_spec(spec)
    exec(compile(src, "tiff_lzw_model_mutant", "exec"), mod.__dict__)
    return mod


@pytest.mark.parametrize("what,old,new,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mutated_model_fails_its_case(what, old, new, name):
    check(C.case(name))
    with pytest.raises(AssertionError):
        check(C.case(name), mutant((old, new)))


@pytest.mark.parametrize("what,pairs", EQUIVALENT, ids=[m[0] for m in EQUIVALENT])
def test_the_spare_slot_of_P_makes_two_mutations_equivalent(what, pairs):
    m = mutant(*pairs)
    for name in FULL_TABLE:
        c = C.case(name)
        assert m.decode(c["stream"], c["ndst"]) == model.decode(c["stream"], c["ndst"])
    with pytest.raises(AssertionError):
        check(C.case("full table: codes 4094 and 4095 used after the freeze, in front of the batch and inside it"), mutant(*BOTH))
