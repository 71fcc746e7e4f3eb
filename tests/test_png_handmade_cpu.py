"""The model of decode_png's inflate kernels (tests/png_inflate_model.py) against zlib on hand-built deflate streams
(tests/png_handmade_cases.py) and on a seeded fuzz, before any such stream reaches a GPU: a stream on which the kernels would
index out of range, stall or write a byte twice fails an assertion of the model here.  The last tests show that the table
tells a slightly wrong decoder from the right one: single-line mutations of a copy of the model each fail a named case."""
import importlib.util
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import deflate_writer as dw  # noqa: E402
import png_handmade_cases as C  # noqa: E402
import png_inflate_model as model  # noqa: E402

ORDER_DIFFERS_SHARE = 0.05


def check(c, m=model):
    """One case against zlib; returns None, or (zlib's words, the model's status) where only the order of discovery differs."""
    want, accept, words = C.zlib_says(c["stream"], c["need"])
    got, M = m.decode(c["stream"], c["h"], c["rb"])
    if "plain" in c:
        assert want is not None and want == c["plain"][:c["need"]], f"zlib: {words}"
    for p in c.get("dyn", ()):
        assert p in M.all_cands and p in M.trace["hits"], f"the dynamic block at bit {p} is not taken from the candidate list"
    for p in c.get("own", ()):
        assert p in M.trace["self"], f"the walker does not decode the block at bit {p} itself"
    for p in c.get("false", ()):
        assert p in [x["pos"] for x in M.cands] and p not in M.trace["hits"] + M.trace["self"], f"false candidate at bit {p}"
    if accept is None:
        assert got == want, f"model: {got if isinstance(got, tuple) else 'other bytes'}"
        return None
    assert isinstance(got, tuple), f"zlib: {words}; the model decodes"
    if C.status_matches(got, accept):
        return None
    assert got[0] in (model.DEFLATE, model.FAR, model.SHORT, model.ADLER), got
    return words, got


def test_the_writer_round_trips_through_zlib():
    rng = np.random.default_rng(1)
    raw = C.raw_rows(C.rows_same(40, 40, 2), 0)
    sink = C.start()
    dw.stored_block(sink, raw[:100], pad=3)
    dw.fixed_block(sink, C.random_symbols(rng, raw, 41, 100, 900))
    dw.dynamic_block(sink, C.random_symbols(rng, raw, 41, 900), final=True, maxlen=9, skew=True)
    assert zlib.decompress(C.finish(sink, raw)) == raw
    for adler in ("wrong", 1, 4):
        with pytest.raises(zlib.error):
            zlib.decompress(C.finish(sink, raw, adler=adler))
    for n in (9, 10, 11, 15):
        f = [int(x) for x in rng.integers(1, 1000, 60)]
        lens = dw.limited_lengths(dw.skewed(f, n), n)
        assert max(lens) == n and sum(2.0 ** -x for x in lens if x) == 1.0


def test_screen_equals_the_device_prefilter_at_every_offset():
    for name in ("dynamic block at bit 560", "false candidate in a stored block's payload", "truncated inside a dynamic header"):
        c = C.case(name)
        P = model.Plan(len(c["stream"]), c["h"], c["rb"])
        M = model.Model(c["stream"], c["h"], c["rb"])
        fast = set(model.screen(c["stream"], P.nbits))
        slow = {p for p in range(16, P.nbits) if p + 17 <= P.nbits and model.prefilter(M.w, P.nw, p)}
        assert fast == slow


@pytest.mark.parametrize("name", C.VALID)
def test_model_equals_zlib_on_valid_streams(name):
    assert check(C.case(name)) is None


def test_the_alignment_cases_cover_every_bit_of_a_quad_and_of_the_last_word():
    cases = [C.case(f"dynamic block at bit {C.ALIGN_FIRST + k}") for k in range(128)]
    assert {c["dyn"][0] % 128 for c in cases} == set(range(128))
    for c in cases:                                           # the block is the last: only padding bits, then the Adler-32
        assert len(c["stream"]) == (c["end"] + 7) // 8 + 4
    assert {c["end"] % 32 for c in cases} == set(range(32))


def test_model_status_is_zlib_s_on_invalid_streams():
    differs = {}
    for name in C.INVALID:
        c = C.case(name)
        d = check(c)
        if d is not None:
            differs[name] = d
        assert (name in differs) == ("differs" in c), (name, d)
        if d is not None:
            assert d == c["differs"], (name, d)
    print(f"invalid cases {len(C.INVALID)}, order differs {sorted(differs)}")
    assert len(differs) <= ORDER_DIFFERS_SHARE * len(C.INVALID)


# ---- 3b: the seeded fuzz ---------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_STREAMS = 20261017, 2000


def fuzz_stream(rng):
    """(stream, h, rb): random block types, code lengths up to 15 bits, overlapping copies, stored lengths; need <= 4096."""
    w = int(rng.integers(1, 48))
    h = int(rng.integers(1, 4096 // (w + 1) + 1))
    img = C.rows_same(w, h, int(rng.integers(1 << 30)), hi=int(rng.choice([3, 20, 256])))
    raw = C.raw_rows(img, 0)
    plain = raw + bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)) if rng.random() < 0.15 else raw
    if rng.random() < 0.05:
        plain = plain[:int(rng.integers(0, len(plain)))]       # too few bytes
    cuts = sorted(int(x) for x in rng.integers(0, len(plain) + 1, int(rng.integers(0, 5))))
    sink = C.start()
    bounds = [0] + cuts + [len(plain)]
    for k in range(len(bounds) - 1):
        a, b = bounds[k], bounds[k + 1]
        final = k == len(bounds) - 2
        t = int(rng.integers(3))
        stop = min(b, len(raw))
        syms = C.random_symbols(rng, raw, w + 1, min(a, stop), stop, p_copy=float(rng.random()) * 0.6) + [("lit", x) for x in plain[max(a, stop):b]]
        if t == 0:
            dw.stored_block(sink, plain[a:b], final=final, pad=int(rng.integers(256)))
        elif t == 1:
            dw.fixed_block(sink, syms, final=final)
        else:
            nl = len({s[1] for s in syms if s[0] == "lit"}) + 1 + len({dw.length_symbol(s[1])[0] for s in syms if s[0] == "copy"})
            nd = len({dw.distance_symbol(s[2])[0] for s in syms if s[0] == "copy"})
            ml, md = int(rng.integers(9, 16)), int(rng.integers(5, 16))
            dw.dynamic_block(sink, syms, final=final, maxlen=ml, skew=nl > ml and rng.random() < 0.7, d_maxlen=md,
                             d_skew=nd > md and rng.random() < 0.7, trim=rng.random() < 0.8,
                             use=[(16, 17, 18), (16,), (17, 18), ()][int(rng.integers(4))])
    return C.finish(sink, plain), h, w


def mutate(rng, stream):
    s = bytearray(stream)
    kind = int(rng.integers(3))
    at = int(rng.integers(2, len(s)))
    if kind == 0:
        s[at] ^= 1 << int(rng.integers(8))
    elif kind == 1:
        del s[at:]
    else:
        s.insert(at, int(rng.integers(256)))
    return bytes(s)


def test_seeded_fuzz_model_equals_zlib():
    rng = np.random.default_rng(FUZZ_SEED)
    errors, differs, equal, unchecked = 0, [], 0, 0
    for k in range(FUZZ_STREAMS):
        stream, h, w = fuzz_stream(rng)
        if k % 2:
            stream = mutate(rng, stream)
        c = dict(stream=stream, h=h, rb=w, need=h * (w + 1))
        assert c["need"] <= 4096
        error = C.zlib_says(stream, c["need"])[1] is not None
        errors += error
        if not error:                                         # more data than the picture: the trailer is not looked at
            try:
                zlib.decompress(stream)
            except zlib.error:
                unchecked += 1
        try:
            d = check(c)
        except AssertionError as e:
            raise AssertionError(f"stream {k}: {e}") from e
        if d is None:
            equal += 1
        else:
            differs.append((k,) + d)
    print(f"fuzz: {FUZZ_STREAMS} streams, {errors} errors by zlib, model == zlib {equal}, order differs {len(differs)}: {differs}")
    print(f"fuzz: {unchecked} decode although zlib.decompress raises: bytes beyond the picture and a damaged or missing Adler-32")
    assert len(differs) <= ORDER_DIFFERS_SHARE * errors


# ---- 3c: the table tells a slightly wrong decoder from the right one ---------------------------------------------------------
MUTATIONS = [
    ("checkpoint every PD_CK symbols: mask off by one", "(nsym & (PD_CK - 1)) == 0", "(nsym & PD_CK) == 0", "symbols 256"),
    ("segment limit >= cap read as > cap", "if nsym >= cap:\n                L.done = 2", "if nsym > cap:\n                L.done = 2",
     "symbols 4097"),
    ("a code of PD_FB + 1 bits in the first-level table", "slow_decode(e, L.lcnt, L.lsym, PD_FB)", "slow_decode(e, L.lcnt, L.lsym, PD_FB + 1)",
     "literal/length codes up to 11 bits"),
    ("the same for distances", "slow_decode(e, L.dcnt, L.dsym, PD_FB)", "slow_decode(e, L.dcnt, L.dsym, PD_FB + 1)",
     "distance codes up to 11 bits"),
    ("pre-filter: the o > 61 read dropped", "elif o > 61:", "elif o > 99:", "dynamic block at bit 560"),
    ("a copy not clipped at need", "while k < v and o + k < need:", "while k < v:", "a copy that straddles the end of the picture"),
    ("a 16 does not carry a length into the distance alphabet", "ln, rep = tmp[idx - 1], 3 + br.bits(2)",
     "ln, rep = (0 if idx == nlen else tmp[idx - 1]), 3 + br.bits(2)", "repeats 16 17 18 at both ends, a 16 across the alphabets"),
    ("284 + 31 read as 257", "ln = C_LBASE[ls] + br.bits(C_LEXT[ls])", "ln = min(257, C_LBASE[ls] + br.bits(C_LEXT[ls]))",
     "length 258 as 285 and as 284+31"),
    ("stored LEN read without skipping the padding bits", "p = (br.pos() + 7) & ~7", "p = br.pos() & ~7",
     "stored blocks of 0, 1 and 65535 bytes, padding bits set"),
]
# quad()'s q + 4 <= nw read as q + 4 < nw changes nothing: pd_plan's nw leaves the last quad zero padding (Model.__init__
# asserts it), so the guarded load and the zeros are the same four words.  Shown below on the cases that read furthest.
EQUIVALENT = ("quad() bound", "if q + 4 <= self.nw:", "if q + 4 < self.nw:",
              ["false candidate that decodes across the end of the stream", "truncated in the middle of a symbol",
               "truncated inside the code-length list", "final block header in the last 3 bits", "dynamic block at bit 687"])


def mutant(old, new):
    src = Path(model.__file__).read_text()
    assert src.count(old) == 1, old
    spec = importlib.util.spec_from_loader("png_inflate_model_mutant", loader=None)
    mod = importlib.util.module_from_spec(spec)
    exec(compile(src.replace(old, new), "png_inflate_model_mutant", "exec"), mod.__dict__)
    return mod


@pytest.mark.parametrize("what,old,new,name", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mutated_model_fails_its_case(what, old, new, name):
    assert check(C.case(name)) is None
    with pytest.raises(AssertionError):
        check(C.case(name), mutant(old, new))


def test_the_quad_bound_mutation_is_equivalent():
    _, old, new, names = EQUIVALENT
    m = mutant(old, new)
    for name in names:
        c = C.case(name)
        assert m.decode(c["stream"], c["h"], c["rb"])[0] == model.decode(c["stream"], c["h"], c["rb"])[0]
