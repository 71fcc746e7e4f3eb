"""The table of hand-built LZW streams for decode_tiff (tests/lzw_writer.py), shared by tests/test_tiff_handmade_cpu.py (the
model of k_td_lzw against the host decoder) and tests/test_gpu_tiff_handmade.py (the kernel against tiffio.read_tiff): what no
encoder writes.  CASES maps a name to a builder; case(name) builds it once.

A case is a dict: stream, ndst (the bytes of the chunk it is decoded into); plain (the whole plaintext of the codes, by the
writer's own string table) where the stream is valid by construction; claims (what the model's event record must show, so
that a case is known to reach what its name says: a set must be contained in the record's, NAME_min is a lower bound, anything
else is equal).  The expectation itself is the host decoder's answer, tiff_cases.host_lzw(stream, ndst); for a case with a
plaintext it must be (plain[:ndst], 0).  SLOW names the cases whose model run takes seconds: they have test functions of
their own."""
import functools

import numpy as np

import lzw_writer as lw
from lzw_writer import CLEAR, EOI, FIRST, Writer

CASES = {}
VALID, INVALID, SLOW = [], [], []
FREEZE = 3839                    # the first index whose code is read from a frozen table
GOOD = "a 63-deep dependency chain inside one batch, not all one byte value"


def register(name, valid=True, slow=False):
    def deco(fn):
        CASES[name] = fn
        (SLOW if slow else VALID if valid else INVALID).append(name)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["name"] = name
    c.setdefault("claims", {})
    return c


def done(w, ndst=None, tail=b"", **claims):
    """The case of a writer whose codes are all valid: its stream, its plaintext, ndst = the plaintext's length + ``ndst`` (an
    offset) and the claims."""
    plain = w.plain()
    assert len(plain) == w.n
    return dict(stream=w.stream() + tail, ndst=len(plain) + (ndst or 0), plain=plain, claims=claims)


def damaged(w, stream=None, extra=64, **claims):
    """The case of a stream that is not valid by construction: the chunk is ``extra`` bytes larger than what the valid codes
    give, so that the decoder reaches the damage."""
    return dict(stream=w.stream() if stream is None else stream, ndst=w.n + extra, claims=claims)


def rng_of(seed):
    return np.random.default_rng(20261018 + seed)


def walk(seed, count, literals=256):
    """A segment of ``count`` random valid codes behind a Clear."""
    return Writer().random(rng_of(seed), count, literals=literals)


# ---- the full table: i >= 3838 ---------------------------------------------------------------------------------------
def frozen_run(k):
    def build():
        w = walk(k, FREEZE + k).eoi()
        return done(w, max_i=FREEZE - 1 + k, pcap_batches_min=1 if k > 1 else 0)
    return build


for _k in (1, 64, 250):
    register(f"full table: {_k} code(s) past i = 3839 without Clear")(frozen_run(_k))


@register("full table: codes 4094 and 4095 used after the freeze, in front of the batch and inside it")
def _():
    w = walk(3, FREEZE + 70)
    w.put(4095).put(4094).lit(9).put(4095).put(4095).put(4094)
    w.random(rng_of(4), 130).put(4094).put(4095).eoi()
    return done(w, max_i_min=FREEZE + 200, pcap_batches_min=2)


@register("full table: code 4095 at i = 3838 is the fill level, the last entry")
def _():
    w = walk(5, FREEZE - 1)
    assert w.i == 3838 and FIRST + w.fill_j() == 4095
    w.fill().put(4095).lit(1).put(4095).eoi()
    return done(w, max_i=FREEZE + 2)


@register("full table: code 4095 at i = 3837 is above the table", valid=False)
def _():
    w = walk(6, FREEZE - 2)
    assert w.i == 3837 and w.fill_j() == 3836
    w.put(4095).lit(1, 2, 3).eoi()
    return damaged(w, max_i=3836)


@register("full table: code 4094 at i = 3837 is the fill level, 4095 follows at i = 3838")
def _():
    w = walk(7, FREEZE - 2).fill().fill().eoi()
    assert w.codes[-3:] == [4094, 4095, EOI]
    return done(w, max_i=3838)


@register("full table: Clear after a frozen stretch, then a normal segment (no stale P[] entry is read)")
def _():
    w = walk(8, FREEZE + 150).clear().random(rng_of(9), 400, literals=3).clear().random(rng_of(10), 90).eoi()
    return done(w, pcap_batches_min=2)


@register("full table: a frozen stream that ends without EOI exactly at the chunk's size")
def _():
    return done(walk(11, FREEZE + 100), max_i=FREEZE + 99)


@register("full table: a frozen stream that ends without EOI five bytes short of the chunk")
def _():
    return done(walk(11, FREEZE + 100), ndst=5, max_i=FREEZE + 99)


@register("full table: a frozen stream cut inside a 12-bit code")
def _():
    w = walk(12, FREEZE + 100)
    stream = w.stream()[:(lw.bit_length(w.codes) - 1) // 8]         # the last code loses 1 to 8 of its 12 bits
    plain = lw.plaintext(w.codes[:-1])
    return dict(stream=stream, ndst=w.n, plain=plain, claims=dict(max_i=FREEZE + 98))


# ---- long strings ----------------------------------------------------------------------------------------------------
def grow(w, seed, varied, upto):
    """Codes behind which the last code's string is ``upto`` bytes long: ``varied`` bytes of it are seeded values (two codes a
    byte: the entry so far, then a literal), the rest repeats its first byte (the fill-level code each time, KwKwK)."""
    s = rng_of(seed).integers(1, 256, varied).tolist()
    w.lit(s[0])
    for b in s[1:]:
        w.lit(b).entry(w.i - 2)
    while w.lengths[-1] < upto:
        w.fill()
    assert w.lengths[-1] == upto
    return w


@register("long strings: the zero chain to 3839 bytes, the longest string six times, ordinary codes behind it", slow=True)
def _():
    w = Writer().lit(0)
    for _ in range(3838):
        w.fill()
    assert w.codes[-1] == 4095 and w.lengths[-1] == 3839
    for _ in range(5):
        w.put(4095)
    w.lit(7).put(4095).put(4094).put(300).eoi()
    return done(w, max_L=3839, stage_full_min=1800, max_i=FREEZE + 8)


def zero_chain_clipped(ndst):
    def build():
        c = case("long strings: the zero chain to 3839 bytes, the longest string six times, ordinary codes behind it")
        return dict(stream=c["stream"], ndst=ndst, plain=c["plain"][:ndst + 1])
    return build


register("long strings: the zero chain decoded into a chunk of 1 byte")(zero_chain_clipped(1))
register("long strings: the zero chain decoded into a chunk of 3839 bytes")(zero_chain_clipped(3839))


def batch_starts(lengths, stage=4096):
    """Where the batches of a segment of valid codes begin, as the kernel cuts them: 64 codes, or as many as fit the stage.
    The cases use it to place a code at a chosen lane; their claims check the placing against the model."""
    starts, at = [], 0
    while at < len(lengths):
        starts.append(at)
        n, total = 0, 0
        while n < 64 and at + n < len(lengths) and total + lengths[at + n] <= stage:
            total += lengths[at + n]
            n += 1
        at += n
    return starts


def pad_to_batch_start(w, nxt):
    """Literals until a code of ``nxt`` bytes would open a batch."""
    while batch_starts(w.lengths + [nxt])[-1] != w.i:
        w.lit(5)
    return w


def long_pair(n):
    def build():
        """The chain to ``n`` bytes; then, at the start of a batch, two strings of n bytes, a literal and the second string's own
        entry: a copy of n + 1 bytes whose source begins in front of that literal and ends with it."""
        w = grow(Writer(), n, 40, n)
        a = w.i - 1                                # the code of n bytes; entry a - 1 has n bytes too
        pad_to_batch_start(w, n).entry(a - 1).entry(a - 1)
        x = w.i - 1
        w.lit(6).entry(x).lit(7).entry(a).eoi()
        claims = dict(max_L=n + 1)
        if n == 2048:                              # 2048 + 2048 fills the stage to the byte; the literal opens the next batch
            claims.update(totals={4096}, dep_b={"lane0"}, straddle_L=2049, next_lanes={1})
        else:                                      # 2049 + 2049 = 4098: cut after the first
            claims.update(totals={2049})
        return done(w, **claims)
    return build


for _n in (2048, 2049):
    register(f"long strings: strings of {_n} bytes, " + ("two of them fill one batch, a copy of 2049 bytes whose source straddles op"
                                                         if _n == 2048 else "two in a row that cannot share a batch"), slow=True)(long_pair(_n))


def batch_sum(last):
    def build():
        """Batch 0: the chain to 64 bytes (2080 bytes); batch 1: 63 strings of 64 bytes and one of ``last``."""
        w = Writer().lit(3)
        for _ in range(63):
            w.fill()
        assert w.i == 64 and w.lengths[-1] == 64
        for _ in range(63):
            w.entry(62)
        w.entry(62 + last - 64).lit(8, 9).entry(70).eoi()
        return done(w, totals={2080, 4096 if last == 64 else 4032}, stage_full=0 if last == 64 else 1)
    return build


register("long strings: a batch of 64 codes whose inclusive sum is exactly 4096")(batch_sum(64))
register("long strings: a batch of 64 codes whose inclusive sum is 4097 at the last lane")(batch_sum(65))


# ---- code choices within a batch -------------------------------------------------------------------------------------
@register("batch: the fill-level code at lane 0 and at lane 63")
def _():
    w = walk(20, 64).fill().random(rng_of(21), 62).fill().random(rng_of(22), 10).eoi()
    return done(w, fill_lanes={0, 63})


@register("batch: an entry j with j + 1 == seg_i, seen from lanes 1 and 63")
def _():
    w = walk(23, 64, literals=4).lit(200).entry(63)
    w.random(rng_of(24), 61, literals=4).entry(63).random(rng_of(25), 10).eoi()
    return done(w, next_lanes={1, 63}, dep_b={"lane0"})


@register(GOOD)
def _():
    w = Writer().lit(10, 20)
    for _ in range(62):
        w.entry(w.i - 2)
    w.lit(30).eoi()
    plain = w.plain()
    assert len(set(plain)) == 3 and plain[2:4] == bytes([10, 20])
    return done(w, rounds_min=63, dep_b={"inside"})


@register("batch: every kind of second dependency in one batch, the fill-level code after a cut batch")
def _():
    w = grow(Writer(), 26, 30, 200)
    w.random(rng_of(27), 200, literals=2).eoi()
    return done(w, dep_b={"self", "none", "inside", "lane0"}, stage_full_min=1)


# ---- Clear, EOI and the width changes --------------------------------------------------------------------------------
@register("clear: Clear at each of the 64 lanes")
def _():
    w, rng = Writer(), rng_of(30)
    for lane in range(64):
        w.random(rng, lane, literals=5).clear()
    w.random(rng, 20).eoi()
    return done(w, clear_lanes=set(range(64)))


def eoi_at(lane):
    def build():
        w = walk(31 + lane, 64 + lane, literals=7).eoi()
        return done(w, ndst=3, tail=b"\xff\xff\xff", eoi_lanes={lane})
    return build


for _lane in (0, 1, 62, 63):
    register(f"clear: EOI at lane {_lane}, corrupt codes behind it, chunk 3 bytes short")(eoi_at(_lane))


@register("clear: two and three Clears in a row, at the start, in the middle and before EOI")
def _():
    w = Writer().clear().random(rng_of(40), 70).clear().clear().clear().random(rng_of(41), 30).clear().clear().eoi()
    return done(w, ndst=1, clear_lanes={0})


@register("clear: Clear followed directly by EOI")
def _():
    return done(Writer().eoi(), ndst=1)


@register("clear: EOI alone")
def _():
    return done(Writer(leading_clear=False).eoi(), ndst=1)


@register("clear: a zero-length stream")
def _():
    return dict(stream=b"", ndst=1, plain=b"")


@register("clear: no leading Clear")
def _():
    w = Writer(leading_clear=False).lit(65).random(rng_of(42), 300, literals=6).clear().random(rng_of(43), 20).eoi()
    return done(w)


def width_change(last, code, after):
    def build():
        """``code`` (Clear or EOI) as code ``last`` of a segment, the last of its width, or as code ``last`` + 1."""
        at = last + after
        w = walk(at, at, literals=16)
        assert w.i == at and lw.width_of(at) == lw.width_of(last) + after
        if code == EOI:
            return done(w.eoi(), ndst=2, tail=b"\xff\xff", first_at={at})
        w.clear().random(rng_of(at + 1), 300, literals=16).eoi()
        return done(w, first_at={at})
    return build


for _last in (253, 765, 1789):
    for _code in (CLEAR, EOI):
        for _after in (0, 1):
            register(f"width: {'Clear' if _code == CLEAR else 'EOI'} at i = {_last + _after}, the "
                     f"{'first' if _after else 'last'} code of its width")(width_change(_last, _code, _after))


@register("width: data codes on both sides of every change, Clear as the code behind it")
def _():
    w = walk(50, 1795).clear().random(rng_of(51), 770).clear().random(rng_of(52), 258).clear().lit(1).eoi()
    return done(w)


@register("clear: a first code >= 258 after a Clear in mid-stream", valid=False)
def _():
    w = walk(53, 100).clear().put(FIRST).lit(1, 2).eoi()
    return damaged(w)


@register("clear: a first code >= 258 where the stream has no leading Clear", valid=False)
def _():
    return damaged(Writer(leading_clear=False).put(300).lit(1).eoi())


@register("batch: a code one above the fill level at lane 63", valid=False)
def _():
    w = walk(54, 63)
    assert w.fill_j() == 62
    return damaged(w.put(FIRST + 63).lit(1).eoi(), max_i=62)


@register("batch: a code one above the fill level at lane 0", valid=False)
def _():
    w = walk(55, 128)
    assert w.fill_j() == 127
    return damaged(w.put(FIRST + 128).lit(1).eoi(), max_i=127)


# ---- the end of the chunk --------------------------------------------------------------------------------------------
def chunk_end(offset):
    def build():
        w = walk(60, 200, literals=3)
        w.entry(int(np.argmax(w.lengths[:w.held()])))
        assert w.lengths[-1] >= 3
        n = w.n
        w.lit(1, 2).put(511)                       # 511 is above the table: corrupt if it were read
        return dict(stream=w.stream(), ndst=n + offset, plain=lw.plaintext(w.codes[:-1]))
    return build


register("end: a code that ends exactly at ndst, a corrupt code behind it")(chunk_end(0))
register("end: a code that ends one byte over ndst, a corrupt code behind it")(chunk_end(-1))
register("end: a code that ends one byte short of ndst, a literal fills it, a corrupt code behind it")(chunk_end(1))


@register("end: the stream ends one byte short of ndst")
def _():
    return done(walk(61, 200, literals=3).eoi(), ndst=1)


def literal_fills(then, unread=(), valid=True):
    def build():
        """Clear, literal: the chunk is full and the host decoder goes on reading ``then``; it never reads ``unread``."""
        w = walk(62, 100, literals=3).clear().lit(77)
        n = w.n
        for code in then:
            w.put(code)
        c = dict(stream=lw.pack(w.codes + list(unread)), ndst=n)
        if valid:
            c["plain"] = lw.plaintext(w.codes)
        return c
    return build


register("end: the literal that fills the chunk, then Clear and more codes")(literal_fills([CLEAR, 1], [2, FIRST, 300, EOI]))
register("end: the literal that fills the chunk, then Clear, Clear, a literal and a corrupt code")(literal_fills([CLEAR, CLEAR, 1], [300]))
register("end: the literal that fills the chunk, then a literal")(literal_fills([5], [300, EOI]))
register("end: the literal that fills the chunk, then the fill-level code")(literal_fills([FIRST], [300, EOI]))
register("end: the literal that fills the chunk, then EOI and corrupt codes")(literal_fills([EOI], [400, 400]))
register("end: the literal that fills the chunk, then a code above the table", valid=False)(literal_fills([FIRST + 1, EOI], valid=False))


@register("end: a one-byte chunk, a literal, then a code above the table", valid=False)
def _():
    return dict(stream=lw.pack([CLEAR, 9, 300, EOI]), ndst=1)


@register("end: a one-byte chunk filled by a first literal without a leading Clear, the stream ends")
def _():
    return dict(stream=lw.pack([9]), ndst=1, plain=b"\x09")


@register("end: trailing bytes after EOI that would be corrupt codes if read")
def _():
    return done(walk(63, 150).eoi(), ndst=2, tail=bytes([0xFF]) * 40)


# ---- a greedy encoder with a chosen clear policy ---------------------------------------------------------------------
def encoded(data, **policy):
    def build():
        codes = lw.encode(data(), **policy)
        plain = lw.plaintext(codes)
        assert plain == data()
        claims = {}
        if policy.get("clear_at") is None or policy.get("frozen_run"):
            claims = dict(max_i_min=FREEZE + 50)
        return dict(stream=lw.pack(codes), ndst=len(plain), plain=plain, claims=claims)
    return build


def noise():
    return rng_of(70).integers(0, 3, 60000, dtype=np.uint8).tobytes()


register("encoder: never clearing, 60 000 bytes over 3 symbols")(encoded(noise))
register("encoder: Clear when the table is full (4096)")(encoded(noise, clear_at=4096))
register("encoder: Clear at 4095")(encoded(noise, clear_at=4095))
register("encoder: a deferred Clear, 300 codes after the table froze")(encoded(noise, clear_at=4096, frozen_run=300))
register("encoder: clearing early, at 300 codes")(encoded(noise, clear_at=300))
register("encoder: never clearing, no leading Clear, no EOI")(encoded(lambda: b"\x01" + noise()[:30000], leading_clear=False, eoi=False))


# ---- the seeded fuzz -------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_STREAMS = 20261018, 2000


def fuzz_stream(rng):
    """(codes, plaintext) of one stream that is valid by construction but not greedy: a few tens to a few hundred codes, one in
    40 of about 4000 codes without Clear, past the freeze; seeded Clears in the others; literals from an alphabet of 2 to 256 values."""
    long = rng.random() < 0.025
    count = int(rng.integers(3850, 4300)) if long else int(rng.integers(1, 700))
    literals = int(rng.choice([2, 4, 32, 256]))
    w = Writer(leading_clear=rng.random() > 0.1)
    if not w.codes:
        w.lit(int(rng.integers(2, 256)))                   # 00 and an odd byte first would read as old-style LZW
    w.random(rng, count, p_clear=0.0 if long else float(rng.choice([0, 0, 0.002, 0.02, 0.2])), literals=literals)
    if rng.random() > 0.15:
        w.eoi()
    return w.codes, w.plain()


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    """FUZZ_STREAMS of (kind, stream, ndst, plaintext or None): every fourth is cut, every fourth has bits flipped, every
    fourth has a code spliced in (Clear, EOI, the code above the fill level, any 12-bit value)."""
    rng = np.random.default_rng(FUZZ_SEED)
    out = []
    for k in range(FUZZ_STREAMS):
        codes, plain = fuzz_stream(rng)
        ndst = max(1, len(plain) + int(rng.choice([0, 0, 0, -1, 1, 7, -len(plain) // 2])))
        kind = ("valid", "cut", "flip", "splice")[k % 4]
        stream = lw.pack(codes)
        if kind == "cut":
            stream = stream[:int(rng.integers(0, len(stream)))]
        elif kind == "flip":
            s = bytearray(stream)
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            stream = bytes(s)
        elif kind == "splice":
            at = int(rng.integers(0, len(codes) + 1))
            i = 0
            for c in codes[:at]:
                i = 0 if c == CLEAR else i + 1
            new = [CLEAR, EOI, FIRST + i, FIRST + max(i - 1, 0), int(rng.integers(0, 4096))][int(rng.integers(0, 5))]
            codes = codes[:at] + [new] + codes[at:] if rng.random() < 0.5 else codes[:at] + [new] + codes[at + 1:]
            stream = lw.pack(codes)
        out.append((kind, stream, ndst, plain if kind == "valid" else None))
    return out


def old_style(stream):
    """What lars_tiff_info refuses before any kernel runs: 00 and an odd byte first."""
    return len(stream) >= 2 and stream[0] == 0 and stream[1] & 1
