"""The table of hand-built deflate streams for decode_png (tests/deflate_writer.py), shared by tests/test_png_handmade_cpu.py
(the model of the kernels against zlib) and tests/test_gpu_png_handmade.py (the kernels against Pillow): what zlib's own
deflate never writes.  CASES maps a name to a builder; case(name) builds it once.

A case is a dict: mode, w, h, stream; plain (what the writer started from: filter-0 rows, then any trailing bytes) for a
valid stream; dyn (bit offsets of true dynamic blocks the mark phase must list and the walker must take from the list),
own (bit offsets of blocks the walker must decode itself), false (bit offsets of valid dynamic headers the true chain never
starts a block at: listed, decoded by pass A, ignored by the walker); end (the bit after the end-of-block code of an
alignment case); differs ((zlib's message, (code, detail) of the device)) where the kernels find another error first than
zlib does."""
import functools
import struct
import sys
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import deflate_writer as dw  # noqa: E402
import png_inflate_model as model  # noqa: E402
from test_gpu_png_decode import CTYPE, build_png, raw_rows  # noqa: E402

CHANNELS = {"L": 1, "RGB": 3, "RGBA": 4}
CASES = {}
VALID, INVALID = [], []


def register(name, valid=True):
    def deco(fn):
        CASES[name] = fn
        (VALID if valid else INVALID).append(name)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["name"] = name
    c.setdefault("mode", "L")
    c["rb"] = c["w"] * CHANNELS[c["mode"]]
    c["need"] = c["h"] * (1 + c["rb"])
    if "plain" in c:
        assert len(c["plain"]) >= c["need"]
    return c


def png_file(c):
    return build_png(c["w"], c["h"], CTYPE[c["mode"]], c["stream"])


# ---- what zlib says about a stream, as a device status ---------------------------------------------------------------
DETAIL = {"invalid block type": 1, "invalid stored block lengths": 2, "too many length or distance symbols": 3,
          "invalid code lengths set": 3, "invalid bit length repeat": 3, "invalid literal/lengths set": 3,
          "invalid distances set": 3, "invalid code -- missing end-of-block": 3, "invalid literal/length code": 4,
          "invalid distance code": 4}
MESSAGE = {(model.DEFLATE, 1): "deflate error: invalid block type", (model.DEFLATE, 2): "deflate error: stored block length",
           (model.DEFLATE, 3): "deflate error: invalid code lengths", (model.DEFLATE, 4): "deflate error: invalid code$",
           (model.DEFLATE, 5): "deflate error: stream truncated", model.FAR: "too far back", model.SHORT: "too few decoded bytes",
           model.ADLER: "Adler-32 mismatch"}


def message_of(status):
    return MESSAGE[status[0]] if status[0] in MESSAGE else MESSAGE[(status[0], status[1])]


def zlib_says(stream, need):
    """(bytes, None) where zlib inflates the stream and the picture is complete, else (None, {acceptable (code, detail)}, zlib's
    words).  The Adler-32 is zlib's "incorrect data check" only where the stream decodes to exactly ``need`` bytes: with more
    data than the picture the device does not check it (k_pd_adler), and that is by design, not an order of discovery."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream[2:]) + d.flush()
    except zlib.error as e:
        msg = str(e).split(": ", 1)[1]
        if msg == "invalid distance too far back":
            return None, {(model.FAR, None)}, msg
        return None, {(model.DEFLATE, DETAIL[msg])}, msg
    if not d.eof:
        return None, {(model.DEFLATE, 5), (model.SHORT, None)}, "incomplete or truncated stream"
    if len(out) < need:
        return None, {(model.SHORT, len(out))}, "short"
    if len(out) == need:
        if len(d.unused_data) < 4:
            return None, {(model.DEFLATE, 5), (model.SHORT, None)}, "incomplete or truncated stream"
        if d.unused_data[:4] != struct.pack(">I", zlib.adler32(out)):
            return None, {(model.ADLER, 0)}, "incorrect data check"
    return out[:need], None, None


def status_matches(status, accept):
    return any(status[0] == c and (d is None or status[1] == d) for c, d in accept)


# ---- pictures ------------------------------------------------------------------------------------------------------------
def rows_same(w, h, seed, lo=1, hi=256):
    """An L picture whose rows are all the same: any copy at a distance that is a multiple of w + 1 is right."""
    row = np.random.default_rng(seed).integers(lo, hi, w, dtype=np.uint8)
    return np.tile(row, (h, 1))


def period5(h=64, values=(150, 154, 164, 155)):
    """64 columns: with the filter byte 0 the filtered bytes have period 5."""
    row = np.array(([0] + list(values)) * 13, np.uint8)[1:]
    return np.tile(row, (h, 1))


def noise(w, h, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (h, w), dtype=np.uint8)


def exact_symbols(raw, period, n):
    """``raw`` (of the given period after its first ``period`` bytes) as exactly n symbols: the first period as literals, then
    copies at that distance and literals."""
    total = len(raw)
    r, s = total - period, n - period
    assert s >= 1 and s <= r <= 258 * s
    ncopy = 0 if r == s else max(1, -(-(r - s) // 257))
    while True:
        todo = r - (s - ncopy)                                # bytes the copies must make
        if 3 * ncopy <= todo <= 258 * ncopy:
            break
        ncopy += 1
    syms = [("lit", b) for b in raw[:period]]
    pos, lens = period, []
    for k in range(ncopy):
        ln = min(258, todo - 3 * (ncopy - k - 1))
        lens.append(ln)
        todo -= ln
    assert todo == 0
    nlit = s - ncopy
    for k in range(max(ncopy, nlit)):                         # interleaved, so that copies and literals meet in every segment
        if k < ncopy:
            syms.append(("copy", lens[k], period))
            pos += lens[k]
        if k < nlit:
            syms.append(("lit", raw[pos]))
            pos += 1
    assert pos == total and len(syms) == n and dw.plaintext(syms) == raw
    return syms


def tokenize(raw, dists, max_len=258, min_len=3, before=b""):
    """Greedy: the longest match at one of the given distances, else a literal."""
    buf = bytes(before) + bytes(raw)
    i, syms = len(before), []
    while i < len(buf):
        best = (0, 0)
        for d in dists:
            if d <= i:
                n = 0
                while n < max_len and i + n < len(buf) and buf[i + n] == buf[i + n - d]:
                    n += 1
                best = max(best, (n, -d))
        if best[0] >= min_len:
            syms.append(("copy", best[0], -best[1]))
            i += best[0]
        else:
            syms.append(("lit", buf[i]))
            i += 1
    return syms


def random_symbols(rng, raw, period, start=0, stop=None, p_copy=0.3, max_dist=32768):
    """Symbols of raw[start:stop] (of that period throughout): random copies at multiples of the period, overlaps included."""
    stop = len(raw) if stop is None else stop
    i, syms = start, []
    while i < stop:
        kmax = min(i, max_dist) // period
        if kmax and stop - i >= 3 and rng.random() < p_copy:
            d = period * int(rng.integers(1, kmax + 1)) if rng.random() < 0.5 else period * int(min(kmax, rng.integers(1, 4)))
            ln = int(min(stop - i, rng.integers(3, 259) if rng.random() < 0.5 else rng.integers(3, 12)))
            syms.append(("copy", ln, d))
            i += ln
        else:
            syms.append(("lit", raw[i]))
            i += 1
    return syms


def one_block(syms, final=True, **kw):
    sink = dw.BitSink()
    sink.raw(b"\x78\x01")
    dw.dynamic_block(sink, syms, final=final, **kw)
    return sink


def finish(sink, plain, **kw):
    return dw.zlib_stream(bytes(sink.getvalue())[2:], plain, **kw)


def start():
    sink = dw.BitSink()
    sink.raw(b"\x78\x01")
    return sink


# ---- valid: one block with a chosen symbol count ------------------------------------------------------------------------------
def symcount(n, w, h, seed):
    def build():
        img = rows_same(w, h, seed)
        raw = raw_rows(img, 0)
        sink = one_block(exact_symbols(raw, w + 1, n))
        return dict(w=w, h=h, stream=finish(sink, raw), plain=raw, **({"dyn": [16]} if n < model.PD_CAP_SYMBOLS else {"own": [16]}))
    return build


for _n in (255, 256, 257, 4095, 4096, 4097, 8192):
    register(f"symbols {_n}")(symcount(_n, 128, 128, _n))
for _n in (131071, 131072, 131073):
    register(f"over cap {_n}")(symcount(_n, 512, 512, _n))


@register("over cap 262000 then a normal block")
def _():
    img = noise(512, 512, 77)
    raw = raw_rows(img, 0)
    sink = start()
    dw.dynamic_block(sink, [("lit", b) for b in raw[:262000]])
    at = sink.nbits
    dw.dynamic_block(sink, [("lit", b) for b in raw[262000:]], final=True)
    return dict(w=512, h=512, stream=finish(sink, raw), plain=raw, own=[16], dyn=[at])


@register("over cap 262656 and 600 trailing bytes")
def _():
    img = noise(512, 512, 78)
    raw = raw_rows(img, 0) + bytes(np.random.default_rng(79).integers(0, 256, 600, dtype=np.uint8))
    sink = one_block([("lit", b) for b in raw])
    return dict(w=512, h=512, stream=finish(sink, raw), plain=raw, own=[16])


# ---- valid: code lengths ---------------------------------------------------------------------------------------------------
def p5_symbols(seed, **kw):
    raw = raw_rows(period5(), 0)
    return raw, random_symbols(np.random.default_rng(seed), raw, 5, **kw)


P5_DISTANCES = (5, 10, 15, 20, 25, 35, 50, 65, 100, 130, 195, 260, 385, 515, 770, 1025, 1540, 2050, 3075)    # 19 distance codes


def with_lengths(seed, **kw):
    def build():
        raw = raw_rows(period5(), 0)
        rng = np.random.default_rng(seed)
        syms = random_symbols(rng, raw, 5, 0, 3100, p_copy=0.5) + [("copy", 5, d) for d in P5_DISTANCES]
        syms += random_symbols(rng, raw, 5, 3100 + 5 * len(P5_DISTANCES), p_copy=0.5)
        assert dw.plaintext(syms) == raw
        sink = one_block(syms, **kw)
        return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])
    return build


for _l in (9, 10, 11, 15):
    register(f"literal/length codes up to {_l} bits")(with_lengths(_l, maxlen=_l, skew=True))
    register(f"distance codes up to {_l} bits")(with_lengths(100 + _l, d_maxlen=_l, d_skew=True))


@register("HLIT 29 and HDIST 29")
def _():
    raw, syms = p5_symbols(29)
    fl, fd = [1] * 286, [1] * 30
    for a, c, _, _ in dw.tokens(syms):
        (fl if a == "l" else fd)[c] += 50
    sink = one_block(syms, ll_lens=dw.limited_lengths(fl, 15), d_lens=dw.limited_lengths(fd, 15))
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


@register("two 1-bit code-length codes, literal-only, empty distance set")
def _():
    img = noise(64, 64, 5, hi=7) + 1                          # 7 literals (0: the filter byte, 1..7 less one) and end-of-block
    img[img == 7] = 1
    raw = raw_rows(img, 0)
    ll = [0] * 257
    for s in (0, 1, 2, 3, 4, 5, 6, 256):
        ll[s] = 3
    cl = [0] * 19
    cl[0] = cl[3] = 1
    sink = one_block([("lit", b) for b in raw], ll_lens=ll, d_lens=[0], cl_lens=cl, use=())
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


@register("literal-only noise, empty distance set")
def _():
    raw = raw_rows(noise(64, 64, 6), 0)
    sink = one_block([("lit", b) for b in raw])
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


# One block written by hand: repeats 16, 17 and 18 at their least and greatest counts, a 16 that carries length 6 from the
# last literal/length code (259) over the first three distance codes, and a code-length code of 18 entries in which
# symbol 2 (entry 15, bits 62..64 of the header: the pre-filter's straddling read) has 4 bits.
CRAFT_LL = [3] + [0] * 149 + [5] * 4 + [6] * 7 + [0] * 3 + [5] + [0] * 91 + [1, 4, 5, 6]
CRAFT_D = [6, 6, 6, 1, 2, 3, 4, 6]
CRAFT_CL_SYMS = [(3, 0), (18, 127), (18, 0), (5, 0), (16, 0), (6, 0), (16, 3), (17, 0), (5, 0), (17, 7), (18, 70), (1, 0), (4, 0),
                 (5, 0), (6, 0), (16, 0), (1, 0), (2, 0), (3, 0), (4, 0), (6, 0)]
CRAFT_CL = [0, 3, 4, 3, 4, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 3, 3]


def craft_check():
    out = []
    for s, ev in CRAFT_CL_SYMS:
        if s < 16:
            out.append(s)
        elif s == 16:
            if len(out) < len(CRAFT_LL) < len(out) + 3 + ev or len(out) == len(CRAFT_LL):
                craft_check.crossing = True
            out += [out[-1]] * (3 + ev)
        else:
            out += [0] * ((3 if s == 17 else 11) + ev)
    assert out == CRAFT_LL + CRAFT_D and len(CRAFT_LL) == 260
    assert out[259] == 6 and out[260:263] == [6, 6, 6] and CRAFT_CL_SYMS[15] == (16, 0)      # the 16 after length code 259


craft_check()


def craft_symbols(raw, start=0, stop=None):
    """raw (period 5) as literals and copies of 3, 4, 5 bytes at distances 5, 10, 15."""
    stop = len(raw) if stop is None else stop
    syms, i, k = [], start, 0
    while i < stop:
        ln, d = 3 + k % 3, 5 * (1 + (k // 3) % 3)
        if k % 4 and d <= i and i + ln <= stop:
            syms.append(("copy", ln, d))
            i += ln
        else:
            syms.append(("lit", raw[i]))
            i += 1
        k += 1
    return syms


def craft_block(sink, syms, final=True):
    dw.dynamic_block(sink, syms, final=final, ll_lens=CRAFT_LL, d_lens=CRAFT_D, cl_syms=CRAFT_CL_SYMS, cl_lens=CRAFT_CL)


@register("repeats 16 17 18 at both ends, a 16 across the alphabets")
def _():
    raw = raw_rows(period5(), 0)
    sink = start()
    craft_block(sink, craft_symbols(raw))
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


@register("distance set of one 1-bit code")
def _():
    img = np.repeat(noise(8, 64, 8), 8, axis=1)               # runs of 8 equal bytes
    raw = raw_rows(img, 0)
    sink = one_block(tokenize(raw, (1,)))
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


# ---- valid: copies ---------------------------------------------------------------------------------------------------------
@register("length 258 as 285 and as 284+31")
def _():
    raw = raw_rows(period5(), 0)
    syms = [("lit", b) for b in raw[:10]]
    i, k = 10, 0
    while i < len(raw):
        ln = min(258, len(raw) - i)
        syms.append(("copy", ln, 5 * (1 + k % 2)) + (("284+31",) if k % 2 and ln == 258 else ()))
        i += ln
        k += 1
    sink = one_block(syms)
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


@register("distance 32768 and distance equal to the output so far")
def _():
    img = rows_same(255, 255, 32768)
    raw = raw_rows(img, 0)
    syms = [("lit", b) for b in raw[:256]] + [("copy", 256, 256)]          # at byte 256: distance = output so far
    i = 512
    while i < len(raw):
        ln = min(258, len(raw) - i)
        syms.append(("copy", ln, 32768 if i >= 32768 else i if i % 512 == 0 else 256))
        i += ln
    sink = one_block(syms)
    return dict(w=255, h=255, stream=finish(sink, raw), plain=raw, dyn=[16])


@register("distance 1 runs of 258 across the picture")
def _():
    raw = raw_rows(np.zeros((64, 64), np.uint8), 0)
    sink = one_block(tokenize(raw, (1,)))
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


@register("copies from a stored block, an earlier block and across it")
def _():
    img = rows_same(64, 64, 12)
    raw = raw_rows(img, 0)
    sink = start()
    dw.stored_block(sink, raw[:130], pad=5)
    a = sink.nbits
    dw.dynamic_block(sink, [("copy", 200, 65), ("lit", raw[330])] + [("copy", 258, 130)] * 2)
    b = sink.nbits
    rest = len(raw) - 847
    dw.dynamic_block(sink, [("copy", 258, 715)] + [("copy", 129, 65)] * ((rest - 258) // 129) + [("copy", (rest - 258) % 129, 780)], final=True)
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, own=[16], dyn=[a, b])


@register("a copy that straddles the end of the picture")
def _():
    img = rows_same(64, 64, 13)
    raw = raw_rows(img, 0)
    syms = exact_symbols(raw[:4100], 65, 500) + [("copy", 200, 65)] + [("lit", 7)] * 50
    plain = dw.plaintext(syms)
    assert plain[:4160] == raw
    sink = one_block(syms)
    return dict(w=64, h=64, stream=finish(sink, plain), plain=plain, dyn=[16])


@register("overlapping copies at distances 1 2 3 4, lengths no multiple of them")
def _():
    rng = np.random.default_rng(14)
    img = np.stack([np.resize(rng.integers(5, 256, 1 + y % 4, dtype=np.uint8), 64) for y in range(64)])
    raw = raw_rows(img, 0)
    syms = tokenize(raw, (1, 2, 3, 4), max_len=59)
    assert {(s[2], s[1]) for s in syms if s[0] == "copy"} >= {(1, 59), (2, 59), (3, 59), (4, 59)}
    sink = one_block(syms)
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[16])


# ---- valid: block sequences -----------------------------------------------------------------------------------------------
@register("stored blocks of 0, 1 and 65535 bytes, padding bits set")
def _():
    raw = raw_rows(noise(64, 64, 15), 0)
    plain = raw + bytes(np.random.default_rng(16).integers(0, 256, 1 + 65535 + 3 - len(raw) + 40, dtype=np.uint8))
    sink = start()
    dw.stored_block(sink, b"", pad=0x1F)
    dw.stored_block(sink, plain[:1], pad=0x1F)
    dw.fixed_block(sink, [("lit", b) for b in plain[1:4]])    # leaves the next header off the byte boundary
    dw.stored_block(sink, plain[4:4 + 65535], pad=0x7F)
    dw.stored_block(sink, plain[4 + 65535:], final=True, pad=0x15)
    return dict(w=64, h=64, stream=finish(sink, plain), plain=plain, own=[16])


@register("300 one-literal fixed blocks")
def _():
    raw = raw_rows(noise(64, 64, 17), 0)
    sink = start()
    for b in raw[:300]:
        dw.fixed_block(sink, [("lit", b)])
    at = sink.nbits
    dw.dynamic_block(sink, [("lit", b) for b in raw[300:]], final=True)
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, own=[16, 16 + 18], dyn=[at])


@register("every ordered pair of block types, empty blocks between, final empty stored")
def _():
    img = rows_same(64, 64, 18)
    raw = raw_rows(img, 0)
    rng = np.random.default_rng(19)
    sink, pos, dyn, types = start(), 0, [], ""
    # ten data blocks with an empty stored, fixed and dynamic block after each, then four with nothing between them
    for k, t in enumerate("SSFFDDSDFS" + "SDFF"):
        n = 65 * 4
        piece = raw[pos:pos + n]
        syms = [("lit", b) for b in piece] if pos == 0 else random_symbols(rng, raw, 65, pos, pos + n)
        if t == "S":
            dw.stored_block(sink, piece, pad=k)
        elif t == "F":
            dw.fixed_block(sink, syms)
        else:
            dyn.append(sink.nbits)
            dw.dynamic_block(sink, syms)
        pos += n
        types += t
        if k < 10:
            dw.stored_block(sink, b"", pad=0x55)               # empty blocks of every type
            dw.fixed_block(sink, [])
            dyn.append(sink.nbits)
            dw.dynamic_block(sink, [])
            types += "SFD"
    dyn.append(sink.nbits)
    dw.dynamic_block(sink, random_symbols(rng, raw, 65, pos))
    dw.stored_block(sink, b"", final=True, pad=0x2A)
    types += "DS"
    assert {types[i:i + 2] for i in range(len(types) - 1)} == {a + b for a in "SFD" for b in "SFD"}
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, own=[16], dyn=dyn)


# ---- valid: alignment --------------------------------------------------------------------------------------------------------
ALIGN_FIRST = 560


def align_prefix(target):
    """(bytes of the prefix, fixed blocks) so that fixed blocks of raw[:n] literals end at bit ``target``."""
    raw = raw_rows(period5(), 0)
    for nblocks in range(1, 40):
        bits = 16 + 10 * nblocks
        for n in range(0, 400):
            if bits == target:
                return n, nblocks
            bits += 8 if raw[n] < 144 else 9
    raise AssertionError(target)


def aligned(target, final_header_last=False):
    def build():
        raw = raw_rows(period5(), 0)
        n, nblocks = align_prefix(target)
        sink = start()
        for k in range(nblocks):
            dw.fixed_block(sink, [("lit", b) for b in raw[n * k // nblocks:n * (k + 1) // nblocks]])
        assert sink.nbits == target
        craft_block(sink, craft_symbols(raw, n), final=not final_header_last)
        end = sink.nbits                                      # the bit after the end-of-block code
        own = [16]
        if final_header_last:
            assert sink.nbits % 8 == 5
            own.append(sink.nbits)
            dw.stored_block(sink, b"", final=True)
        return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, dyn=[target], own=own, end=end)
    return build


for _k in range(128):
    register(f"dynamic block at bit {ALIGN_FIRST + _k}")(aligned(ALIGN_FIRST + _k))


def _final_header_target():
    raw = raw_rows(period5(), 0)
    for t in range(ALIGN_FIRST, ALIGN_FIRST + 128):
        n, _ = align_prefix(t)
        sink = dw.BitSink()
        sink.put(0, t % 8)
        craft_block(sink, craft_symbols(raw, n), final=False)
        if sink.nbits % 8 == 5:
            return t
    raise AssertionError


register("final block header in the last 3 bits")(lambda: aligned(_final_header_target(), True)())


# ---- valid: false candidates -----------------------------------------------------------------------------------------------
def false_block(eob=True, lits=(9, 8, 7, 9, 9, 8, 200, 9), copy=(4, 2), **kw):
    """A complete dynamic block of a few symbols, as bytes (and its length in bits)."""
    sink = dw.BitSink()
    dw.dynamic_block(sink, [("lit", b) for b in lits] + [("copy",) + tuple(copy)], eob=eob, **kw)
    n = sink.nbits
    return sink.getvalue(pad=0), n


def bits_of(data, n):
    return [(data[i >> 3] >> (i & 7)) & 1 for i in range(n)]


FIXED_SYMBOL = {v: s for s, v in dw.canonical(dw.FIXED_LL).items()}


def fixed_literals(bits, stop):
    """``bits`` read as symbols of the fixed code up to the first symbol boundary at or after ``stop``: (the literals, that
    boundary), or None where one of them is no literal.  The fixed code is complete, so any bits are symbols; the bits past
    the end of the list are zeros."""
    out, i = [], 0
    while i < stop:
        code, n = 0, 0
        while (code, n) not in FIXED_SYMBOL:
            code, n = code << 1 | (bits[i + n] if i + n < len(bits) else 0), n + 1
        if FIXED_SYMBOL[code, n] > 255:
            return None
        out.append(FIXED_SYMBOL[code, n])
        i += n
    return out, i


def false_block_of_fixed_literals(first, tries=20000):
    """(pad bits, false block's bits, literals): a false block after 1..7 pad bits, such that a fixed block whose symbols
    reach bit ``first`` goes on with literals alone through all of it, and the false block starts off the byte boundary.
    The search varies the block's literals, its copy, the longest code and the code-length code: all 19 of its lengths are
    sent and none is zero, since no literal of the fixed code has more than seven zero bits in a row and the header that
    dynamic_block() writes by default has runs of a dozen.  A symbol is a literal with probability 0.78 and the block is
    some 30 to 50 symbols long: about one try in a thousand is kept."""
    rng = np.random.default_rng(23)
    for _ in range(tries):
        lits = [int(x) for x in rng.integers(0, 256, 8)]
        cl = dw.limited_lengths([int(x) for x in rng.integers(1, 40, 19)], 7)
        blk, nbits = false_block(lits=lits, copy=(int(rng.integers(3, 12)), int(rng.integers(1, 9))), maxlen=int(rng.integers(4, 10)),
                                 cl_lens=cl)
        npad = int(rng.integers(1, 8))
        pad = [int(x) for x in rng.integers(0, 2, npad)]
        if (first + npad) % 8 == 0 or npad + nbits > 440:
            continue
        got = fixed_literals(pad + bits_of(blk, nbits), npad + nbits)
        if got is not None:
            return pad, bits_of(blk, nbits), got[0]
    raise AssertionError("no false block that reads as literals of the fixed code")


@register("false candidate in a stored block's payload")
def _():
    img = noise(64, 64, 20)
    blk, _ = false_block()
    assert len(blk) < 60
    img[3, 2:2 + len(blk)] = np.frombuffer(blk, np.uint8)
    raw = raw_rows(img, 0)
    sink = start()
    dw.stored_block(sink, raw[:1000])
    at = sink.nbits - 8 * 1000 + 8 * (3 * 65 + 3)
    dw.dynamic_block(sink, [("lit", b) for b in raw[1000:]], final=True)
    return dict(w=64, h=64, stream=finish(sink, raw), plain=raw, own=[16], false=[at])


@register("false candidate in the literals of a fixed block, off every symbol boundary")
def _():
    img = noise(64, 64, 24)
    before = 3 * 65 + 3                                       # the literals that hold it start at row 3, column 2
    pre = raw_rows(img, 0)[:before]
    width = [8 if b < 144 else 9 for b in pre]
    first = 16 + 3 + sum(width)
    pad, fbits, lits = false_block_of_fixed_literals(first)
    assert len(lits) <= 60
    img[3, 2:2 + len(lits)] = lits
    raw = raw_rows(img, 0)
    assert raw[:before] == pre and raw[before:before + len(lits)] == bytes(lits)
    sink = start()
    dw.fixed_block(sink, [("lit", b) for b in raw[:1000]])
    nxt = sink.nbits
    dw.dynamic_block(sink, [("lit", b) for b in raw[1000:]], final=True)
    stream = finish(sink, raw)
    at = first + len(pad)
    assert bits_of(stream, at + len(fbits))[at:] == fbits     # the false block, bit for bit, inside the fixed block's symbols
    bounds, p = {16, nxt}, 19
    for b in raw[:1000]:
        bounds.add(p)
        p += 8 if b < 144 else 9
    bounds.add(p)                                             # the end-of-block code
    assert p + 7 == nxt and at % 8 and at not in bounds and 19 < at < nxt
    return dict(w=64, h=64, stream=stream, plain=raw, own=[16], dyn=[nxt], false=[at])


@register("false candidate in trailing data")
def _():
    raw = raw_rows(noise(64, 64, 21), 0)
    sink = one_block([("lit", b) for b in raw])
    blk, _ = false_block()
    stream = finish(sink, raw, trailing=b"\x00" + blk + b"\x00" * 8)
    return dict(w=64, h=64, stream=stream, plain=raw, dyn=[16], false=[8 * (len(stream) - len(blk) - 8)])


@register("false candidate that decodes across the end of the stream")
def _():
    raw = raw_rows(noise(64, 64, 22), 0)
    sink = one_block([("lit", b) for b in raw])
    blk, nbits = false_block(eob=False)
    stream = finish(sink, raw, trailing=b"\x00" + blk)
    return dict(w=64, h=64, stream=stream, plain=raw, dyn=[16], false=[8 * (len(stream) - len(blk))])


# ---- invalid ------------------------------------------------------------------------------------------------------------------
SMALL = raw_rows(np.tile(np.array([[3, 4, 5, 6, 7, 8, 9, 10]], np.uint8), (8, 1)), 0)     # 8 x 8, L: 72 filtered bytes


def invalid(name, differs=None):
    def deco(fn):
        def build():
            sink = start()
            kw = fn(sink) or {}
            cut = kw.pop("cut", None)
            stream = finish(sink, SMALL, **kw)
            if cut is not None:
                stream = stream[:cut(stream)]
            c = dict(w=8, h=8, stream=stream)
            if differs:
                c["differs"] = differs
            return c
        register(name, valid=False)(build)
        return fn
    return deco


LITS = [("lit", b) for b in SMALL]


@invalid("invalid block type")
def _(s):
    s.put(1, 1)
    s.put(3, 2)


@invalid("stored block with a wrong NLEN")
def _(s):
    dw.stored_block(s, SMALL, final=True, nlen=0x1234)


@invalid("HLIT 30")
def _(s):
    dw.dynamic_block(s, LITS, final=True, hlit=30)


@invalid("HDIST 30")
def _(s):
    dw.dynamic_block(s, LITS, final=True, hdist=30)


@invalid("code-length code over-subscribed")
def _(s):
    cl = [0] * 19
    cl[0] = cl[3] = cl[4] = 1
    dw.dynamic_block(s, LITS, final=True, cl_lens=cl, cl_syms=[(3, 0), (4, 0), (0, 0)])


@invalid("code-length code incomplete")
def _(s):
    cl = [0] * 19
    cl[0], cl[3], cl[4] = 1, 2, 3
    dw.dynamic_block(s, LITS, final=True, cl_lens=cl, cl_syms=[(3, 0), (4, 0), (0, 0)])


@invalid("HCLEN 0: no literal/length code can be sent, so no end-of-block")
def _(s):
    cl = [0] * 19
    cl[0] = cl[18] = 1
    dw.dynamic_block(s, [], final=True, ll_lens=[0] * 257, d_lens=[0], cl_lens=cl, cl_syms=[(18, 127), (18, 109)], hclen=0, eob=False)


@invalid("16 as the first code-length symbol")
def _(s):
    ll = [0] * 257
    ll[0] = ll[256] = 1
    dw.dynamic_block(s, [], final=True, ll_lens=ll, d_lens=[0], cl_syms=[(16, 0), (1, 0), (18, 127), (18, 103), (1, 0), (0, 0)])


@invalid("repeat past HLIT + HDIST")
def _(s):
    ll = [0] * 257
    ll[0] = ll[256] = 1
    dw.dynamic_block(s, [], final=True, ll_lens=ll, d_lens=[0], cl_syms=[(1, 0), (18, 127), (18, 106), (1, 0), (17, 0)])


@invalid("literal/length set over-subscribed")
def _(s):
    ll = [0] * 257
    ll[3] = ll[4] = ll[256] = 1
    dw.dynamic_block(s, [("lit", 3)], final=True, ll_lens=ll, d_lens=[0])


@invalid("literal/length set incomplete")
def _(s):
    ll = [0] * 257
    ll[3], ll[4], ll[256] = 1, 2, 3
    dw.dynamic_block(s, [("lit", 3)], final=True, ll_lens=ll, d_lens=[0])


@invalid("distance set over-subscribed")
def _(s):
    dw.dynamic_block(s, LITS, final=True, d_lens=[1, 1, 1])


@invalid("distance set incomplete")
def _(s):
    dw.dynamic_block(s, LITS, final=True, d_lens=[1, 2, 3])


@invalid("no code for end-of-block")
def _(s):
    ll = [0] * 257
    ll[3] = ll[4] = 1
    dw.dynamic_block(s, [("lit", 3)], final=True, ll_lens=ll, d_lens=[0], eob=False)


@invalid("fixed code 286")
def _(s):
    dw.fixed_block(s, LITS[:5] + [("raw", 286, 0, 0)], final=True)


@invalid("fixed code 287")
def _(s):
    dw.fixed_block(s, LITS[:5] + [("raw", 287, 0, 0)], final=True)


@invalid("fixed distance code 30")
def _(s):
    dw.fixed_block(s, LITS[:5] + [("raw", 257, 0, 0), ("rawdist", 30, 0, 0)], final=True)


@invalid("fixed distance code 31")
def _(s):
    dw.fixed_block(s, LITS[:5] + [("raw", 257, 0, 0), ("rawdist", 31, 0, 0)], final=True)


@invalid("the unused code of a one-code distance set")
def _(s):
    dw.dynamic_block(s, LITS[:5] + [("raw", 257, 0, 0)], d_lens=[1], eob=False)
    s.put(1, 1)
    s.put(0, 20)


@invalid("a length symbol under an empty distance set")
def _(s):
    ll = dw.limited_lengths([1 if (3 <= i <= 10 or i in (0, 256, 257)) else 0 for i in range(258)], 15)
    dw.dynamic_block(s, LITS[:5] + [("raw", 257, 0, 0)], ll_lens=ll, d_lens=[0], eob=False)
    s.put(0, 24)


@invalid("one-code literal/length set, the other bit")
def _(s):
    ll = [0] * 257
    ll[256] = 1
    dw.dynamic_block(s, [], final=True, ll_lens=ll, d_lens=[0], eob=False)
    s.put(1, 1)
    s.put(0, 20)


@invalid("copy one byte too far back in the first block")
def _(s):
    dw.fixed_block(s, LITS[:5] + [("copy", 3, 6)] + LITS[8:], final=True)


@invalid("copy one byte too far back in the fifth block")
def _(s):
    for k in range(4):
        dw.fixed_block(s, LITS[8 * k:8 * k + 8])
    dw.dynamic_block(s, [("copy", 3, 33)] + LITS[35:], final=True)


@invalid("wrong Adler-32")
def _(s):
    dw.dynamic_block(s, LITS, final=True)
    return {"adler": "wrong"}


@invalid("too few bytes, stream complete")
def _(s):
    dw.dynamic_block(s, LITS[:60], final=True)


def cut_at(marker_bits):
    return lambda stream: (marker_bits["at"] + 7) // 8


@invalid("truncated inside a stored LEN")
def _(s):
    dw.fixed_block(s, LITS[:8])
    dw.stored_block(s, SMALL[8:], final=True)
    n = len(s.out) - len(SMALL[8:]) - 3
    return {"cut": lambda stream: n}


# HLIT, HDIST and HCLEN are there, the code-length code is cut: pd_header reads the missing lengths as zero bits and finds
# the code incomplete before it asks whether it has read past the end; zlib asks for more input first
@invalid("truncated inside a dynamic header", differs=("incomplete or truncated stream", (model.DEFLATE, 3)))
def _(s):
    dw.fixed_block(s, LITS[:8])
    at = s.nbits
    dw.dynamic_block(s, LITS[8:], final=True)
    return {"cut": lambda stream: (at + 14) // 8}


@invalid("truncated inside the code-length list")
def _(s):
    dw.fixed_block(s, LITS[:8])
    at = s.nbits
    dw.dynamic_block(s, LITS[8:], final=True)
    return {"cut": lambda stream: (at + 17 + 57 + 30) // 8}


@invalid("truncated in the middle of a symbol")
def _(s):
    dw.dynamic_block(s, LITS, final=True)
    n = len(s.getvalue())
    return {"cut": lambda stream: n - 9}


@invalid("truncated between the last block and the Adler-32")
def _(s):
    dw.dynamic_block(s, LITS, final=True)
    return {"cut": lambda stream: len(stream) - 4}


for _k in (1, 2, 3):
    def _cut(s, k=_k):
        dw.dynamic_block(s, LITS, final=True)
        return {"adler": 4 - k}
    invalid(f"truncated {_k} bytes into the Adler-32")(_cut)


@invalid("an invalid block type after the picture is complete")
def _(s):
    dw.dynamic_block(s, LITS)
    s.put(0, 1)
    s.put(3, 2)
    s.put(0, 16)


GOOD = "symbols 255"                                          # the file decoded after every error
