"""The phases of k_td_inflate (csrc/tiff_decode.hip) restated in Python / NumPy: the zlib header, the block headers and their
tables (pd_header of csrc/inflate_device.h, in the order that stops at the end of the input before it judges), batches of
TD_ZBATCH records decoded by one lane from a window of TD_ZWIN staged bytes, their expansion into the chunk buffer by the wave
(literals first, then each copy with src = o - dist + k % dist), Adler-32 from the sums the lanes keep, and the walk after the
chunk is full.  Every index the kernel forms is asserted here.  The specification is tiffio._chunk on zlib: test_tiff_deflate_cpu.py holds the two together.

What zlib.decompressobj().decompress(raw, want) does, as far as _chunk can see it:
  * out of input is never an error, wherever it happens: a value whose bits are not all there is not judged, decoding stops;
  * a value whose bits are there is judged at once, also after `want` bytes: block type 3, LEN / NLEN, HLIT / HDIST, the
    code-length code (once all its lengths are there), repeats (once their extra bits are there), the two codes (once every
    length is there), a literal/length or distance code without a symbol (one bit is enough: zlib's tables mark it with one
    bit), length symbols 286 / 287 and distance symbols 30 / 31 (their code is enough);
  * with the chunk full, end-of-block codes, block headers and empty stored blocks go by; the first literal, match (after
    its distance's extra bits; the distance itself is not judged any more) or stored byte stops the decoder, and what it
    has not yet taken from the input is unconsumed_tail: "inflates past" exactly when a whole byte is left, so a stream cut
    right behind that symbol is accepted;
  * a distance larger than the bytes produced so far is corrupt while there is room; the header's window size limits nothing;
  * after the final block the Adler-32 trailer is compared when its four bytes are there, and what follows is ignored.
"""
import numpy as np

from deflate_writer import CLORDER, DBASE, DEXT, LBASE, LEXT

BATCH = 256                 # TD_ZBATCH: records one lane decodes between two expansions
WIN = 2048                  # TD_ZWIN: bytes of the stream staged in LDS for one batch
FB = 10                     # PD_FB: bits of the first-level tables
WAVE = 64
ADLER = 65521
OK, CORRUPT, PAST = 0, 1, 2  # bad[k] of the kernel


class Bits:
    """The chunk's bytes as the bit reader sees them: LSB first, zero words behind the last byte; no byte past it is loaded."""

    def __init__(self, data):
        self.data = bytes(data)
        self.cnt = len(self.data)
        self.nbits = 8 * self.cnt
        self.big = int.from_bytes(self.data, "little")

    def peek(self, pos, n):
        assert 0 <= n <= 32 and pos >= 0
        assert pos <= self.nbits + 64, "the reader is never asked further than two words past the end"
        return (self.big >> pos) & ((1 << n) - 1)

    def byte(self, i):
        assert 0 <= i < self.cnt, "a load outside the chunk's bytes"
        return self.data[i]


def slow_decode(v, count, sym, maxlen):
    """pd_slow_decode: canonical decode one bit at a time; (symbol, bits used) or (-1, 0)."""
    code = first = index = 0
    for ln in range(1, maxlen + 1):
        code |= v & 1
        v >>= 1
        c = count[ln]
        if code - c < first:
            assert 0 <= index + (code - first) < len(sym)
            return sym[index + (code - first)], ln
        index += c
        first += c
        first <<= 1
        code <<= 1
    return -1, 0


def code_check(count, codes):
    """pd_code_check: zlib's inflate_table acceptance."""
    mx = 15
    while mx >= 1 and count[mx] == 0:
        mx -= 1
    if mx == 0:
        return 1 if codes else 0
    left = 1
    for ln in range(1, 16):
        left = (left << 1) - count[ln]
        if left < 0:
            return 1
    return 1 if left > 0 and (codes or mx != 1) else 0


def sorted_symbols(lens):
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    return count, [s for n in range(1, 16) for s, m in enumerate(lens) if m == n]


class Header:
    err = kind = final = data_pos = stored_len = 0
    lcnt = dcnt = lsym = dsym = None


def header(b, pos):
    """pd_header<true>: err 0, 1 (block type), 2 (LEN / NLEN), 3 (code lengths) or 5 (the input ends first)."""
    h = Header()
    if pos + 3 > b.nbits:
        h.err = 5
        return h
    h.final = b.peek(pos, 1)
    h.kind = b.peek(pos + 1, 2)
    pos += 3
    if h.kind == 3:
        h.err = 1
        return h
    if h.kind == 0:
        p = (pos + 7) & ~7
        if p + 32 > b.nbits:
            h.err = 5
            return h
        ln = b.byte(p // 8) | b.byte(p // 8 + 1) << 8
        nln = b.byte(p // 8 + 2) | b.byte(p // 8 + 3) << 8
        if ln != (~nln & 0xFFFF):
            h.err = 2
            return h
        h.data_pos, h.stored_len = p + 32, ln
        if h.data_pos + 8 * ln > b.nbits:
            h.err = 5                                        # the kernel takes the bytes that are there
        return h
    if h.kind == 1:
        lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32
    else:
        nlen, ndist, ncode = b.peek(pos, 5) + 257, b.peek(pos + 5, 5) + 1, b.peek(pos + 10, 4) + 4
        pos += 14
        if pos > b.nbits:
            h.err = 5
            return h
        if nlen > 286 or ndist > 30:
            h.err = 3
            return h
        cl = [0] * 19
        for i in range(ncode):
            cl[CLORDER[i]] = b.peek(pos, 3)
            pos += 3
        if pos > b.nbits:
            h.err = 5
            return h
        clcnt, clsym = sorted_symbols(cl)
        if code_check(clcnt, True):
            h.err = 3
            return h
        tmp, n = [], nlen + ndist
        while len(tmp) < n:
            s, used = slow_decode(b.peek(pos, 7), clcnt, clsym, 7)
            assert s >= 0, "a complete code of at most 7 bits decodes any 7 bits"
            pos += used
            if s < 16:
                ln, rep = s, 1
            elif s == 16:
                ln, rep = (tmp[-1] if tmp else 0), 3 + b.peek(pos, 2)
                pos += 2
            elif s == 17:
                ln, rep = 0, 3 + b.peek(pos, 3)
                pos += 3
            else:
                ln, rep = 0, 11 + b.peek(pos, 7)
                pos += 7
            if pos > b.nbits:
                h.err = 5
                return h
            if (s == 16 and not tmp) or len(tmp) + rep > n:
                h.err = 3
                return h
            tmp += [ln] * rep
            assert len(tmp) <= 316
        lens = (tmp[:nlen] + [0] * 288)[:288] + (tmp[nlen:] + [0] * 32)[:32]
        if lens[256] == 0:
            h.err = 3
            return h
    h.lcnt, h.lsym = sorted_symbols(lens[:288])
    h.dcnt, h.dsym = sorted_symbols(lens[288:])
    if code_check(h.lcnt, False) or code_check(h.dcnt, False):
        h.err = 3
        return h
    h.data_pos = pos
    return h


class Table:
    """pd_fast_tables + pd_symbol: the first-level entry of the low FB bits (formed when first asked for: the same value
    the wave stores), the canonical decode for longer codes."""

    def __init__(self, count, sym):
        self.count, self.sym, self.fast = count, sym, {}

    def symbol(self, b, pos):
        e = b.peek(pos, FB)
        assert 0 <= e < (1 << FB)
        if e not in self.fast:
            s, used = slow_decode(e, self.count, self.sym, FB)
            self.fast[e] = 0 if s < 0 else (s << 4 | used)
        v = self.fast[e]
        if v:
            return v >> 4, v & 15
        return slow_decode(b.peek(pos, 15), self.count, self.sym, 15)


def inflate(stream, want):
    """One chunk: (bytes produced, OK / CORRUPT / PAST) -- produced[k] and bad[k] of the kernel."""
    assert want >= 1
    b = Bits(stream)
    dst = np.zeros(want, dtype=np.uint8)                     # the chunk buffer: `full` >= want bytes in the kernel
    lane_s1, lane_s2 = [0] * WAVE, [0] * WAVE                # per lane: sum x_i, sum i x_i (mod ADLER after every batch)
    op = 0

    def put(lane, i, v):
        v = int(v)
        assert 0 <= i < want, "a store outside the chunk"
        dst[i] = v
        lane_s1[lane] += v
        lane_s2[lane] += i * v
        assert lane_s2[lane] < 1 << 63

    def fold():
        for ln in range(WAVE):
            lane_s1[ln] %= ADLER
            lane_s2[ln] %= ADLER

    def result(status):
        return dst[:op].tobytes(), status

    if b.cnt < 2:
        return result(OK)
    cmf, flg = b.byte(0), b.byte(1)
    if ((cmf << 8) | flg) % 31 or (cmf & 15) != 8 or (cmf >> 4) > 7:
        return result(CORRUPT)
    if flg & 32:
        return result(CORRUPT if b.cnt >= 6 else OK)          # the dictionary id has to be there before zlib asks for one
    pos = 16
    steps = 0
    while True:
        steps += 1
        assert steps <= b.nbits + 2, "every block takes at least three bits"
        h = header(b, pos)
        stored_cut = h.err == 5 and h.kind == 0 and h.data_pos != 0
        if h.err == 5 and not stored_cut:
            return result(OK)
        if h.err and not stored_cut:
            return result(CORRUPT)
        if h.kind == 0:
            there = min(h.stored_len, (b.nbits - h.data_pos) // 8)
            take = min(there, want - op)
            for k in range(take):                            # lane k % 64, one byte each round
                put(k % WAVE, op + k, b.byte(h.data_pos // 8 + k))
            fold()
            op += take
            if there > take:
                return result(PAST)                          # a stored byte that is there and has no room
            if there < h.stored_len:
                return result(OK)
            pos = h.data_pos + 8 * there
        else:
            lt, dt = Table(h.lcnt, h.lsym), Table(h.dcnt, h.dsym)
            pos = h.data_pos
            out = op
            end = None                                       # "eob", "stop", CORRUPT, PAST
            while end is None:
                recs = []                                    # (offset, distance or 0, length or the literal)
                rel = (pos >> 5) << 5                        # the window starts at the word that holds the batch's first bit
                assert rel <= b.nbits
                while len(recs) < BATCH and end is None and pos - rel < (WIN - 64) * 8:
                    assert pos - rel + 48 + 3 * 32 <= WIN * 8, "a record and the reader's words ahead lie inside the window"
                    s, used = lt.symbol(b, pos)
                    if s < 0:
                        end = "stop" if pos + 1 > b.nbits else CORRUPT
                        break
                    pos += used
                    if pos > b.nbits:
                        end = "stop"
                    elif s < 256:
                        if out == want:
                            end = PAST if (pos + 7) // 8 < b.cnt else "stop"
                        else:
                            recs.append((out, 0, s))
                            out += 1
                    elif s == 256:
                        end = "eob"
                    else:
                        ls = s - 257
                        if ls >= 29:
                            end = CORRUPT
                            break
                        ln = LBASE[ls] + b.peek(pos, LEXT[ls])
                        pos += LEXT[ls]
                        if pos > b.nbits:
                            end = "stop"
                            break
                        ds, used = dt.symbol(b, pos)
                        if ds < 0:
                            end = "stop" if pos + 1 > b.nbits else CORRUPT
                            break
                        pos += used
                        if pos > b.nbits:
                            end = "stop"
                            break
                        if ds >= 30:
                            end = CORRUPT
                            break
                        dist = DBASE[ds] + b.peek(pos, DEXT[ds])
                        pos += DEXT[ds]
                        if pos > b.nbits:
                            end = "stop"
                        elif out == want:
                            end = PAST if (pos + 7) // 8 < b.cnt else "stop"
                        elif dist > out:
                            end = CORRUPT
                        elif out + ln > want:
                            recs.append((out, dist, want - out))
                            out = want
                            end = PAST if (pos + 7) // 8 < b.cnt else "stop"
                        else:
                            recs.append((out, dist, ln))
                            out += ln
                assert len(recs) <= BATCH and (recs or end is not None), "a batch moves on in the stream"
                if end == CORRUPT:
                    return result(CORRUPT)
                # the wave: literals of the batch at once, then copy after copy (a barrier in front of each)
                for r, (o, d, v) in enumerate(recs):
                    if d == 0:
                        put(r % WAVE, o, v)
                copies = [r for r, rec in enumerate(recs) if rec[1]]         # Z.cpy: lane 0 lists them as it decodes
                for r in copies:
                    o, d, ln = recs[r]
                    assert 1 <= d <= o and 1 <= ln <= 258
                    for k in range(ln):
                        src = o - d + (k if k < d else k % d)
                        assert 0 <= src < o
                        put(k % WAVE, o + k, dst[src])
                fold()
                op = out
            if end == PAST:
                return result(PAST)
            if end == "stop":
                return result(OK)
        if h.final:
            break
    # the end of the stream: the trailer, when its four bytes are there
    p = (pos + 7) // 8
    if p + 4 <= b.cnt:
        s1, s2, n = sum(lane_s1) % ADLER, sum(lane_s2) % ADLER, op % ADLER
        a = (1 + s1) % ADLER
        bb = (n + n * s1 + ADLER - s2) % ADLER
        stored = b.byte(p) << 24 | b.byte(p + 1) << 16 | b.byte(p + 2) << 8 | b.byte(p + 3)
        if (bb << 16 | a) != stored:
            return result(CORRUPT)
    return result(OK)


def outcome(stream, want):
    """What tiffio._chunk makes of the chunk: ("bytes", data), ("corrupt",), ("past",) or ("short", n, want)."""
    data, status = inflate(stream, want)
    if status == CORRUPT:
        return ("corrupt",)
    if status == PAST:
        return ("past",)
    if len(data) < want:
        return ("short", len(data), want)
    return ("bytes", data)
