"""Baseline JPEG writer from quantised coefficients (helper, not collected): the mirror of ``jpeg_model.decode``.

Written from the JPEG standard (ITU-T T.81): marker segments of annex B, the Huffman procedures of annexes C, F and K.2.
``write()`` takes the frame, the tables and the coefficients as the decoder will see them and has a knob for everything the
host parser accepts: 16-bit DQT, SOF0 / SOF1, JFIF / Adobe / no header, any component and table ids, tables joined or one
segment each, tables defined twice, DRI twice, fill ``FF``s before markers, extra segments, bytes after EOI.  The ``damage``
knobs make entropy data that is wrong in one chosen way.  Nothing here is fast; the files the tests make are small or sparse.
"""
import struct

import numpy as np

from jpeg_model import ZIGZAG

SAMPLING = {"L": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}


# ---------------------------------------------------------------------------------------------------------------------
# Huffman tables: (counts[16], values)
# ---------------------------------------------------------------------------------------------------------------------
def huff_from_freq(freq):
    """Annex K.2: code lengths from symbol frequencies ({symbol: count}), limited to 16 bits, the all-ones code reserved."""
    f = [0] * 257
    for s, n in freq.items():
        f[s] = max(int(n), 1)
    f[256] = 1                                              # the reserved code point: takes the all-ones code, then leaves
    size, others = [0] * 257, [-1] * 257
    while True:
        live = [i for i in range(257) if f[i]]
        if len(live) < 2:
            break
        v1 = min(live, key=lambda i: (f[i], -i))            # least frequency, the largest symbol on a tie
        v2 = min((i for i in live if i != v1), key=lambda i: (f[i], -i))
        f[v1] += f[v2]
        f[v2] = 0
        size[v1] += 1                                       # every symbol of both subtrees gets one bit longer
        while others[v1] != -1:
            v1 = others[v1]
            size[v1] += 1
        others[v1] = v2                                     # and v2's chain goes behind v1's
        size[v2] += 1
        while others[v2] != -1:
            v2 = others[v2]
            size[v2] += 1
    bits = [0] * (max(size) + 2)
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    bits += [0] * max(0, 18 - len(bits))
    i = len(bits) - 1
    while i > 16:                                           # figure K.3: move pairs of the longest codes up
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                            # the reserved code point
    values = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    counts = bits[1:17]
    assert sum(counts) == len(values)
    return counts, values


def huff_codes(table):
    """{symbol: (code, length)} of a table, the canonical assignment of annex C."""
    counts, values = table
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[values[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def by_use(symbols, freq=None):
    """The symbols, most frequent first (ties by value): the deliberate shapes give their shortest codes to the first."""
    freq = freq or {}
    return sorted(set(symbols), key=lambda s: (-freq.get(s, 0), s))


def shape_long(symbols):
    """One code of 1 bit, one of 2 bits, every other code 16 bits long."""
    assert 1 <= len(symbols) <= 2 + 16383
    counts = [0] * 16
    counts[0] = 1
    if len(symbols) > 1:
        counts[1] = 1
    counts[15] = max(0, len(symbols) - 2)
    return counts, list(symbols)


def shape_all_16(symbols):
    """Every code 16 bits long: nothing is found in a short look-up table."""
    counts = [0] * 16
    counts[15] = len(symbols)
    return counts, list(symbols)


def shape_single(symbol):
    """One code, the single bit 0."""
    return [1] + [0] * 15, [symbol]


def shape_255x8(symbols):
    """Up to 255 codes of 8 bits; 11111111 stays free."""
    assert len(symbols) <= 255
    counts = [0] * 16
    counts[7] = len(symbols)
    return counts, list(symbols)


def shape_256(symbols=None):
    """All 256 values: 255 codes of 8 bits and one of 9; the listed symbols first."""
    first = list(symbols or [])
    values = first + [s for s in range(256) if s not in set(first)]
    counts = [0] * 16
    counts[7], counts[8] = 255, 1
    return counts, values


def shape_staircase(symbols):
    """One code of every length 1 ... 8 (0, 10, 110, ...), the rest at 16 bits behind the prefix 11111111."""
    assert len(symbols) <= 8 + 255
    counts = [0] * 16
    n = len(symbols)
    for ln in range(8):
        if n > 0:
            counts[ln] = 1
            n -= 1
    counts[15] = n
    return counts, list(symbols)


# ---------------------------------------------------------------------------------------------------------------------
# entropy coding
# ---------------------------------------------------------------------------------------------------------------------
def category(v):
    return int(abs(int(v))).bit_length()


def block_symbols(dc_diff, block):
    """One block as [(symbol, extra-bit value, extra-bit count)]: the DC difference, then the AC coefficients in zigzag order."""
    s = category(dc_diff)
    out = [(s, dc_diff if dc_diff >= 0 else dc_diff + (1 << s) - 1, s)]
    run = 0
    zz = [int(block[ZIGZAG[k]]) for k in range(1, 64)]
    last = max((k for k in range(63) if zz[k]), default=-1)
    for k in range(last + 1):
        v = zz[k]
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((0xF0, 0, 0))
            run -= 16
        s = category(v)
        out.append((run << 4 | s, v if v >= 0 else v + (1 << s) - 1, s))
        run = 0
    if last < 62:
        out.append((0x00, 0, 0))
    return out


def symbols_used(coefs, layout, per):
    """Symbol frequencies per component of the scan: ([dc freq], [ac freq]) -- what a table for this file has to hold."""
    ncomp = max(layout) + 1
    dc, ac = [dict() for _ in range(ncomp)], [dict() for _ in range(ncomp)]
    pred = [0] * ncomp
    bpm = len(layout)
    for i, blk in enumerate(coefs):
        if per and i % (per * bpm) == 0:
            pred = [0] * ncomp
        c = layout[i % bpm]
        syms = block_symbols(int(blk[0]) - pred[c], blk)
        pred[c] = int(blk[0])
        dc[c][syms[0][0]] = dc[c].get(syms[0][0], 0) + 1
        for s, _v, _n in syms[1:]:
            ac[c][s] = ac[c].get(s, 0) + 1
    return dc, ac


class Bits:
    def __init__(self):
        self.acc, self.n, self.whole = 0, 0, bytearray()

    def put(self, value, nbits):
        self.acc = self.acc << nbits | (value & ((1 << nbits) - 1))
        self.n += nbits
        if self.n >= 1024:                                  # whole bytes leave the accumulator: it stays short
            r = self.n % 8
            self.whole += (self.acc >> r).to_bytes(self.n // 8, "big")
            self.acc &= (1 << r) - 1
            self.n = r

    def done(self, cut=0):
        """The bytes, the last one padded with 1 bits; ``cut`` bits are taken off the end first."""
        acc, n = (int.from_bytes(self.whole, "big") << self.n | self.acc) >> cut, len(self.whole) * 8 + self.n - cut
        pad = -n % 8
        acc = acc << pad | ((1 << pad) - 1)
        return acc.to_bytes((n + pad) // 8, "big")


def stuff(data):
    return data.replace(b"\xff", b"\xff\x00")


# ---------------------------------------------------------------------------------------------------------------------
# the file
# ---------------------------------------------------------------------------------------------------------------------
def geometry(w, h, sampling):
    """(MCUs across, MCUs down, component of each block of an MCU)."""
    if sampling is None:
        return -(-w // 8), -(-h // 8), [0]
    hs, vs = sampling
    return -(-w // (8 * hs)), -(-h // (8 * vs)), [0] * (hs * vs) + [1, 2]


def segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


def dqt_body(tq, table, pq):
    zz = [int(table[ZIGZAG[k]]) for k in range(64)]
    return bytes([pq << 4 | tq]) + (struct.pack(">64H", *zz) if pq else bytes(zz))


def dht_body(tc, th, table):
    counts, values = table
    return bytes([tc << 4 | th]) + bytes(counts) + bytes(values)


def write(w, h, sampling, coefs, qts, hts, *, tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1), ids=(1, 2, 3), ri=0, sof=0xC0, header="jfif",
          pq=0, split=False, redefine=False, dri_twice=False, fill=0, fill_rst=None, extras=False, trailer=b"",
          inject=None, skip=(), repeat=(), cut=None):
    """A baseline JPEG file.

    sampling   None (one component) or Y's (h, v); coefs [block in scan order][64], natural order, DC as the value itself
    qts        {id: [64] natural order}; hts {(class, id): (counts, values)}; tq / td / ta: the ids each component uses
    pq         1: 16-bit DQT entries (for every table, or a set of ids);  sof 0xC0 / 0xC1;  header "jfif", "adobe", None
    split      one DQT / DHT segment per table instead of one for all;  redefine: every table once wrong, then right
    fill       FFs in front of every marker of the header and EOI;  fill_rst: in front of every RSTn (default: fill)
    extras     a COM or APPn segment between every pair of segments;  trailer: bytes after EOI
    inject     {block: [(value, nbits), ...]} raw bits after that block;  skip / repeat: blocks left out / coded twice;
    cut        {interval: bits} taken off the end of that interval before its padding
    """
    mcux, mcuy, layout = geometry(w, h, sampling)
    ncomp = max(layout) + 1
    bpm, nmcu = len(layout), mcux * mcuy
    coefs = np.asarray(coefs)
    assert coefs.shape == (nmcu * bpm, 64), (coefs.shape, nmcu * bpm)
    per = ri if 0 < ri < nmcu else nmcu
    dc_codes = [huff_codes(hts[(0, td[c])]) for c in range(ncomp)]
    ac_codes = [huff_codes(hts[(1, ta[c])]) for c in range(ncomp)]
    inject, cut = inject or {}, cut or {}
    intervals = []
    for first in range(0, nmcu, per):
        bw, pred = Bits(), [0] * ncomp
        for i in range(first * bpm, min(first + per, nmcu) * bpm):
            c = layout[i % bpm]
            syms = block_symbols(int(coefs[i][0]) - pred[c], coefs[i])
            pred[c] = int(coefs[i][0])
            for _ in range(0 if i in skip else 2 if i in repeat else 1):
                for k, (s, v, n) in enumerate(syms):
                    bw.put(*(dc_codes if k == 0 else ac_codes)[c][s])
                    bw.put(v, n)
                if i in repeat:
                    syms[0] = (0, 0, 0)                      # the copy repeats the picture: a DC difference of 0
            for v, n in inject.get(i, ()):
                bw.put(v, n)
        intervals.append(stuff(bw.done(cut.get(len(intervals), 0))))

    ff = b"\xff" * fill
    n_extra = [0]

    def extra():
        if not extras:
            return b""
        n_extra[0] += 1
        k = n_extra[0]
        return segment(0xFE, b"comment %d \xff\xd9 \xff\x00" % k) if k % 2 else segment(0xE1 + k % 14, bytes(range(k % 40)))

    out = bytearray(b"\xff\xd8")

    def add(marker, body):
        out.extend(extra() + ff + segment(marker, body))

    if header == "jfif":
        add(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0")
    elif header == "adobe":
        add(0xEE, b"Adobe\0\x64\0\0\0\0\1")                 # transform 1: YCbCr
    pq_of = (lambda t: int(t in pq)) if isinstance(pq, (set, frozenset, tuple, list)) else (lambda t: int(pq))
    used_q = sorted(set(tq[:ncomp]))
    used_h = sorted({(0, td[c]) for c in range(ncomp)} | {(1, ta[c]) for c in range(ncomp)})
    if redefine:                                            # wrong tables first: the later definition has to win
        wrong_q = b"".join(dqt_body(t, [(int(x) * 3 + 1) % 256 or 1 for x in qts[t]], 0) for t in used_q)
        add(0xDB, wrong_q)
        add(0xC4, b"".join(dht_body(tc, th, shape_255x8(list(range(12 if tc == 0 else 200)))) for tc, th in used_h))
    if split:
        for t in used_q:
            add(0xDB, dqt_body(t, qts[t], pq_of(t)))
    else:
        add(0xDB, b"".join(dqt_body(t, qts[t], pq_of(t)) for t in used_q))
    if dri_twice:
        add(0xDD, struct.pack(">H", (ri + 5) % 65536))
    frame = struct.pack(">BHHB", 8, h, w, ncomp)
    for c in range(ncomp):
        hs, vs = (sampling if c == 0 and sampling else (1, 1))
        frame += bytes([ids[c], hs << 4 | vs, tq[c]])
    add(sof, frame)
    if split:
        for tc, th in used_h:
            add(0xC4, dht_body(tc, th, hts[(tc, th)]))
    else:
        add(0xC4, b"".join(dht_body(tc, th, hts[(tc, th)]) for tc, th in used_h))
    if ri or dri_twice:
        add(0xDD, struct.pack(">H", ri))
    sos = bytes([ncomp]) + b"".join(bytes([ids[c], td[c] << 4 | ta[c]]) for c in range(ncomp)) + b"\0\x3f\0"
    add(0xDA, sos)
    frst = b"\xff" * (fill if fill_rst is None else fill_rst)
    for k, data in enumerate(intervals):
        if k:
            out.extend(frst + bytes([0xFF, 0xD0 + (k - 1) % 8]))
        out.extend(data)
    out.extend(ff + b"\xff\xd9" + trailer)
    return bytes(out)


def tables_for(coefs, sampling, ri, w, h, td=(0, 1, 1), ta=(0, 1, 1), dc_shape=None, ac_shape=None):
    """Huffman tables that hold every symbol the coefficients need: from the file's own statistics (annex K.2), or of a
    deliberate shape (a function of the symbol list, most used first).  Components sharing an id share the statistics."""
    mcux, mcuy, layout = geometry(w, h, sampling)
    nmcu = mcux * mcuy
    dc, ac = symbols_used(coefs, layout, ri if 0 < ri < nmcu else nmcu)
    hts = {}
    for cls, freqs, ids, shape in ((0, dc, td, dc_shape), (1, ac, ta, ac_shape)):
        for th in sorted(set(ids[:len(freqs)])):
            f = {}
            for c in range(len(freqs)):
                if ids[c] == th:
                    for s, n in freqs[c].items():
                        f[s] = f.get(s, 0) + n
            if not f:
                f = {0: 1}
            hts[(cls, th)] = shape(by_use(f, f)) if shape else huff_from_freq(f)
    return hts
