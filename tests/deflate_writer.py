"""A deflate / zlib writer under the test's control (standard library only): a bit sink and builders for stored, fixed and
dynamic blocks that write exactly what they are told, valid or not.  tests/png_handmade_cases.py builds its streams with it.

A symbol is ("lit", byte), ("copy", length, distance) or ("copy", length, distance, "284+31") for length 258 written as
code 284 with extra bits 31, ("raw", code, extra value, extra bits) for any literal/length code, ("rawdist", code, extra
value, extra bits) for any distance code (286/287 and 30/31 exist only in the fixed code)."""
import heapq
import struct
import zlib

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


class BitSink:
    """Bits in deflate's order: values LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.cnt = 0

    @property
    def nbits(self):
        return len(self.out) * 8 + self.cnt

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0 and v == 0, (v, n)
        self.acc |= v << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.cnt -= 8

    def code(self, c, n):
        r = 0
        for i in range(n):
            r |= ((c >> i) & 1) << (n - 1 - i)
        self.put(r, n)

    def align(self, pad=0):
        """Up to the next byte with the low bits of ``pad``."""
        n = -self.cnt % 8
        self.put(pad & ((1 << n) - 1), n)

    def raw(self, data):
        assert self.cnt == 0
        self.out += data

    def getvalue(self, pad=0):
        self.align(pad)
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} as inflate assigns them; an over-subscribed set keeps the low bits of each code."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def limited_lengths(freqs, maxlen):
    """Huffman code lengths for the symbols with freq > 0, none longer than maxlen, complete (one symbol: length 1)."""
    used = [s for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    assert 2 <= len(used) <= (1 << maxlen)
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    depth = dict.fromkeys(used, 0)
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    count = [0] * (max(max(depth.values()), maxlen) + 1)
    for d in depth.values():
        count[min(d, maxlen)] += 1
    total = sum(c << (maxlen - n) for n, c in enumerate(count[:maxlen + 1]) if n)
    while total > (1 << maxlen):                              # shorten the budget: one code of maxlen less, one shorter code split
        count[maxlen] -= 1
        for b in range(maxlen - 1, 0, -1):
            if count[b]:
                count[b] -= 1
                count[b + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda s: (-freqs[s], s))
    i = 0
    for n in range(1, maxlen + 1):
        for _ in range(count[n]):
            lens[order[i]] = n
            i += 1
    assert i == len(used)
    return lens


def skewed(freqs, maxlen):
    """The same symbols with frequencies that force a longest code of exactly maxlen under limited_lengths."""
    used = sorted((s for s, f in enumerate(freqs) if f > 0), key=lambda s: (freqs[s], s))
    assert len(used) > maxlen, "too few symbols for a code of that length"
    out = [f * (1 << (maxlen + 2)) if f else 0 for f in freqs]
    for k, s in enumerate(used[:maxlen + 1]):
        out[s] = 1 << max(k - 1, 0)
    return out


def length_symbol(length, alt258=False):
    if length == 258 and alt258:
        return 284, 31, 5
    for c in range(28, -1, -1):
        if LBASE[c] <= length:
            assert length - LBASE[c] < (1 << LEXT[c]) or LEXT[c] == 0 and length == LBASE[c]
            return 257 + c, length - LBASE[c], LEXT[c]
    raise ValueError(length)


def distance_symbol(dist):
    for c in range(29, -1, -1):
        if DBASE[c] <= dist:
            assert dist - DBASE[c] < (1 << DEXT[c])
            return c, dist - DBASE[c], DEXT[c]
    raise ValueError(dist)


def tokens(symbols):
    """[(alphabet 'l' or 'd', code, extra value, extra bits)] of a symbol list."""
    out = []
    for s in symbols:
        if s[0] == "lit":
            out.append(("l", s[1], 0, 0))
        elif s[0] == "copy":
            out.append(("l",) + length_symbol(s[1], len(s) > 3 and s[3] == "284+31"))
            out.append(("d",) + distance_symbol(s[2]))
        elif s[0] == "raw":
            out.append(("l", s[1], s[2], s[3]))
        elif s[0] == "rawdist":
            out.append(("d", s[1], s[2], s[3]))
        else:
            raise ValueError(s)
    return out


def plaintext(symbols, before=b""):
    """What a valid symbol list decodes to, after ``before``."""
    out = bytearray(before)
    for s in symbols:
        if s[0] == "lit":
            out.append(s[1])
        else:
            assert s[0] == "copy" and 1 <= s[2] <= len(out), s
            for _ in range(s[1]):
                out.append(out[-s[2]])
    return bytes(out[len(before):])


def put_tokens(sink, toks, ll, dd, eob):
    for alpha, code, ev, eb in toks:
        c, n = (ll if alpha == "l" else dd)[code]
        sink.code(c, n)
        sink.put(ev, eb)
    if eob:
        sink.code(*ll[256])


def stored_block(sink, data, final=False, pad=0, nlen=None):
    """A stored block of 0..65535 bytes; ``pad``: the bits up to the byte boundary; ``nlen``: instead of the complement."""
    assert len(data) <= 65535
    sink.put(int(final), 1)
    sink.put(0, 2)
    sink.align(pad)
    sink.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen))
    sink.raw(data)


def fixed_block(sink, symbols, final=False, eob=True):
    sink.put(int(final), 1)
    sink.put(1, 2)
    put_tokens(sink, tokens(symbols), canonical(FIXED_LL), canonical(FIXED_D), eob)


def run_length(lengths, use=(16, 17, 18)):
    """zlib-like greedy run-length coding of a code-length list into (symbol, extra value) pairs, with the repeats in ``use``."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, run = lengths[i], 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        if v == 0 and run >= 11 and 18 in use:
            r = min(run, 138)
            out.append((18, r - 11))
        elif v == 0 and run >= 3 and 17 in use:
            r = min(run, 10)
            out.append((17, r - 3))
        elif v and run >= 4 and 16 in use:
            r = min(run - 1, 6)
            out.append((v, 0))
            out.append((16, r - 3))
            r += 1
        else:
            r = 1
            out.append((v, 0))
        i += r
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_block(sink, symbols, final=False, ll_lens=None, d_lens=None, maxlen=15, d_maxlen=15, skew=False, d_skew=False,
                  cl_syms=None, cl_lens=None, hclen=None, hlit=None, hdist=None, trim=True, use=(16, 17, 18), eob=True):
    """A dynamic block.  Code lengths: given (ll_lens, d_lens: lists from symbol 0) or optimal for the symbols with the given
    maximum (skew: frequencies bent so that the longest code has exactly that length).  trim False or hlit / hdist: how many
    lengths are sent.  cl_syms: the run-length coded list itself, [(0..18, extra value)]; cl_lens: the 19 code-length code
    lengths; hclen: how many of them are sent, less 4.  Nothing is checked: an invalid block is written as asked."""
    toks = tokens(symbols)
    if ll_lens is None:
        f = [0] * 286
        f[256] = 1
        for a, c, _, _ in toks:
            if a == "l":
                f[c] += 1
        ll_lens = limited_lengths(skewed(f, maxlen) if skew else f, maxlen)
    if d_lens is None:
        f = [0] * 30
        for a, c, _, _ in toks:
            if a == "d":
                f[c] += 1
        d_lens = limited_lengths(skewed(f, d_maxlen) if d_skew else f, d_maxlen) if any(f) else [0] * 30
    ll_lens, d_lens = list(ll_lens), list(d_lens)
    if hlit is None:
        n = len(ll_lens)
        while trim and n > 257 and ll_lens[n - 1] == 0:
            n -= 1
        hlit = max(n, 257) - 257
    if hdist is None:
        n = len(d_lens)
        while trim and n > 1 and d_lens[n - 1] == 0:
            n -= 1
        hdist = max(n, 1) - 1
    ll_sent = (ll_lens + [0] * 288)[:hlit + 257]
    d_sent = (d_lens + [0] * 32)[:hdist + 1]
    if cl_syms is None:
        cl_syms = run_length(ll_sent + d_sent, use)
    if cl_lens is None:
        f = [0] * 19
        for s, _ in cl_syms:
            f[s] += 1
        if sum(1 for x in f if x) == 1:                       # a complete code needs two codes
            f[0 if f[0] == 0 else 1] += 1
        cl_lens = limited_lengths(f, 7)
    if hclen is None:
        n = 19
        while n > 4 and cl_lens[CLORDER[n - 1]] == 0:
            n -= 1
        hclen = n - 4
    sink.put(int(final), 1)
    sink.put(2, 2)
    sink.put(hlit, 5)
    sink.put(hdist, 5)
    sink.put(hclen, 4)
    for i in range(hclen + 4):
        sink.put(cl_lens[CLORDER[i]], 3)
    cl = canonical(cl_lens)
    for s, ev in cl_syms:
        sink.code(*cl[s])
        sink.put(ev, CL_EXTRA.get(s, 0))
    ll, dd = canonical(ll_sent + [0] * (288 - len(ll_sent))), canonical(d_sent + [0] * (32 - len(d_sent)))
    put_tokens(sink, toks, ll, dd, eob)


def zlib_stream(body, plain=b"", header=b"\x78\x01", adler="ok", trailing=b""):
    """header + deflate body + Adler-32 of ``plain``: "ok", "wrong", or an int 1..4: that many bytes cut off its end."""
    a = struct.pack(">I", zlib.adler32(plain))
    if adler == "wrong":
        a = bytes([a[0], a[1], a[2], a[3] ^ 1])
    elif adler != "ok":
        a = a[:4 - int(adler)]
    return header + body + a + trailing
