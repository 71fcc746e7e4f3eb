"""A Python restatement of lane 0's work in k_png_deflate (csrc/png.hip) for one segment of the filtered stream: the symbol
histogram and its rank sort, huff_lengths with the repair that limits the code lengths, huff_codes, the run-length coding of
the 259 code lengths (symbols 16, 17, 18), the code-length code, the ``hclen`` trim, the header's bits, and the choice between
the dynamic block and the stored form.  Every index the kernel forms on that path is formed here and asserted to be in range.
read_header() is the other direction and shares nothing with it: it reads a dynamic block's header out of a deflate stream,
so that tests can look at the code lengths a device wrote.

The packing of the literals by all threads is not restated: zlib judges it in test_png_cpu.check_png."""
SEG = 32768                      # PNG_SEG
OUT_WORDS = (SEG + 64) // 4      # PNG_OUT_WORDS
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def huff_lengths(key, maxbits, info=None):
    """huff_lengths: ``key`` ascending frequencies; returns the code length of every sorted symbol.  ``info``, a dict, gets
    ``depth`` (the longest minimum-redundancy length, before the limit) and ``repairs`` (rounds of the Kraft loop)."""
    key = list(key)
    n = len(key)
    assert 1 <= n <= 288 and all(0 < k < 1 << 32 for k in key) and key == sorted(key)
    if info is not None:
        info.update(depth=1, repairs=0)
    if n == 1:
        return [1]

    def at(i):
        assert 0 <= i < n, i
        return i

    key[0] += key[at(1)]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or key[at(root)] < key[at(leaf)]:
            key[at(nxt)] = key[at(root)]
            key[at(root)] = nxt
            root += 1
        else:
            key[at(nxt)] = key[at(leaf)]
            leaf += 1
        if leaf >= n or (root < nxt and key[at(root)] < key[at(leaf)]):
            key[at(nxt)] += key[at(root)]
            key[at(root)] = nxt
            root += 1
        else:
            key[at(nxt)] += key[at(leaf)]
            leaf += 1
        assert key[nxt] < 1 << 32
    key[at(n - 2)] = 0
    for nxt in range(n - 3, -1, -1):
        key[at(nxt)] = key[at(key[at(nxt)])] + 1
    avbl, used, dpth = 1, 0, 0
    root, nxt = n - 2, n - 1
    while avbl > 0:
        while root >= 0 and key[at(root)] == dpth:
            used += 1
            root -= 1
        while avbl > used:
            key[at(nxt)] = dpth
            nxt -= 1
            avbl -= 1
        avbl = 2 * used
        dpth += 1
        used = 0
    count = [0] * 33
    for i in range(n):
        count[min(key[i], 32)] += 1
    assert count[32] == 0 or max(key) == 32, "a length above 32 would be counted as 32"
    if info is not None:
        info["depth"] = max(key)
    for i in range(maxbits + 1, 33):
        count[maxbits] += count[i]
        count[i] = 0
    total = 0
    for i in range(maxbits, 0, -1):
        total += count[i] << (maxbits - i)
    assert total < 1 << 32
    while total != 1 << maxbits:
        assert total > 1 << maxbits and count[maxbits] > 0
        count[maxbits] -= 1
        for i in range(maxbits - 1, 0, -1):
            if count[i]:
                count[i] -= 1
                assert i + 1 <= 32
                count[i + 1] += 2
                break
        else:
            raise AssertionError("no shorter code to lengthen")
        total -= 1
        if info is not None:
            info["repairs"] += 1
    j = n
    for length in range(1, maxbits + 1):
        for _ in range(count[length]):
            j -= 1
            key[at(j)] = length
    assert j == 0
    return key


def huff_codes(lens):
    """huff_codes: [(length, bit-reversed canonical code)] of every symbol; lengths at most 15."""
    bl = [0] * 16
    for v in lens:
        assert 0 <= v < 16
        bl[v] += 1
    bl[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for v in lens:
        rev = 0
        if v:
            c = nxt[v]
            nxt[v] += 1
            assert c < 1 << v, "over-subscribed code"
            for i in range(v):
                rev |= ((c >> i) & 1) << (v - 1 - i)
        out.append((v, rev))
    return out


def sorted_symbols(freq):
    """The rank sort: the used symbols by (frequency, symbol)."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    return [f for f, _ in used], [s for _, s in used]


def run_code(lens):
    """The 16 / 17 / 18 coding of lens[0 .. 259): [(symbol, extra)]; at most 260 of them (the kernel's arrays)."""
    assert len(lens) == 259
    out, i = [], 0
    while i < 259:
        v, run = lens[i], 1
        while i + run < 259 and lens[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, 0)] * run
        assert len(out) <= 260, len(out)
    return out


class Bits:
    """put_bits into a buffer of OUT_WORDS words."""

    def __init__(self):
        self.value, self.pos = 0, 0

    def put(self, v, n):
        assert 0 <= n <= 16 and 0 <= v < 1 << n, (v, n)
        assert (self.pos + n + 31) // 32 <= OUT_WORDS and (self.pos >> 5) + (1 if (self.pos & 31) + n > 32 else 0) < OUT_WORDS
        self.value |= v << self.pos
        self.pos += n


def segment(data, last, info=None):
    """Lane 0's work for one segment: a dict with ``lens`` (259 code lengths: 257 literal / end-of-block, two distance codes),
    ``runs`` [(symbol, extra)], ``clen`` (19), ``hclen``, ``header`` (the header's bits as an int, LSB first) and ``hdr_bits``,
    ``huff_bytes``, ``stored`` (the decision) and ``body`` (the segment's bytes without zlib header and Adler-32).  ``info`` gets
    the depths before the limits: ``lit_depth``, ``cl_depth``, ``lit_repairs``, ``cl_repairs``."""
    n = len(data)
    assert 1 <= n <= SEG
    hist = [0] * 288
    for b in data:
        hist[b] += 1
    hist[256] = 1
    key, sym = sorted_symbols(hist[:257])
    nused = len(key)
    assert 2 <= nused <= 257
    li = {}
    lengths = huff_lengths(key, 15, li)
    lens = [0] * 260
    for i in range(nused):
        assert 0 <= sym[i] < 257 and 1 <= lengths[i] <= 15
        lens[sym[i]] = lengths[i]
    table = huff_codes(lens[:257])
    assert sum(2.0 ** -v for v in lens[:257] if v) == 1.0 or nused == 1
    lens[257] = lens[258] = 1
    runs = run_code(lens[:259])
    nr = len(runs)
    cfreq = [0] * 19
    for s, _ in runs:
        assert 0 <= s < 19
        cfreq[s] += 1
    ckey, csym = sorted_symbols(cfreq)          # the insertion sort is stable in the symbol: the same order
    nc = len(ckey)
    assert 2 <= nc <= 19
    ci = {}
    clengths = huff_lengths(ckey, 7, ci)
    clen = [0] * 19
    for i in range(nc):
        assert 1 <= clengths[i] <= 7
        clen[csym[i]] = clengths[i]
    ccode = huff_codes(clen)
    hclen = 19
    while hclen > 4 and clen[ORDER[hclen - 1]] == 0:
        hclen -= 1
    out = Bits()
    out.put(1 if last else 0, 1)
    out.put(2, 2)
    out.put(0, 5)
    out.put(1, 5)
    out.put(hclen - 4, 4)
    for i in range(hclen):
        out.put(clen[ORDER[i]], 3)
    for s, extra in runs:
        length, code = ccode[s]
        assert length > 0
        out.put(code, length)
        if s == 16:
            assert 0 <= extra < 4
            out.put(extra, 2)
        elif s == 17:
            assert 0 <= extra < 8
            out.put(extra, 3)
        elif s == 18:
            assert 0 <= extra < 128
            out.put(extra, 7)
        else:
            assert extra == 0
    data_bits = sum(hist[s] * table[s][0] for s in range(256))
    assert data_bits < 1 << 32
    bits = out.pos + data_bits + table[256][0]
    huff_bytes = (bits + 7) // 8 if last else (bits + 3 + 7) // 8 + 4
    stored = not huff_bytes <= n + 5
    if not stored:
        assert huff_bytes <= 4 * OUT_WORDS          # every bit position of the dynamic block lies within the LDS buffer
    if info is not None:
        info.update(lit_depth=li["depth"], cl_depth=ci["depth"], lit_repairs=li["repairs"], cl_repairs=ci["repairs"], nused=nused, nc=nc,
                    nr=nr)
    return dict(lens=lens[:259], runs=runs, clen=clen, hclen=hclen, header=out.value, hdr_bits=out.pos, huff_bytes=huff_bytes,
                stored=stored, body=n + 5 if stored else huff_bytes, table=table)


def body_bytes(data, last):
    """The bytes k_png_deflate leaves for the segment, zlib header and Adler-32 apart: the dynamic block (and, for a segment that
    is not the last, the empty stored block that brings it to a byte boundary) or the stored form."""
    n = len(data)
    seg = segment(data, last)
    if seg["stored"]:
        return bytes([1 if last else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + bytes(data)
    value, pos = seg["header"], seg["hdr_bits"]
    for b in data:
        length, code = seg["table"][b]
        assert length > 0
        value |= code << pos
        pos += length
    length, code = seg["table"][256]
    value |= code << pos
    pos += length
    if last:
        out = value.to_bytes((pos + 7) // 8, "little")
    else:
        q = (pos + 3 + 7) // 8
        out = value.to_bytes(q, "little") + b"\x00\x00\xff\xff"
    assert len(out) == seg["huff_bytes"]
    return out


def unlimited_depth(freqs):
    """The longest code of a minimum-redundancy code for these frequencies (zeros left out), by the textbook heap."""
    import heapq
    heap = [(f, 0) for f in freqs if f]
    if len(heap) == 1:
        return 1
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


# ---------------------------------------------------------------------------------------------------------------------
# the reader
# ---------------------------------------------------------------------------------------------------------------------
def kraft(lens):
    """Sum of 2^-length over the used symbols, as a fraction of 2^15."""
    return sum(1 << (15 - v) for v in lens if v)


def read_header(stream, bitpos=0):
    """The header of the dynamic block that starts at bit ``bitpos`` of ``stream`` (deflate bit order): a dict with ``final``,
    ``hlit``, ``hdist``, ``hclen``, ``clen`` (19, by symbol), ``runs`` [(symbol, extra)], ``lens`` (hlit + hdist lengths) and
    ``end`` (the bit after the header).  AssertionError where it is not a dynamic block or its code-length code is not a
    complete prefix code."""
    value, nbits = int.from_bytes(stream, "little"), 8 * len(stream)
    pos = bitpos

    def take(n):
        nonlocal pos
        assert pos + n <= nbits, "the header runs past the stream"
        v = (value >> pos) & ((1 << n) - 1)
        pos += n
        return v

    final = take(1)
    assert take(2) == 2, "not a dynamic block"
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    clen = [0] * 19
    for i in range(hclen):
        clen[ORDER[i]] = take(3)
    assert sum(1 << (7 - v) for v in clen if v) == 1 << 7, "the code-length code is not complete"
    # canonical codes, MSB first
    codes, code = {}, 0
    for length in range(1, 8):
        for s in range(19):
            if clen[s] == length:
                codes[(length, code)] = s
                code += 1
        code <<= 1
    lens, runs = [], []
    while len(lens) < hlit + hdist:
        length, code = 0, 0
        while True:
            code = (code << 1) | take(1)
            length += 1
            assert length <= 7, "no code-length code matches"
            if (length, code) in codes:
                break
        s = codes[(length, code)]
        if s < 16:
            runs.append((s, 0))
            lens.append(s)
        elif s == 16:
            extra = take(2)
            assert lens, "a repeat with nothing before it"
            runs.append((16, extra))
            lens += [lens[-1]] * (3 + extra)
        elif s == 17:
            extra = take(3)
            runs.append((17, extra))
            lens += [0] * (3 + extra)
        else:
            extra = take(7)
            runs.append((18, extra))
            lens += [0] * (11 + extra)
    assert len(lens) == hlit + hdist, "a run crosses the end of the lengths"
    return dict(final=final, hlit=hlit, hdist=hdist, hclen=hclen, clen=clen, runs=runs, lens=lens, end=pos)
