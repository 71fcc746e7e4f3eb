"""The stream the Deflate coder writes with the knob ``deflate_matching`` at 1 (csrc/deflate_lz_device.h), in Python, byte for byte.

Framing as without matching (png_encode_model): segments of 32768 bytes, ``78 01`` in front, an empty stored block behind every
segment but the last, the Adler-32 at the end.  Per segment ``b[0 .. n)``:

* hash(j), j <= n - 4: the four bytes at j, little-endian, times 2654435761 mod 2^32, top 12 bits.
* Positions go in tiles of 256.  head[h] of a tile: the largest position before the tile's first that has hash h.
* Candidates at j <= n - 3, by rising distance: j-1 .. j-4 (where >= 0), then head[hash(j)] of j's tile (where j <= n - 4).
* Match length: the common prefix, at most min(258, n - j).  The longest candidate wins, the nearer one on a tie; it is taken
  from 3 bytes on (the near candidates find 3-byte repeats; the table's candidates share 4 bytes unless the hash collides).
* Greedy parse from 0: a taken match skips its length, else one literal.
* The matched block: dynamic, HLIT 286 and HDIST 30 always, both trees limited to 15 bits by huff_lengths; a distance tree with
  fewer than two used symbols is padded with length-1 codes (none used: symbols 0 and 1; one used: that one and symbol 0, or 1
  where the used one is 0).  The 316 code lengths go through the 16/17/18 run coder as one sequence.
* The matched block is written only where it is shorter than both the literal-only dynamic block and the stored block; otherwise
  the segment is what png_encode_model.body_bytes gives."""
import zlib

import png_encode_model as pm

SEG = pm.SEG
TILE = 256
MIN_MATCH = 3
MAX_MATCH = 258
HASH_BITS = 12
NLL, ND = 286, 30


def hash4(b, j):
    return ((int.from_bytes(b[j:j + 4], "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3 .. 258."""
    assert MIN_MATCH <= length <= MAX_MATCH
    if length == 258:
        return 285, 0, 0
    v = length - 3
    if v < 8:
        return 257 + v, 0, 0
    k = v.bit_length() - 1
    eb = k - 2
    return 261 + 4 * eb + ((v >> eb) & 3), eb, v & ((1 << eb) - 1)


def distance_symbol(dist):
    """(symbol, extra bits, extra value) of a distance 1 .. 32768."""
    assert 1 <= dist <= 32768
    v = dist - 1
    if v < 4:
        return v, 0, 0
    k = v.bit_length() - 1
    eb = k - 1
    return 2 * k + ((v >> eb) & 1), eb, v & ((1 << eb) - 1)


def candidates(b):
    """cand[j], j <= n - 4: head[hash(j)] as j's tile sees it, or None."""
    n = len(b)
    cand = [None] * n
    head = {}
    for t0 in range(0, max(0, n - 3), TILE):
        t1 = min(t0 + TILE, n - 3)
        hs = [hash4(b, j) for j in range(t0, t1)]
        for j, h in zip(range(t0, t1), hs):
            cand[j] = head.get(h)
        for j, h in zip(range(t0, t1), hs):
            head[h] = j                       # rising j: the largest stays
    return cand


def match_length(b, c, j, cap):
    if b[c:c + cap] == b[j:j + cap]:
        return cap
    k = 0
    while b[c + k] == b[j + k]:
        k += 1
    return k


def best_match(b, cand, j):
    """(length, distance) of the chosen candidate at j, (0, 0) where none is taken."""
    n = len(b)
    if j > n - MIN_MATCH:
        return 0, 0
    cap = min(MAX_MATCH, n - j)
    best, dist = 0, 0
    cs = [j - d for d in (1, 2, 3, 4) if j - d >= 0]
    if j <= n - 4 and cand[j] is not None:
        cs.append(cand[j])
    for c in cs:
        assert 0 <= c < j
        k = match_length(b, c, j, cap)
        if k > best:
            best, dist = k, j - c
        if best == cap:
            break
    return (best, dist) if best >= MIN_MATCH else (0, 0)


def parse(b):
    """The greedy parse: [(byte,)] and [(length, distance)] tokens."""
    b = bytes(b)
    cand = candidates(b)
    out, j = [], 0
    while j < len(b):
        length, dist = best_match(b, cand, j)
        if length:
            out.append((length, dist))
            j += length
        else:
            out.append((b[j],))
            j += 1
    assert j == len(b)
    return out


def run_code(lens):
    """png_encode_model.run_code for any number of lengths."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
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
    assert len(out) <= n
    return out


def tree(freq, maxbits=15):
    """Code lengths by symbol for the used symbols of ``freq`` (at least one used)."""
    key, sym = pm.sorted_symbols(freq)
    lengths = pm.huff_lengths(key, maxbits)
    lens = [0] * len(freq)
    for s, v in zip(sym, lengths):
        lens[s] = v
    return lens


def matched_block(tokens, last, record=None):
    """The matched dynamic block of one segment's tokens: (value, bits) LSB first, without the flush that follows it."""
    lhist, dhist = [0] * NLL, [0] * ND
    for t in tokens:
        if len(t) == 1:
            lhist[t[0]] += 1
        else:
            lhist[length_symbol(t[0])[0]] += 1
            dhist[distance_symbol(t[1])[0]] += 1
    lhist[256] = 1
    llens = tree(lhist)
    used = [s for s in range(ND) if dhist[s]]
    if len(used) == 0:
        dlens = [1, 1] + [0] * (ND - 2)
    elif len(used) == 1:
        dlens = [0] * ND
        dlens[used[0]] = 1
        dlens[1 if used[0] == 0 else 0] = 1
    else:
        dlens = tree(dhist)
    ltab, dtab = pm.huff_codes(llens), pm.huff_codes(dlens)
    runs = run_code(llens + dlens)
    cfreq = [0] * 19
    for s, _ in runs:
        cfreq[s] += 1
    clen = tree(cfreq, 7)
    ccode = pm.huff_codes(clen)
    hclen = 19
    while hclen > 4 and clen[pm.ORDER[hclen - 1]] == 0:
        hclen -= 1
    value, pos = 0, 0

    def put(v, nbits):
        nonlocal value, pos
        assert 0 <= v < 1 << nbits
        value |= v << pos
        pos += nbits

    put(1 if last else 0, 1)
    put(2, 2)
    put(NLL - 257, 5)
    put(ND - 1, 5)
    put(hclen - 4, 4)
    for i in range(hclen):
        put(clen[pm.ORDER[i]], 3)
    for s, extra in runs:
        put(ccode[s][1], ccode[s][0])
        if s >= 16:
            put(extra, {16: 2, 17: 3, 18: 7}[s])
    for t in tokens:
        if len(t) == 1:
            put(ltab[t[0]][1], ltab[t[0]][0])
            continue
        start = pos
        ls, leb, lev = length_symbol(t[0])
        ds, deb, dev = distance_symbol(t[1])
        assert ltab[ls][0] and dtab[ds][0]
        put(ltab[ls][1], ltab[ls][0])
        put(lev, leb)
        put(dtab[ds][1], dtab[ds][0])
        put(dev, deb)
        if record is not None:
            record.setdefault("lsyms", set()).add(ls)
            record.setdefault("dsyms", set()).add(ds)
            record["max_token_bits"] = max(record.get("max_token_bits", 0), pos - start)
    put(ltab[256][1], ltab[256][0])
    if record is not None:
        record["max_code_len"] = max(record.get("max_code_len", 0), max(llens), max(dlens))
    return value, pos


def body_bytes(data, last, record=None):
    """The bytes of one segment, zlib header and Adler-32 apart.  ``record``, a dict, collects what the segments used: ``forms``
    (a list of 'matched' / 'literal' / 'stored'), ``lsyms``, ``dsyms``, ``max_token_bits``, ``max_code_len`` (of written matched
    blocks only)."""
    data = bytes(data)
    n = len(data)
    assert 1 <= n <= SEG
    today = pm.body_bytes(data, last)
    rec = {}
    value, pos = matched_block(parse(data), last, rec)
    mbytes = (pos + 7) // 8 if last else (pos + 3 + 7) // 8 + 4
    seg = pm.segment(data, last)
    if not mbytes < min(seg["huff_bytes"], n + 5):
        if record is not None:
            record.setdefault("forms", []).append("stored" if seg["stored"] else "literal")
        return today
    if record is not None:
        record.setdefault("forms", []).append("matched")
        for k in ("lsyms", "dsyms"):
            record.setdefault(k, set()).update(rec.get(k, ()))
        for k in ("max_token_bits", "max_code_len"):
            record[k] = max(record.get(k, 0), rec.get(k, 0))
    out = value.to_bytes((pos + 7) // 8, "little") if last else value.to_bytes((pos + 3 + 7) // 8, "little") + b"\x00\x00\xff\xff"
    assert len(out) == mbytes < len(today)
    return out


def stream(data, record=None):
    """The zlib stream of ``data`` (at least one byte)."""
    data = bytes(data)
    assert data
    out = [b"\x78\x01"]
    for at in range(0, len(data), SEG):
        out.append(body_bytes(data[at:at + SEG], at + SEG >= len(data), record))
    out.append(zlib.adler32(data).to_bytes(4, "big"))
    return b"".join(out)
