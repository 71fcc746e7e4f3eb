"""A Python restatement of the phases of the TIFF encoder's kernels (csrc/tiff_encode.hip), not of lzw_writer's loop: the
bytes of a strip read 64 at a time with the predictor applied on the read, the string table as the 8192-slot open-addressed
hash the kernel keeps in LDS (slot = key << 12 | code, 0 = empty), probe sequences of 64 consecutive slots per step, the code
widths, the bit accumulator and the byte index of every store into the strip's buffer; then the scan of the padded strip
lengths, the directory and the strips' places in the file.  Every index the kernels form is formed here and asserted to be
in range.  tests/test_tiff_encode_cpu.py holds the codes against lzw_writer.encode(data, clear_at=4094), the specification.

The picture is a NumPy array; a strip's bytes are never materialised differenced, as in the kernel."""
import struct

import numpy as np

SLOTS = 8192                 # TE_SLOTS
CLEAR, EOI, FIRST, CLEAR_AT = 256, 257, 258, 4094
SEG_CODES = CLEAR_AT - FIRST  # 3836
LANES = 64
MAX_ENTRIES = 13             # TE_MAX_ENTRIES
DEFAULT_STRIP_BYTES = 65536  # the knob tiff_strip_bytes


def width_of(i):
    return 9 if i <= 253 else 10 if i <= 765 else 11 if i <= 1789 else 12


def hash_of(key):
    return ((key * 2654435761) & 0xFFFFFFFF) >> 19


def strip_cap(n):
    """te_strip_cap: at most n codes that take input, n // 3836 Clears after full segments, the leading Clear and EOI, 12 bits
    each, the last byte filled up, one pad byte to an even length."""
    nbytes = (12 * (n + n // SEG_CODES + 2) + 7) // 8
    return nbytes + (nbytes & 1)


class Geometry:
    """te_geometry."""

    def __init__(self, h, w, channels, itemsize, rows_per_strip=None, predictor=False, strip_bytes=DEFAULT_STRIP_BYTES):
        assert 1 <= h <= 1 << 24 and 1 <= w <= 1 << 24 and 1 <= channels <= 5 and itemsize in (1, 2)
        self.rowb = w * channels * itemsize
        rps = rows_per_strip if rows_per_strip else max(1, strip_bytes // self.rowb)
        self.rps = min(rps, h)
        assert self.rps * self.rowb <= 1 << 30
        self.nstrips = -(-h // self.rps)
        self.pitch = (strip_cap(self.rps * self.rowb) + 3) & ~3
        self.width, self.height, self.spp, self.bps, self.predictor = w, h, channels, itemsize, bool(predictor)

    def strip_bytes(self, k):
        return min(self.rps, self.height - k * self.rps) * self.rowb


def bound(g):
    """te_bound."""
    last = g.strip_bytes(g.nstrips - 1)
    return (8 + (g.nstrips - 1) * strip_cap(g.rps * g.rowb) + strip_cap(last) + 2 + 12 * MAX_ENTRIES + 4 + 4 * g.spp + 8 * g.nstrips)


def file_byte(img8, img16, g, B):
    """te_byte: byte B of the picture as the file stores it.  img8 / img16: the picture's memory as bytes / as uint16."""
    assert 0 <= B < g.height * g.rowb
    if not g.predictor:
        return int(img8[B])
    q = B % g.rowb
    if g.bps == 1:
        left = int(img8[B - g.spp]) if q >= g.spp else 0
        assert q < g.spp or B - g.spp >= 0
        return (int(img8[B]) - left) & 255
    e = B >> 1
    assert 0 <= e < img16.size and g.rowb % 2 == 0
    left = 0
    if (q >> 1) >= g.spp:
        assert e - g.spp >= 0
        left = int(img16[e - g.spp])
    v = (int(img16[e]) - left) & 0xFFFF
    return v >> 8 if q & 1 else v & 255


def new_events():
    """What encode_strip() records for tests that assert coverage: ``clears`` table-full Clears, ``widths`` the code widths
    used, ``max_steps`` the longest probe sequence in steps of 64 slots, ``max_taken`` the most slots taken, ``wrapped`` a probe
    window that wrapped round the table's end; ``match_step`` / ``insert_step`` the deepest step (counted from 0) at which a
    match was found / an empty slot was taken, -1 for never; ``wrapped_late`` a window that wrapped on a step after the first;
    ``wrap_step`` the deepest such step; ``final_clear`` the Clear in front of EndOfInformation that follows a last code which
    is the 3836th of its segment."""
    return dict(clears=0, widths=set(), max_steps=0, max_taken=0, wrapped=False, match_step=-1, insert_step=-1, wrapped_late=False,
                wrap_step=-1, final_clear=False)


def encode_strip(img8, img16, g, k, events=None):
    """k_te_lzw for strip k: (the codes, the strip buffer's bytes up to the stream's length, over)."""
    ev = events if events is not None else new_events()
    assert 0 <= k < g.nstrips
    n = g.strip_bytes(k)
    assert 1 <= n <= 1 << 30
    base = k * g.rps * g.rowb
    cap = g.pitch
    dst = bytearray(cap)
    tab = [0] * SLOTS
    state = dict(acc=0, nbits=0, op=0, i=0, over=False)
    codes = []

    def emit(code):
        assert 0 <= code < 4096
        width = width_of(state["i"])
        assert code < (1 << width), (code, width)
        ev["widths"].add(width)
        codes.append(code)
        state["acc"] = (state["acc"] << width) | code
        state["nbits"] += width
        assert state["nbits"] <= (28 if code == EOI else 19) and state["acc"] < 1 << 32
        while state["nbits"] >= 8:
            state["nbits"] -= 8
            if state["op"] < cap:
                dst[state["op"]] = (state["acc"] >> state["nbits"]) & 255
            else:
                state["over"] = True
            state["op"] += 1
        state["acc"] &= (1 << state["nbits"]) - 1
        state["i"] = 0 if code == CLEAR else state["i"] + 1

    emit(CLEAR)
    nxt, w, taken = FIRST, -1, 0
    for t0 in range(0, n, LANES):
        mine = [file_byte(img8, img16, g, base + t0 + lane) if t0 + lane < n else 0 for lane in range(LANES)]
        cnt = min(LANES, n - t0)
        for u in range(cnt):
            byte = mine[u]
            if w < 0:
                w = byte
                continue
            assert 0 <= w < 4096
            key = (w << 8) | byte
            assert key < 1 << 20
            h0 = hash_of(key)
            assert 0 <= h0 < SLOTS
            found, slot_at = -1, -1
            for step in range(SLOTS // LANES):
                slots = [(h0 + step * LANES + lane) & (SLOTS - 1) for lane in range(LANES)]
                assert all(0 <= q < SLOTS for q in slots)
                if slots[-1] < slots[0]:
                    ev["wrapped"] = True
                    if step >= 1:
                        ev["wrapped_late"] = True
                        ev["wrap_step"] = max(ev["wrap_step"], step)
                hits = [lane for lane in range(LANES) if tab[slots[lane]] == 0 or tab[slots[lane]] >> 12 == key]
                if hits:
                    first = hits[0]
                    vv = tab[slots[first]]
                    if vv:
                        found = vv & 4095
                        assert FIRST <= found < nxt
                        ev["match_step"] = max(ev["match_step"], step)
                    else:
                        slot_at = slots[first]
                        ev["insert_step"] = max(ev["insert_step"], step)
                    ev["max_steps"] = max(ev["max_steps"], step + 1)
                    break
            if found >= 0:
                w = found
                continue
            emit(w)
            assert slot_at >= 0, "the table never holds more than 3836 entries"
            assert tab[slot_at] == 0 and FIRST <= nxt < CLEAR_AT
            tab[slot_at] = (key << 12) | nxt
            assert tab[slot_at] < 1 << 32
            taken += 1
            ev["max_taken"] = max(ev["max_taken"], taken)
            nxt += 1
            if nxt >= CLEAR_AT:
                emit(CLEAR)
                ev["clears"] += 1
                tab = [0] * SLOTS
                nxt, taken = FIRST, 0
            w = byte
    emit(w)
    if nxt + 1 >= CLEAR_AT:                                   # libtiff's LZWPostEncode: the last code counts as an entry
        assert width_of(state["i"]) == 12 and state["nbits"] < 8
        codes.append(CLEAR)                                   # into the accumulator, in front of EndOfInformation: one emit writes both
        state["acc"] = (state["acc"] << 12) | CLEAR
        state["nbits"] += 12
        state["i"] = 0
        ev["clears"] += 1
        ev["final_clear"] = True
    emit(EOI)
    if state["nbits"]:
        if state["op"] < cap:
            dst[state["op"]] = (state["acc"] << (8 - state["nbits"])) & 255
        else:
            state["over"] = True
        state["op"] += 1
    op = state["op"]
    assert not state["over"] and op + (op & 1) <= strip_cap(n) <= cap, (op, n, cap)
    if op & 1:
        assert op < cap
        dst[op] = 0
    return codes, bytes(dst[:op]), state["over"]


def encode_file(array, rows_per_strip=None, predictor=False, strip_bytes=DEFAULT_STRIP_BYTES, out_cap=None):
    """k_te_lzw for every strip, then k_te_frame and k_te_pack: (status, the file's bytes or None, the file's length)."""
    a = np.ascontiguousarray(array)
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    g = Geometry(h, w, c, a.dtype.itemsize, rows_per_strip, predictor, strip_bytes)
    img8 = a.reshape(-1).view(np.uint8)
    img16 = a.reshape(-1) if a.dtype == np.uint16 else None
    streams = [encode_strip(img8, img16, g, k)[1] for k in range(g.nstrips)]
    zlen = [len(s) for s in streams]
    # k_te_frame: the scan of the padded lengths
    off, o = [], 8
    for m in zlen:
        off.append(o)
        o += m + (m & 1)
    n = g.nstrips
    extra = c - 3 if c > 3 else (1 if c == 2 else 0)
    nent = 11 + (1 if g.predictor else 0) + (1 if extra else 0)
    assert nent <= MAX_ENTRIES
    ifd_at = o
    over_at = ifd_at + 2 + 12 * nent + 4
    bits_at = over_at
    offs_at = bits_at + (2 * c if c >= 3 else 0)
    cnts_at = offs_at + (4 * n if n > 1 else 0)
    fmt_at = cnts_at + (4 * n if n > 1 else 0)
    size = fmt_at + (2 * c if c >= 3 else 0)
    assert size <= bound(g), (size, bound(g))
    cap = bound(g) if out_cap is None else out_cap
    if size >= 1 << 32:
        return 2, None, 0
    if size > cap:
        return 1, None, size
    out = bytearray(cap)

    def put(at, fmt, *values):
        raw = struct.pack("<" + fmt, *values)
        assert 0 <= at and at + len(raw) <= size, (at, len(raw), size)
        out[at:at + len(raw)] = raw

    def entry(at, tag, typ, count, value, inline, where):
        put(at, "HHI", tag, typ, count)
        if not inline:
            put(at + 8, "I", where)
        elif typ == 4:
            put(at + 8, "I", value)
        else:
            assert count <= 2
            put(at + 8, "4x")
            put(at + 8, str(count) + "H", *([value] * count))
        return at + 12

    if n > 1:
        for k in range(n):
            put(offs_at + 4 * k, "I", off[k])
            put(cnts_at + 4 * k, "I", zlen[k])
    put(0, "2sHI", b"II", 42, ifd_at)
    put(ifd_at, "H", nent)
    p = ifd_at + 2
    bits = 8 * g.bps
    p = entry(p, 256, 4, 1, w, True, 0)
    p = entry(p, 257, 4, 1, h, True, 0)
    p = entry(p, 258, 3, c, bits, c < 3, bits_at)
    p = entry(p, 259, 3, 1, 5, True, 0)
    p = entry(p, 262, 3, 1, 2 if c >= 3 else 1, True, 0)
    p = entry(p, 273, 4, n, 8, n == 1, offs_at)
    p = entry(p, 277, 3, 1, c, True, 0)
    p = entry(p, 278, 4, 1, g.rps, True, 0)
    p = entry(p, 279, 4, n, zlen[0], n == 1, cnts_at)
    p = entry(p, 284, 3, 1, 1, True, 0)
    if g.predictor:
        p = entry(p, 317, 3, 1, 2, True, 0)
    if extra:
        p = entry(p, 338, 3, extra, 0, True, 0)
    p = entry(p, 339, 3, c, 1, c < 3, fmt_at)
    put(p, "I", 0)
    assert p + 4 == over_at
    if c >= 3:
        for j in range(c):
            put(bits_at + 2 * j, "H", bits)
            put(fmt_at + 2 * j, "H", 1)
    # k_te_pack
    for k in range(n):
        m = zlen[k] + (zlen[k] & 1)
        assert m <= g.pitch and off[k] % 2 == 0 and off[k] + m <= ifd_at
        out[off[k]:off[k] + zlen[k]] = streams[k]
    return 0, bytes(out[:size]), size
