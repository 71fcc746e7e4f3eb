"""A code-level writer of TIFF LZW streams for the decode_tiff tests (tiff_handmade_cases.py): it emits exactly the codes it
is told to, at the widths a TIFF decoder reads them.  pack / unpack move codes to bytes and back; encode() is a greedy encoder
with a chosen Clear policy (never, at a fill level, early, some codes after the table froze); Writer keeps a segment's state
so that a stream can be put together code by code -- literals, any entry the table holds, the fill-level code (KwKwK), codes
above the table, Clear and EOI wherever wanted -- and random() walks it through streams that are valid but not greedy;
plaintext() is a plain string-table decoder that shares nothing with tiff_lzw_model.py or with the host decoder.

Within a segment (the codes between two Clears) code i is 9 bits wide for i <= 253, 10 for i <= 765, 11 for i <= 1789 and 12
after that; reading code i >= 1 adds entry 258 + (i - 1) until entry 4095 exists (i = 3838), then the table is frozen."""
CLEAR, EOI, FIRST, MAXCODES = 256, 257, 258, 4096
LAST_J = MAXCODES - 1 - FIRST           # 3837: the index of entry 4095


def width_of(i):
    """The width of code i of a segment."""
    return 9 if i <= 253 else 10 if i <= 765 else 11 if i <= 1789 else 12


def unpack(stream):
    """The codes of a stream, up to and including EOI, at the widths the decoder reads them."""
    codes, at, i, nbits = [], 0, 0, len(stream) * 8
    value = int.from_bytes(stream, "big")
    while True:
        w = width_of(i)
        if at + w > nbits:
            return codes
        code = (value >> (nbits - at - w)) & ((1 << w) - 1)
        at += w
        codes.append(code)
        if code == EOI:
            return codes
        i = 0 if code == CLEAR else i + 1


def pack(codes):
    """Codes -> bytes at the decoder's widths (a code too wide for its slot loses its high bits, as a damaged file's would)."""
    out, acc, nbits, i = bytearray(), 0, 0, 0
    for code in codes:
        w = width_of(i)
        acc = (acc << w) | (code & ((1 << w) - 1))
        nbits += w
        while nbits >= 8:
            nbits -= 8
            out.append((acc >> nbits) & 0xFF)
        acc &= (1 << nbits) - 1
        i = 0 if code == CLEAR else i + 1
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


def bit_length(codes):
    """Bits the codes take."""
    n, i = 0, 0
    for code in codes:
        n += width_of(i)
        i = 0 if code == CLEAR else i + 1
    return n


def plaintext(codes):
    """What the codes decode to, by the textbook string table; AssertionError on a code the table does not hold.  Codes after
    EOI are not looked at."""
    table, prev, out = [bytes([b]) for b in range(256)] + [b"", b""], None, bytearray()
    for code in codes:
        if code == EOI:
            break
        if code == CLEAR:
            del table[FIRST:]
            prev = None
            continue
        if prev is None:
            assert code < 256, f"code {code} after Clear"
            s = table[code]
        elif code < len(table):
            s = table[code]
        else:
            assert code == len(table) < MAXCODES, f"code {code}, table holds {len(table)}"
            s = prev + prev[:1]
        if prev is not None and len(table) < MAXCODES:
            table.append(prev + s[:1])
        out += s
        prev = s
    return bytes(out)


def encode(data, clear_at=None, frozen_run=0, leading_clear=True, eoi=True):
    """The codes of a greedy encoder.  ``clear_at``: send Clear once the encoder's table holds that many codes (259 .. 4096; 4094
    is what libtiff does, and as libtiff does a Clear then also follows a last code that would have brought the table to 4094; small
    values clear early); None: never, the table freezes at 4096 and the frozen table goes on
    being used.  ``frozen_run``: with clear_at 4096, that many more codes are sent from the frozen table before the Clear (a
    deferred clear)."""
    assert clear_at is None or FIRST < clear_at <= MAXCODES
    codes = [CLEAR] if leading_clear else []
    table, frozen, w = {bytes([b]): b for b in range(256)}, 0, b""
    nxt = FIRST
    for byte in data:
        wc = w + bytes([byte])
        if wc in table:
            w = wc
            continue
        codes.append(table[w])
        if nxt < MAXCODES:
            table[wc] = nxt
            nxt += 1
        else:
            frozen += 1
        if clear_at is not None and nxt >= clear_at and frozen >= (frozen_run if clear_at == MAXCODES else 0):
            codes.append(CLEAR)
            table, frozen, nxt = {bytes([b]): b for b in range(256)}, 0, FIRST
        w = bytes([byte])
    if w:
        codes.append(table[w])
        if clear_at == 4094 and nxt + 1 >= clear_at:        # libtiff's LZWPostEncode counts the last code as an entry and clears a full table
            codes.append(CLEAR)
    if eoi:
        codes.append(EOI)
    return codes


class Writer:
    """A stream under construction.  ``i`` is the index the next code gets in its segment, ``lengths[k]`` the bytes code k of
    the segment gives, ``n`` the bytes of the whole stream so far.  Entry j (code 258 + j) is held for j <= i - 2 and is the
    fill-level code, valid too, for j = i - 1; both only up to j = 3837."""

    def __init__(self, leading_clear=True):
        self.codes, self.i, self.lengths, self.n = [], 0, [], 0
        if leading_clear:
            self.clear()

    def held(self):
        """Entries the table holds before the next code is read: j < held()."""
        return min(max(self.i - 1, 0), LAST_J + 1)

    def fill_j(self):
        """The j of the fill-level code, or None where there is none (a first code, a frozen table)."""
        return self.i - 1 if 1 <= self.i <= LAST_J + 1 else None

    def put(self, code):
        """Any code, valid or not; lengths are kept only for valid ones."""
        self.codes.append(code)
        if code == CLEAR:
            self.i, self.lengths = 0, []
        elif code != EOI:
            j = code - FIRST
            length = 1 if code < 256 else self.lengths[j] + 1 if 0 <= j < len(self.lengths) else 0
            self.lengths.append(length)
            self.n += length
            self.i += 1
        return self

    def lit(self, *values):
        for b in values:
            assert 0 <= b < 256
            self.put(b)
        return self

    def entry(self, j):
        assert 0 <= j < self.held() or j == self.fill_j(), (j, self.i)
        return self.put(FIRST + j)

    def fill(self):
        assert self.fill_j() is not None
        return self.put(FIRST + self.fill_j())

    def clear(self):
        return self.put(CLEAR)

    def eoi(self):
        return self.put(EOI)

    def random(self, rng, count, clears=(), p_clear=0.0, literals=256):
        """``count`` more codes, each drawn uniformly from everything valid at its position (literals below ``literals``, any
        held entry, the fill-level code); a Clear goes in front of the codes whose number, counted from 0 here, is in
        ``clears``, and in front of any code with probability ``p_clear``."""
        clears = set(clears)
        draws = rng.random((count, 2))
        for k in range(count):
            if k in clears or draws[k, 0] < p_clear:
                self.clear()
            nent = 0 if self.i == 0 else self.held() + (self.fill_j() is not None)
            pick = min(int(draws[k, 1] * (literals + nent)), literals + nent - 1)
            if pick < literals:
                self.put(pick)
            elif pick - literals < self.held():
                self.put(FIRST + pick - literals)
            else:
                self.fill()
        return self

    def stream(self):
        return pack(self.codes)

    def plain(self):
        return plaintext(self.codes)
