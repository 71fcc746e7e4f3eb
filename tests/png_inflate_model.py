"""A Python restatement of the inflate phases of csrc/png_decode.hip, not of an inflate loop: pd_plan's sizes, k_pd_mark's
candidate test at every bit offset (pre-filter and full test), the compacted and capped candidate list, pass A's counting
decode with its 256-symbol check cadence and its checkpoints, the walker's binary search, hit or self-decode choice and
segment list, pass B's batches of literal / copy records, the pointer-jumping rounds as the host bounds them, and the
resolve step with the Adler-32 from per-workgroup partial sums.  BitReader is the kernel's reader, quads and all.  Every
index the kernel forms from stream bytes is formed here too and asserted to be in range against the size the plan gave the
array, every loop bounded by stream bytes is asserted to make progress, and every output byte is asserted to be written by
exactly one segment; so a hostile stream is seen by these assertions on the CPU before it reaches a GPU.
tests/test_png_handmade_cpu.py holds the model against zlib."""
import numpy as np

PD_FB = 10
PD_BATCH = 256
PD_CAP_SYMBOLS = 1 << 17
PD_CK = 4096
PD_CKMAX = PD_CAP_SYMBOLS // PD_CK
PD_MARK_THREADS = 256
PD_RESOLVE_BYTES = 64
PD_ADLER_MOD = 65521
NOLIMIT = 0xFFFFFFFF
M64 = (1 << 64) - 1

OK, CRC, ZLIB_HEADER, DEFLATE, FAR, SHORT, ADLER, FILTER, INTERNAL = range(9)     # LARS_PNGD_*

C_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
C_LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
C_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
           8193, 12289, 16385, 24577)
C_DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
C_CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Plan:
    """pd_plan's sizes for a picture of ``need`` filtered bytes (h rows of 1 + rb) and a stream of idat_bytes."""

    def __init__(self, idat_bytes, h, rb):
        self.need = h * (1 + rb)
        self.h, self.rb = h, rb
        self.nbits = idat_bytes * 8
        self.nw = ((idat_bytes + 3) // 4 + 4 + 3) & ~3
        self.nmark = (self.nbits + PD_MARK_THREADS - 1) // PD_MARK_THREADS
        self.ncap = self.nbits // 64 + 256
        self.bcap = min(self.nbits // 18, self.need) + 2 + self.need // PD_CK + PD_CKMAX
        self.nslot = min(self.ncap, self.nbits // 4096 + 256)
        self.nparts = (self.need + 256 * PD_RESOLVE_BYTES - 1) // (256 * PD_RESOLVE_BYTES)
        self.rbp = (rb + 15) & ~15


class BitReader:
    def __init__(self, w, nw, pos):
        self.w, self.nw = w, nw
        assert 0 <= pos
        self.wt = pos >> 5
        self.cur = self.quad(self.wt & ~3)
        self.nxt = self.quad((self.wt & ~3) + 4)
        sh = pos & 31
        self.buf = self.take() >> sh
        self.cnt = 32 - sh
        self.refill()

    def quad(self, q):
        assert q >= 0 and q % 4 == 0
        if q + 4 <= self.nw:
            assert q + 3 < len(self.w)
            return self.w[q:q + 4]
        return (0, 0, 0, 0)

    def take(self):
        v = self.cur[self.wt & 3]
        self.wt += 1
        if (self.wt & 3) == 0:
            self.cur = self.nxt
            self.nxt = self.quad(self.wt + 4)
        return v

    def refill(self):
        if self.cnt <= 32:
            self.buf |= self.take() << self.cnt
            self.cnt += 32
            assert self.buf <= M64

    def bits(self, n):
        assert 0 <= n <= 32 and n <= self.cnt, (n, self.cnt)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def need(self, n):
        if self.cnt < n:
            self.refill()
        return self.bits(n)

    def pos(self):
        return self.wt * 32 - self.cnt


def slow_decode(b, count, sym, maxlen):
    """(symbol or -1, bits used)"""
    code = first = index = 0
    assert maxlen < len(count)
    for ln in range(1, maxlen + 1):
        code |= b & 1
        b >>= 1
        c = count[ln]
        if code - c < first:
            k = index + (code - first)
            assert 0 <= k < len(sym), (k, len(sym))
            return sym[k], ln
        index += c
        first += c
        first <<= 1
        code <<= 1
    return -1, 0


def code_check(count, codes):
    mx = 15
    while mx >= 1 and count[mx] == 0:
        mx -= 1
    if mx == 0:
        return 1 if codes else 0
    left = 1
    for ln in range(1, 16):
        left <<= 1
        left -= count[ln]
        if left < 0:
            return 1
    if left > 0 and (codes or mx != 1):
        return 1
    return 0


def word(w, nw, i):
    assert 0 <= i < nw, (i, nw)
    return w[i]


def prefilter(w, nw, pos):
    wi, sh = pos >> 5, pos & 31
    a = word(w, nw, wi) | word(w, nw, wi + 1) << 32
    b = word(w, nw, wi + 2) | word(w, nw, wi + 3) << 32
    if sh:
        a = ((a >> sh) | (b << (64 - sh))) & M64
        b >>= sh
    if ((a >> 1) & 3) != 2 or ((a >> 3) & 31) > 29 or ((a >> 8) & 31) > 29:
        return False
    ncode = ((a >> 13) & 15) + 4
    kraft = 0
    for i in range(ncode):
        o = 17 + 3 * i
        if o >= 64:
            ln = (b >> (o - 64)) & 7
        elif o > 61:
            ln = ((a >> o) | (b << (64 - o))) & 7
        else:
            ln = (a >> o) & 7
        if ln:
            kraft += 128 >> ln
    return kraft == 128


def dynamic_ok(w, nw, nbits, pos):
    """pd_dynamic_ok"""
    if pos + 17 > nbits:
        return False
    if not prefilter(w, nw, pos):
        return False
    br = BitReader(w, nw, pos)
    br.bits(1)
    if br.bits(2) != 2:
        return False
    nlen, ndist, ncode = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    if nlen > 286 or ndist > 30:
        return False
    cl = [0] * 19
    for i in range(ncode):
        cl[C_CLORDER[i]] = br.need(3)
    count, sym, offs = [0] * 16, [0] * 19, [0] * 16
    for i in range(19):
        count[cl[i]] += 1
    count[0] = 0
    if code_check(count, True):
        return False
    for ln in range(1, 15):
        offs[ln + 1] = offs[ln] + count[ln]
    for s in range(19):
        if cl[s]:
            assert offs[cl[s]] < 19
            sym[offs[cl[s]]] = s
            offs[cl[s]] += 1
    lcount, dcount = [0] * 16, [0] * 16
    idx = prev = eob = 0
    n = nlen + ndist
    while idx < n:
        br.refill()
        s, used = slow_decode(br.buf, count, sym, 7)
        if s < 0:
            return False
        br.bits(used)
        if s < 16:
            ln, rep = s, 1
        elif s == 16:
            if idx == 0:
                return False
            ln, rep = prev, 3 + br.bits(2)
        elif s == 17:
            ln, rep = 0, 3 + br.bits(3)
        else:
            ln, rep = 0, 11 + br.bits(7)
        if idx + rep > n:
            return False
        for _ in range(rep):
            assert 0 <= ln < 16
            if idx < nlen:
                lcount[ln] += 1
                if idx == 256:
                    eob = ln
            else:
                dcount[ln] += 1
            idx += 1
        prev = ln
        if br.pos() > nbits:
            return False
    lcount[0] = dcount[0] = 0
    return eob != 0 and not code_check(lcount, False) and not code_check(dcount, False)


def screen(stream, nbits):
    """Bit offsets >= 16 that pass the pre-filter, by numpy over all offsets at once (the same arithmetic as prefilter();
    mark() runs prefilter() itself on every survivor, and the CPU test holds the two against each other)."""
    bits = np.unpackbits(np.frombuffer(bytes(stream) + bytes(24), np.uint8), bitorder="little").astype(np.int32)
    n = nbits
    v3 = bits[:-2] + 2 * bits[1:-1] + 4 * bits[2:]

    def field(off, width):
        return sum(bits[off + k:off + k + n] << k for k in range(width))

    okay = (bits[1:1 + n] == 0) & (bits[2:2 + n] == 1) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    ncode = field(13, 4) + 4
    weight = np.array([0, 64, 32, 16, 8, 4, 2, 1], np.int32)
    kraft = np.zeros(n, np.int32)
    for i in range(19):
        kraft += np.where(i < ncode, weight[v3[17 + 3 * i:17 + 3 * i + n]], 0)
    okay &= kraft == 128
    pos = np.nonzero(okay)[0]
    return [int(p) for p in pos if p >= 16 and p + 17 <= nbits]


class Lds:
    """PdLds"""

    def __init__(self):
        self.lfast, self.dfast = [0] * (1 << PD_FB), [0] * (1 << PD_FB)
        self.lcnt, self.dcnt, self.clcnt = [0] * 16, [0] * 16, [0] * 16
        self.lsym, self.dsym, self.clsym = [0] * 288, [0] * 32, [0] * 19
        self.lens = [0] * 320
        self.kind = self.err = self.final_ = self.done = 0
        self.data_pos = self.end = self.bytes = self.stored_len = 0
        self.tables_of = None


def header(L, w, nw, nbits, pos, stream):
    """pd_header"""
    L.err = 0
    if pos + 3 > nbits:
        L.err = 5
        return
    br = BitReader(w, nw, pos)
    L.final_ = br.bits(1)
    L.kind = br.bits(2)
    if L.kind == 3:
        L.err = 1
        return
    if L.kind == 0:
        p = (br.pos() + 7) & ~7
        if p + 32 > nbits:
            L.err = 5
            return
        assert p // 8 + 3 < len(stream)
        ln = stream[p // 8] | stream[p // 8 + 1] << 8
        nl = stream[p // 8 + 2] | stream[p // 8 + 3] << 8
        if ln != (~nl & 0xFFFF):
            L.err = 2
            return
        L.data_pos = p + 32
        L.stored_len = ln
        if L.data_pos + 8 * ln > nbits:
            L.err = 5
        return
    nlen, ndist = 288, 32
    if L.kind == 1:
        for i in range(288):
            L.lens[i] = 8 if i < 144 else 9 if i < 256 else 7 if i < 280 else 8
        for i in range(32):
            L.lens[288 + i] = 5
    else:
        nlen, ndist, ncode = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
        if nlen > 286 or ndist > 30:
            L.err = 3
            return
        cl = [0] * 19
        for i in range(ncode):
            cl[C_CLORDER[i]] = br.need(3)
        for i in range(16):
            L.clcnt[i] = 0
        for i in range(19):
            L.clcnt[cl[i]] += 1
        L.clcnt[0] = 0
        if code_check(L.clcnt, True):
            L.err = 3
            return
        offs = [0] * 16
        for ln in range(1, 15):
            offs[ln + 1] = offs[ln] + L.clcnt[ln]
        for s in range(19):
            if cl[s]:
                assert offs[cl[s]] < 19
                L.clsym[offs[cl[s]]] = s
                offs[cl[s]] += 1
        tmp = [0] * 316
        idx, n = 0, nlen + ndist
        while idx < n:
            before = br.pos()
            br.refill()
            s, used = slow_decode(br.buf, L.clcnt, L.clsym, 7)
            if s < 0:
                L.err = 3
                return
            br.bits(used)
            if s < 16:
                ln, rep = s, 1
            elif s == 16:
                if idx == 0:
                    L.err = 3
                    return
                ln, rep = tmp[idx - 1], 3 + br.bits(2)
            elif s == 17:
                ln, rep = 0, 3 + br.bits(3)
            else:
                ln, rep = 0, 11 + br.bits(7)
            if idx + rep > n:
                L.err = 3
                return
            for _ in range(rep):
                assert idx < 316
                tmp[idx] = ln
                idx += 1
            assert br.pos() > before
            if br.pos() > nbits:
                L.err = 5
                return
        for i in range(288):
            L.lens[i] = tmp[i] if i < nlen else 0
        for i in range(32):
            L.lens[288 + i] = tmp[nlen + i] if i < ndist else 0
        if L.lens[256] == 0:
            L.err = 3
            return
    for i in range(16):
        L.lcnt[i] = L.dcnt[i] = 0
    for i in range(288):
        L.lcnt[L.lens[i]] += 1
    for i in range(32):
        L.dcnt[L.lens[288 + i]] += 1
    L.lcnt[0] = L.dcnt[0] = 0
    if code_check(L.lcnt, False) or code_check(L.dcnt, False):
        L.err = 3
        return
    lo, dof = [0] * 16, [0] * 16
    for ln in range(1, 15):
        lo[ln + 1] = lo[ln] + L.lcnt[ln]
        dof[ln + 1] = dof[ln] + L.dcnt[ln]
    for s in range(288):
        if L.lens[s]:
            assert lo[L.lens[s]] < 288
            L.lsym[lo[L.lens[s]]] = s
            lo[L.lens[s]] += 1
    for s in range(32):
        if L.lens[288 + s]:
            assert dof[L.lens[288 + s]] < 32
            L.dsym[dof[L.lens[288 + s]]] = s
            dof[L.lens[288 + s]] += 1
    L.data_pos = br.pos()


FAST = {}            # the tables of a set of code lengths, built once (the kernel builds them again for every block)


def fast_tables(L):
    key = bytes(L.lens)
    if key not in FAST:
        lfast, dfast = [0] * (1 << PD_FB), [0] * (1 << PD_FB)
        for e in range(1 << PD_FB):
            s, used = slow_decode(e, L.lcnt, L.lsym, PD_FB)
            lfast[e] = 0 if s < 0 else s << 4 | used
            s, used = slow_decode(e, L.dcnt, L.dsym, PD_FB)
            dfast[e] = 0 if s < 0 else s << 4 | used
        FAST[key] = (lfast, dfast)
    L.lfast, L.dfast = FAST[key]


def symbol(br, fast, cnt, sym):
    v = fast[br.buf & ((1 << PD_FB) - 1)]
    if v:
        br.bits(v & 15)
        return v >> 4
    s, used = slow_decode(br.buf, cnt, sym, 15)
    if s >= 0:
        br.bits(used)
    return s


def block(L, M, pos, write, base, cap, start=0, ckp=None):
    """pd_block.  M: the Model (stream, sizes, lit / src / written).  ckp: (checks array, first index) or None.  Returns nck."""
    w, nw, nbits, need = M.w, M.P.nw, M.P.nbits, M.P.need
    header(L, w, nw, nbits, pos, M.stream)
    L.done = 0
    L.bytes = 0
    if L.err:
        return 0
    if L.kind == 0:
        n = L.stored_len
        if write:
            at = L.data_pos // 8
            for k in range(n):
                o = base + k
                assert at + k < len(M.stream)
                if o < need:
                    M.put_lit(o, M.stream[at + k])
        L.end, L.bytes, L.done = L.data_pos + 8 * n, n, 1
        return 0
    fast_tables(L)
    br = BitReader(w, nw, start if start else L.data_pos)
    out = nsym = 0
    if not write:
        err = done = 0
        while True:
            before = br.pos()
            br.refill()
            s = symbol(br, L.lfast, L.lcnt, L.lsym)
            if s < 256:
                if s < 0:
                    err = 4
                    break
                out += 1
            elif s == 256:
                done = 1
                break
            else:
                ls = s - 257
                if ls >= 29:
                    err = 4
                    break
                out += C_LBASE[ls] + br.bits(C_LEXT[ls])
                br.refill()
                ds = symbol(br, L.dfast, L.dcnt, L.dsym)
                if ds < 0 or ds >= 30:
                    err = 4
                    break
                br.bits(C_DEXT[ds])
            assert br.pos() > before
            nsym += 1
            if (nsym & 255) == 0:
                if br.pos() > nbits:
                    err = 5
                    break
                if ckp is not None and (nsym & (PD_CK - 1)) == 0 and nsym <= PD_CAP_SYMBOLS:
                    k = nsym // PD_CK - 1
                    assert 0 <= k < PD_CKMAX and 0 <= ckp[1] + k < len(ckp[0])
                    ckp[0][ckp[1] + k] = (br.pos(), out)
                if nsym >= cap:
                    done = 2
                    break
        if br.pos() > nbits:
            err, done = 5, 0
        L.err, L.done, L.end, L.bytes = err, done, br.pos(), out
        return min(nsym // PD_CK, PD_CKMAX)
    while True:
        rec = []
        while len(rec) < PD_BATCH:
            before = br.pos()
            br.refill()
            s = symbol(br, L.lfast, L.lcnt, L.lsym)
            if s < 0:
                L.err = 4
                break
            if s < 256:
                rec.append((out, 0, s))
                out += 1
            elif s == 256:
                L.done = 1
                break
            else:
                ls = s - 257
                if ls >= 29:
                    L.err = 4
                    break
                ln = C_LBASE[ls] + br.bits(C_LEXT[ls])
                br.refill()
                ds = symbol(br, L.dfast, L.dcnt, L.dsym)
                if ds < 0 or ds >= 30:
                    L.err = 4
                    break
                dist = C_DBASE[ds] + br.bits(C_DEXT[ds])
                if dist > base + out:
                    L.err = -1
                    break
                rec.append((out, dist, ln))
                out += ln
            assert br.pos() > before
            if br.pos() > nbits:
                L.err = 5
                break
            nsym += 1
            if nsym >= cap:
                L.done = 2
                break
        assert len(rec) <= PD_BATCH
        for ro, d, v in rec:
            o = base + ro
            if d == 0:
                if o < need:
                    M.put_lit(o, v)
            else:
                k = 0
                while k < v and o + k < need:
                    M.put_src(o + k, o + k - d)
                    k += 1
        if L.err != 0 or L.done != 0:
            break
    L.end, L.bytes = br.pos(), out
    return 0


class Model:
    def __init__(self, stream, h, rb):
        self.stream = bytes(stream)
        self.P = P = Plan(len(self.stream), h, rb)
        assert P.nw - 4 >= (len(self.stream) + 3) // 4          # the last quad is zero padding, whatever quad()'s bound
        padded = self.stream + bytes(P.nw * 4 - len(self.stream))
        self.w = [int(x) for x in np.frombuffer(padded, "<u4")]
        assert len(self.w) == P.nw
        self.status = [0, 0]
        self.lit = [None] * P.need
        self.src = [None] * P.need
        self.trace = {"hits": [], "self": [], "segments": 0}

    def fail(self, code, detail):
        if self.status[0] == 0:
            self.status = [code, detail]

    def put_lit(self, o, v):
        assert 0 <= o < self.P.need and self.src[o] is None, ("lit", o)
        self.lit[o] = v
        self.src[o] = o

    def put_src(self, o, s):
        assert 0 <= o < self.P.need and self.src[o] is None, ("src", o)
        assert 0 <= s < o
        self.src[o] = s

    def mark(self):
        """k_pd_mark, k_pd_scan_u32, k_pd_compact: the sorted candidate positions, capped at ncap."""
        P = self.P
        hits = [p for p in screen(self.stream, P.nbits) if dynamic_ok(self.w, P.nw, P.nbits, p)]
        self.all_cands = hits
        for p in hits:
            assert p // 64 < P.nmark * (PD_MARK_THREADS // 64) and p // PD_MARK_THREADS < P.nmark     # masks, wgcnt
        self.cands = [{"pos": p} for p in hits[:P.ncap]]
        assert len(self.cands) <= P.ncap

    def pass_a(self):
        P = self.P
        self.checks = [None] * (P.nslot * PD_CKMAX)
        L = Lds()
        for c, cand in enumerate(self.cands):
            nck = block(L, self, cand["pos"], False, 0, PD_CAP_SYMBOLS, 0, (self.checks, c * PD_CKMAX) if c < P.nslot else None)
            cand.update(valid=L.err == 0 and L.done == 1, end=L.end, bytes=L.bytes, final_=L.final_,
                        nck=nck if c < P.nslot and L.kind != 0 else 0)

    def walk(self):
        P, s = self.P, self.stream
        cmf, flg = (s[0], s[1]) if len(s) >= 2 else (0, 0)
        if P.nbits < 16 or (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 != 0 or (flg & 32):
            self.fail(ZLIB_HEADER, -1 if P.nbits < 16 else (cmf << 8) | flg)
            return
        s_pos, s_out, stop = 16, 0, 0
        self.blocks = []
        ncand = len(self.cands)
        L = Lds()
        while True:
            lo, hi = 0, ncand
            while lo < hi:
                mid = (lo + hi) // 2
                assert 0 <= mid < P.ncap
                if self.cands[mid]["pos"] < s_pos:
                    lo = mid + 1
                else:
                    hi = mid
            hit = lo < ncand and self.cands[lo]["pos"] == s_pos and self.cands[lo]["valid"]
            if hit:
                c = self.cands[lo]
                end, nbytes, fin = c["end"], c["bytes"], c["final_"]
                self.trace["hits"].append(s_pos)
            else:
                block(L, self, s_pos, False, 0, NOLIMIT)
                if L.err:
                    self.fail(DEFLATE, L.err)
                    return
                end, nbytes, fin = L.end, L.bytes, L.final_
                self.trace["self"].append(s_pos)
            assert end > s_pos and end <= P.nbits
            if nbytes and s_out < P.need:
                nck = self.cands[lo]["nck"] if hit and lo < P.nslot else 0
                if len(self.blocks) + nck + 1 > P.bcap:
                    self.fail(INTERNAL, 1)
                    stop = 1
                else:
                    self.blocks.append((s_pos, 0, s_out, PD_CK if nck else NOLIMIT))
                    for i in range(1, nck + 1):
                        k = lo * PD_CKMAX + i - 1
                        assert 0 <= k < len(self.checks) and self.checks[k] is not None, k
                        ck_pos, ck_out = self.checks[k]
                        if s_out + ck_out >= P.need:
                            break
                        self.blocks.append((s_pos, ck_pos, s_out + ck_out, NOLIMIT if i == nck else PD_CK))
                    assert len(self.blocks) <= P.bcap
            s_out += nbytes
            s_pos = end
            if fin:
                stop = stop or 2
            if stop:
                break
        if stop == 2:
            self.total = s_out
            self.adler_byte = (s_pos + 7) // 8
            if s_out == P.need and self.adler_byte + 4 > P.nbits // 8:
                self.fail(DEFLATE, 5)

    def pass_b(self):
        L = Lds()
        first_far = None
        for b, (pos, start, out, limit) in enumerate(self.blocks):
            block(L, self, pos, True, out, limit, start)
            if L.err:
                if L.err < 0 and first_far is None:
                    first_far = out
                elif L.err > 0:
                    self.fail(DEFLATE, L.err)
            elif b + 1 < len(self.blocks) and self.blocks[b + 1][0] == pos:
                assert L.end == self.blocks[b + 1][1] and out + L.bytes == self.blocks[b + 1][2], "segment does not meet the next"
        if first_far is not None:
            self.fail(FAR, first_far & 0x7FFFFFFF)
        self.trace["segments"] = len(self.blocks)

    def jump(self):
        P = self.P
        n = P.need
        if self.total < n:
            self.fail(SHORT, min(self.total, 0x7FFFFFFF))
            return
        assert all(x is not None for x in self.src), "an output byte no segment wrote"
        src = np.array(self.src, np.int64)
        idx = np.arange(n, dtype=np.int64)
        assert np.all((src >= 0) & (src <= idx))
        rounds = 1
        while (1 << (rounds - 1)) < n and rounds < 64:
            rounds += 1
        changed = True
        for r in range(rounds):
            if not changed:
                break
            t = src[src]
            changed = bool(np.any(t != src))
            src = t
        assert np.all(src[src] == src), "pointer jumping did not finish in the host's rounds"
        self.src = src

    def resolve(self):
        P = self.P
        n = P.need
        lit = np.array([0 if v is None else v for v in self.lit], np.int64)
        assert all(self.lit[int(s)] is not None for s in np.unique(self.src)), "a source that is no literal"
        v = lit[self.src]
        idx = np.arange(n, dtype=np.int64)
        r, col = idx // (P.rb + 1), idx % (P.rb + 1)
        assert r.max(initial=0) < P.h and (col.max(initial=0) - 1) < P.rbp
        a = b = 0
        per = 256 * PD_RESOLVE_BYTES
        for part in range(P.nparts):
            x, i = v[part * per:(part + 1) * per], idx[part * per:(part + 1) * per]
            a += int(x.sum()) % PD_ADLER_MOD
            b += int(((n - i) * x).sum()) % PD_ADLER_MOD
        self.out = bytes(v.astype(np.uint8))
        if self.total == n:
            assert self.adler_byte + 4 <= len(self.stream)
            t = self.stream[self.adler_byte:self.adler_byte + 4]
            want = t[0] << 24 | t[1] << 16 | t[2] << 8 | t[3]
            if (((n % PD_ADLER_MOD + b) % PD_ADLER_MOD) << 16 | (1 + a) % PD_ADLER_MOD) != want:
                self.fail(ADLER, 0)

    def run(self):
        if self.P.nmark:
            self.mark()
            self.pass_a()
        else:
            self.cands, self.all_cands, self.checks = [], [], []
        for step in (self.walk, self.pass_b, self.jump, self.resolve):
            step()
            if self.status[0]:
                return tuple(self.status)
        return self.out


def decode(stream, h, rb):
    """The filtered bytes (h * (1 + rb) of them) or the (code, detail) the kernels would leave, and the Model for its trace."""
    m = Model(stream, h, rb)
    return m.run(), m
