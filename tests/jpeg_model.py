"""NumPy / pure-Python model of the baseline JPEG decoder the device code is written against (helper, not collected).

``decode(file)`` restates libjpeg-turbo's ``JDCT_ISLOW`` path (its SIMD arithmetic, see ``idct_blocks``) with fancy upsampling
-- what Pillow returns at full scale -- with a plain sequential entropy decoder in front: one bit reader, one restart interval after the other.  It is as strict as
``lars.decode_jpeg``: entropy data that ends early, a bit pattern that is no code, a coefficient index past 63, a restart
marker that is missing or out of sequence and a block count that is not the frame's raise ``ValueError``.
``test_jpeg_decode_cpu.py`` pins it to the installed Pillow bit for bit; the GPU tests use it to confirm that their damaged
files are damaged in the way they say.
"""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]


def parse(d):
    """Marker segments up to the end of SOS: frame, tables, restart interval, start of the entropy data."""
    if d[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    p, q, ht, ri, frame = 2, {}, {}, 0, None
    while True:
        if p + 4 > len(d) or d[p] != 0xFF:
            raise ValueError("no marker where one should be")
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        p += 2
        (n,) = struct.unpack(">H", d[p:p + 2])
        if n < 2 or p + n > len(d):
            raise ValueError("segment length leaves the file")
        s = d[p + 2:p + n]
        if m == 0xDB:
            i = 0
            while i < len(s):
                pq, tq = s[i] >> 4, s[i] & 15
                i += 1
                if pq:
                    t = list(struct.unpack(">64H", s[i:i + 128]))
                    i += 128
                else:
                    t = list(s[i:i + 64])
                    i += 64
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = t[k]
                q[tq] = nat
        elif m == 0xC4:
            i = 0
            while i < len(s):
                tc, cnt = s[i], s[i + 1:i + 17]
                i += 17
                vals = s[i:i + sum(cnt)]
                i += sum(cnt)
                code, k, tab = 0, 0, {}
                for ln in range(1, 17):
                    for _ in range(cnt[ln - 1]):
                        tab[(ln, code)] = vals[k]
                        k += 1
                        code += 1
                    code <<= 1
                ht[tc] = tab
        elif m in (0xC0, 0xC1):
            _prec, h, w, nc = struct.unpack(">BHHB", s[:6])
            frame = (h, w, [(s[6 + 3 * i], s[7 + 3 * i] >> 4, s[7 + 3 * i] & 15, s[8 + 3 * i]) for i in range(nc)])
        elif m == 0xDD:
            (ri,) = struct.unpack(">H", s)
        elif m == 0xDA:
            if frame is None:
                raise ValueError("SOS before the frame header")
            scan = [(s[1 + 2 * i], s[2 + 2 * i] >> 4, s[2 + 2 * i] & 15) for i in range(s[0])]
            return frame, q, ht, ri, scan, p + n
        p += n


def entropy_intervals(d, p):
    """The entropy segment from byte ``p``: one destuffed byte string per restart interval; markers checked in sequence."""
    out, cur, expect = [], bytearray(), 0
    while p < len(d):
        c = d[p]
        if c != 0xFF:
            cur.append(c)
            p += 1
            continue
        q = p + 1
        while q < len(d) and d[q] == 0xFF:
            q += 1
        if q >= len(d):
            break
        if d[q] == 0:
            cur.append(0xFF)
        elif 0xD0 <= d[q] <= 0xD7:
            if d[q] != 0xD0 + expect % 8:
                raise ValueError("restart marker out of sequence")
            expect += 1
            out.append(bytes(cur))
            cur = bytearray()
        else:
            break                                            # EOI or another marker ends the segment
        p = q + 1
    out.append(bytes(cur))
    return out


def extend(v, k):
    return v if k == 0 or v >= (1 << (k - 1)) else v - (1 << k) + 1


def decode_interval(data, tables, nblocks_mcu, coefs, first_block):
    """Blocks of one restart interval into ``coefs`` (DC as the difference); returns how many it held.  A symbol that
    would cross the end of the interval is the padding of its last byte: decoding stops there."""
    nbits = len(data) * 8
    buf = data + b"\0\0\0\0\0"
    pos, b, k, blk = 0, 0, 0, first_block
    while pos < nbits:
        tab = tables[b][0 if k == 0 else 1]
        window = (int.from_bytes(buf[pos >> 3:(pos >> 3) + 5], "big") >> (8 - (pos & 7))) & 0xFFFFFFFF
        sym = None
        for ln in range(1, 17):
            sym = tab.get((ln, window >> (32 - ln)))
            if sym is not None:
                break
        if sym is None:
            if pos + 16 > nbits:
                break
            raise ValueError("a bit pattern that is no code of the table in use")
        s = sym & 15
        if pos + ln + s > nbits:
            break
        v = extend((window >> (32 - ln - s)) & ((1 << s) - 1), s) if s else 0
        pos += ln + s
        done = False
        if k == 0:
            if sym > 15:
                raise ValueError("DC category above 15")
            if blk < len(coefs):
                coefs[blk][0] = v
            k = 1
        elif s == 0:
            if sym >> 4 == 15:
                k += 16
                done = k > 63
            else:
                done = True
        else:
            k += sym >> 4
            if k > 63:
                raise ValueError("a coefficient index past 63")
            if blk < len(coefs):
                coefs[blk][ZIGZAG[k]] = v
            k += 1
            done = k > 63
        if done:
            blk, k, b = blk + 1, 0, (b + 1) % nblocks_mcu
    return blk - first_block


FIX = {name: int(round(x * 8192)) for name, x in dict(
    f0_298=0.298631336, f0_390=0.390180644, f0_541=0.541196100, f0_765=0.765366865, f0_899=0.899976223, f1_175=1.175875602,
    f1_501=1.501321110, f1_847=1.847759065, f1_961=1.961570560, f2_053=2.053119869, f2_562=2.562915447, f3_072=3.072711026).items()}


def wrap(x, bits):
    """Two's-complement wrap of an integer array to ``bits`` bits."""
    half = 1 << (bits - 1)
    return ((x + half) & ((1 << bits) - 1)) - half


def idct_pass(x, shift):
    """One 8-point pass of the slow-integer IDCT over the second-to-last axis of ``x`` ([..., 8, n]) in the arithmetic of
    libjpeg-turbo's SIMD code: inputs are 16-bit lanes, so the four sums that are formed before a multiplication
    (x0 + x4, x0 - x4, x7 + x3, x5 + x1) wrap at 16 bits; each rotation is one multiply-add with the constants folded,
    exact in 32 bits; the 32-bit sums wrap; the descaled result is packed with signed saturation to 16 bits."""
    F = FIX
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i, :] for i in range(8))
    t2 = x2 * F["f0_541"] + x6 * (F["f0_541"] - F["f1_847"])
    t3 = x2 * (F["f0_541"] + F["f0_765"]) + x6 * F["f0_541"]
    t0 = wrap(x0 + x4, 16) << 13
    t1 = wrap(x0 - x4, 16) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z3, z4 = wrap(x7 + x3, 16), wrap(x5 + x1, 16)
    z3, z4 = z3 * (F["f1_175"] - F["f1_961"]) + z4 * F["f1_175"], z3 * F["f1_175"] + z4 * (F["f1_175"] - F["f0_390"])
    a0 = x7 * (F["f0_298"] - F["f0_899"]) + x1 * -F["f0_899"] + z3
    a1 = x5 * (F["f2_053"] - F["f2_562"]) + x3 * -F["f2_562"] + z4
    a2 = x5 * -F["f2_562"] + x3 * (F["f3_072"] - F["f2_562"]) + z3
    a3 = x7 * -F["f0_899"] + x1 * (F["f1_501"] - F["f0_899"]) + z4
    half = 1 << (shift - 1)
    rows = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([np.clip(wrap(r + half, 32) >> shift, -32768, 32767) for r in rows], axis=-2)


def idct_blocks(coef, quant):
    """Coefficients [n, 8, 8] and their quantisation table [8, 8] -> samples [n, 8, 8] as libjpeg-turbo's SIMD
    ``jsimd_idct_islow`` gives them (SSE2 and AVX2 alike), which is what Pillow's wheels run.  Inside the 10-bit window
    around the sample centre it is libjpeg's C code (jidctint.c) bit for bit; outside, where the C code wraps through its
    range-limit table, the SIMD code narrows by saturation: the product of coefficient and quantiser keeps its low 16
    bits; a block whose coefficients of rows 1-7 are all zero (row 0 may hold AC terms) takes a short cut in the column
    pass, row 0 * 4 wrapping at 16 bits; every other column result saturates at 16 bits; the row results saturate to 16
    and then to 8 bits."""
    x = wrap(coef * quant, 16)
    dc_only = (coef[:, 1:, :] == 0).all(axis=(1, 2))         # the coefficients, not the products: a quantiser may be 0
    ws = idct_pass(x, 11)                                    # columns
    short = np.broadcast_to(wrap(x[:, :1, :] << 2, 16), x.shape)
    ws = np.where(dc_only[:, None, None], short, ws)
    out = idct_pass(ws.swapaxes(-1, -2), 18).swapaxes(-1, -2)   # rows
    return np.clip(out, -128, 127) + 128


def upsample(P, w, h, hf, vf):
    """A chroma plane (padded to whole blocks) to the image size, libjpeg's way: triangle filters where the plane is more
    than two samples wide, replication else; the neighbours outside the real samples are the edge samples."""
    if hf == 1 and vf == 1:
        return P[:h, :w]
    cw, chh = -(-w // hf), -(-h // vf)
    P = P[:, :cw]
    if cw <= 2:
        return np.repeat(np.repeat(P, vf, axis=0), hf, axis=1)[:h, :w]
    if vf == 2:
        P = P[:chh]
        A = np.vstack([P[:1], P, P[-1:]])
        T = np.empty((2 * chh, cw), np.int64)
        T[0::2] = 3 * A[1:-1] + A[:-2]
        T[1::2] = 3 * A[1:-1] + A[2:]
        L = np.hstack([T[:, :1], T[:, :-1]])
        R = np.hstack([T[:, 1:], T[:, -1:]])
        O = np.empty((2 * chh, 2 * cw), np.int64)
        O[:, 0::2] = (3 * T + L + 8) >> 4
        O[:, 1::2] = (3 * T + R + 7) >> 4
        O[:, 0] = (4 * T[:, 0] + 8) >> 4
        O[:, -1] = (4 * T[:, -1] + 7) >> 4
    else:
        T = P
        L = np.hstack([T[:, :1], T[:, :-1]])
        R = np.hstack([T[:, 1:], T[:, -1:]])
        O = np.empty((T.shape[0], 2 * cw), np.int64)
        O[:, 0::2] = (3 * T + L + 1) >> 2
        O[:, 1::2] = (3 * T + R + 2) >> 2
        O[:, 0] = T[:, 0]
        O[:, -1] = T[:, -1]
    return O[:h, :w]


def decode(d):
    """``np.asarray(Image.open(io.BytesIO(d)))`` of a baseline JPEG file (L, or YCbCr at 4:4:4, 4:2:2, 4:2:0)."""
    d = bytes(d)
    (h, w, comps), q, ht, ri, scan, p = parse(d)
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    mw, mh = -(-w // (8 * hm)), -(-h // (8 * vm))
    tables, owner = [], []                                   # per block of an MCU: (DC table, AC table), component
    for ci, (cid, ch, cv, _tq) in enumerate(comps):
        td, ta = [(x[1], x[2]) for x in scan if x[0] == cid][0]
        if td not in ht or 16 + ta not in ht:
            raise ValueError("missing Huffman table")
        tables += [(ht[td], ht[16 + ta])] * (ch * cv)
        owner += [ci] * (ch * cv)
    bpm, nmcu = len(tables), mw * mh
    per = ri if 0 < ri < nmcu else nmcu
    intervals = entropy_intervals(d, p)
    if len(intervals) != -(-nmcu // per):
        raise ValueError("a restart marker is missing or extra")
    coefs = np.zeros((nmcu * bpm, 64), np.int64)
    for i, data in enumerate(intervals):
        want = (min(per, nmcu - i * per)) * bpm
        if decode_interval(data, tables, bpm, coefs, i * per * bpm) != want:
            raise ValueError("entropy data does not hold the blocks of the frame")
    coefs = coefs.reshape(nmcu, bpm, 64)
    for i in range(0, nmcu, per):                            # DC prediction restarts with every interval
        for ci in range(len(comps)):
            idx = [b for b in range(bpm) if owner[b] == ci]
            seg = coefs[i:i + per, idx, 0]
            coefs[i:i + per, idx, 0] = np.cumsum(seg.reshape(-1)).reshape(seg.shape)
    coefs = wrap(coefs, 16)                                  # a coefficient is stored in 16 bits, the running DC too
    planes, b0 = [], 0
    for ci, (_cid, ch, cv, tq) in enumerate(comps):
        if tq not in q:
            raise ValueError("missing quantisation table")
        blocks = coefs[:, b0:b0 + ch * cv]
        b0 += ch * cv
        px = idct_blocks(blocks.reshape(-1, 8, 8), np.array(q[tq], np.int64).reshape(8, 8)).reshape(mh, mw, cv, ch, 8, 8)
        planes.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(mh * cv * 8, mw * ch * 8))
    if len(comps) == 1:
        return planes[0][:h, :w].astype(np.uint8)
    Y, Cb, Cr = (upsample(P, w, h, hm // c[1], vm // c[2]) for P, c in zip(planes, comps))
    cb, cr = Cb - 128, Cr - 128
    F = lambda x: int(x * 65536 + 0.5)                      # noqa: E731
    R = Y + ((F(1.40200) * cr + 32768) >> 16)
    G = Y + ((-F(0.34414) * cb - F(0.71414) * cr + 32768) >> 16)
    B = Y + ((F(1.77200) * cb + 32768) >> 16)
    return np.clip(np.dstack([R, G, B]), 0, 255).astype(np.uint8)
