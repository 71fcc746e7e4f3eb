"""NumPy model of baseline JPEG decoding at 1/2, 1/4 and 1/8 scale (helper, not collected): what Pillow returns after
``draft`` has set ``decoderconfig == (scale, 0)``, and what ``lars.decode_jpeg(data, scale)`` is written against.

Built on ``jpeg_model`` (parser, entropy decoder, 8 x 8 IDCT, fancy upsampling, colour formulas), which it imports and
does not change.  The rules, from libjpeg's scaling code (jdmaster.c, jidctred.c, jdsample.c), restated:

* geometry: the output is ``ceil(w / scale)`` x ``ceil(h / scale)``; ``m = 8 / scale`` is the smallest block; a component
  starts at ``s = m`` and doubles it while ``s < 8`` and both ``hmax * m`` and ``vmax * m`` are multiples of ``h_c * s * 2``
  and ``v_c * s * 2``.  So luma has ``m``, the chroma of 4:2:0 has ``2 m`` (and is not upsampled at all), the chroma of 4:2:2
  has ``m`` and is upsampled horizontally.
* reduced IDCTs of 4 x 4, 2 x 2 and 1 x 1 samples (``idct4``, ``idct2``, ``idct1``) in the arithmetic of libjpeg-turbo's
  SIMD code for 4 x 4 and 2 x 2 (what Pillow's wheels run) and of its C code for 1 x 1: see the functions.
* upsampling: the triangle filter of full scale on the scaled planes at 1/2 and 1/4 (replication where the chroma plane
  is at most two samples wide); plain replication at 1/8, where libjpeg-turbo turns fancy upsampling off.
* colour as at full scale.

Out-of-range blocks, fitted against Pillow on hand-built files (test_jpeg_scaled_cpu.py) and frozen:

* every size: the product of coefficient and quantiser keeps its low 16 bits, as at full scale -- except 1 x 1, which is C
  code: the quantiser is read as a signed 16-bit number and the product is exact.
* 4 x 4: a block whose coefficient rows 1, 2, 3, 5, 6, 7 are zero in all eight columns (row 0 may hold AC terms, row 4
  anything) takes the short cut ``row 0 << 2`` wrapping at 16 bits; otherwise the column results saturate at 16 bits; the
  32-bit sums wrap; the row results saturate to 8 bits.
* 2 x 2: no short cut; the column results of column 0 stay 32-bit numbers whose shift by 15 in the row pass wraps at 32
  bits, those of columns 1, 3, 5, 7 saturate at 16 bits; the row results saturate to 8 bits.
* 1 x 1: ``(DC * q + 4) >> 3`` goes through libjpeg's range-limit table, which wraps modulo 1024: 0 .. 127 -> 128 .. 255,
  128 .. 511 -> 255, 512 .. 895 -> 0, 896 .. 1023 -> 0 .. 127.

No class of block is left out: the fitted model equals Pillow on every hand-built extreme file of the CPU suite.
"""
import numpy as np

import jpeg_model as M
from jpeg_model import wrap

SCALES = (1, 2, 4, 8)


def fix(x):
    return int(round(x * 8192))


def coefficients(d):
    """The frame and its coefficients: (h, w, comps, quantisation tables, coefs [MCU][block][64] with the DC summed and
    everything in 16 bits, MCUs across, MCUs down).  ``jpeg_model.decode`` up to the IDCT, with its errors."""
    d = bytes(d)
    (h, w, comps), q, ht, ri, scan, p = M.parse(d)
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    mw, mh = -(-w // (8 * hm)), -(-h // (8 * vm))
    tables, owner = [], []
    for ci, (cid, ch, cv, _tq) in enumerate(comps):
        td, ta = [(x[1], x[2]) for x in scan if x[0] == cid][0]
        if td not in ht or 16 + ta not in ht:
            raise ValueError("missing Huffman table")
        tables += [(ht[td], ht[16 + ta])] * (ch * cv)
        owner += [ci] * (ch * cv)
    bpm, nmcu = len(tables), mw * mh
    per = ri if 0 < ri < nmcu else nmcu
    intervals = M.entropy_intervals(d, p)
    if len(intervals) != -(-nmcu // per):
        raise ValueError("a restart marker is missing or extra")
    coefs = np.zeros((nmcu * bpm, 64), np.int64)
    for i, data in enumerate(intervals):
        want = (min(per, nmcu - i * per)) * bpm
        if M.decode_interval(data, tables, bpm, coefs, i * per * bpm) != want:
            raise ValueError("entropy data does not hold the blocks of the frame")
    coefs = coefs.reshape(nmcu, bpm, 64)
    for i in range(0, nmcu, per):
        for ci in range(len(comps)):
            idx = [b for b in range(bpm) if owner[b] == ci]
            seg = coefs[i:i + per, idx, 0]
            coefs[i:i + per, idx, 0] = np.cumsum(seg.reshape(-1)).reshape(seg.shape)
    for c in comps:
        if c[3] not in q:
            raise ValueError("missing quantisation table")
    return h, w, comps, q, wrap(coefs, 16), mw, mh


def block_sizes(comps, scale):
    """Samples per side of one block of each component at this scale."""
    m = 8 // scale
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    out = []
    for _cid, ch, cv, _tq in comps:
        s = m
        while s < 8 and (hm * m) % (ch * s * 2) == 0 and (vm * m) % (cv * s * 2) == 0:
            s *= 2
        out.append(s)
    return out


def descale(v, shift):
    return wrap(v + (1 << (shift - 1)), 32) >> shift


def pass4(x, shift):
    """The 4-point pass over axis -2 of x [..., 8, n] (entry 4 is not read) -> [..., 4, n], saturated to 16 bits."""
    x0, x1, x2, x3, _x4, x5, x6, x7 = (x[..., i, :] for i in range(8))
    t0 = x0 << 14
    t2 = x2 * fix(1.847759065) - x6 * fix(0.765366865)
    a0 = -x7 * fix(0.211164243) + x5 * fix(1.451774981) - x3 * fix(2.172734803) + x1 * fix(1.061594337)
    a2 = -x7 * fix(0.509795579) - x5 * fix(0.601344887) + x3 * fix(0.899976223) + x1 * fix(2.562915447)
    rows = [t0 + t2 + a2, t0 - t2 + a0, t0 - t2 - a0, t0 + t2 - a2]
    return np.stack([np.clip(descale(r, shift), -32768, 32767) for r in rows], axis=-2)


def idct4(coef, quant):
    """Coefficients [n, 8, 8], quantiser [8, 8] -> samples [n, 4, 4]."""
    x = wrap(coef * quant, 16)
    short_cut = (coef[:, [1, 2, 3, 5, 6, 7], :] == 0).all(axis=(1, 2))
    ws = pass4(x, 12)                                        # columns: [n, 4, 8]
    ws = np.where(short_cut[:, None, None], np.broadcast_to(wrap(x[:, :1, :] << 2, 16), ws.shape), ws)
    out = pass4(ws.swapaxes(-1, -2), 19).swapaxes(-1, -2)    # rows: [n, 4, 4]
    return np.clip(out, -128, 127) + 128


def odd2(x):
    """The odd part of the 2-point pass over axis -2 of x [..., 8, n]: entries 1, 3, 5, 7."""
    x1, x3, x5, x7 = (x[..., i, :] for i in (1, 3, 5, 7))
    return -x7 * fix(0.720959822) + x5 * fix(0.850430095) - x3 * fix(1.272758580) + x1 * fix(3.624509785)


def idct2(coef, quant):
    """Coefficients [n, 8, 8], quantiser [8, 8] -> samples [n, 2, 2].  Rows and columns 0, 1, 3, 5, 7 only."""
    x = wrap(coef * quant, 16)
    t10, t0 = x[:, 0, :] << 15, odd2(x)
    ws = np.stack([descale(t10 + t0, 13), descale(t10 - t0, 13)], axis=-2).swapaxes(-1, -2)   # columns: [n, 8, 2]
    t10 = wrap(ws[:, 0, :] << 15, 32)                        # column 0 stays a 32-bit number and the shift wraps
    t0 = odd2(np.clip(ws, -32768, 32767))                    # the others are narrowed to 16 bits by saturation
    out = np.stack([descale(t10 + t0, 20), descale(t10 - t0, 20)], axis=-2).swapaxes(-1, -2)
    return np.clip(out, -128, 127) + 128


def idct1(coef, quant):
    """Coefficients [n, 8, 8], quantiser [8, 8] -> samples [n, 1, 1]: C code, through the range-limit table."""
    v = wrap(coef[:, 0, 0] * wrap(quant[0, 0], 16) + 4, 32) >> 3
    i = v & 1023
    out = np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))
    return out.reshape(-1, 1, 1)


IDCT = {8: M.idct_blocks, 4: idct4, 2: idct2, 1: idct1}


def planes(d, scale):
    """(h, w of the output, comps, the sample planes padded to whole blocks, their block sizes); ``d``: the file, or what
    ``coefficients`` made of it (the entropy decoder is the slow part: a caller decoding at several scales runs it once)."""
    h, w, comps, q, coefs, mw, mh = d if isinstance(d, tuple) else coefficients(d)
    sizes = block_sizes(comps, scale)
    out, b0 = [], 0
    for (_cid, ch, cv, tq), s in zip(comps, sizes):
        blocks = coefs[:, b0:b0 + ch * cv].reshape(-1, 8, 8)
        b0 += ch * cv
        px = IDCT[s](blocks, np.array(q[tq], np.int64).reshape(8, 8)).reshape(mh, mw, cv, ch, s, s)
        out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(mh * cv * s, mw * ch * s))
    return -(-h // scale), -(-w // scale), comps, out, sizes


def decode(d, scale=1):
    """``np.asarray(im)`` of a baseline JPEG file after ``im.draft`` has set ``decoderconfig == (scale, 0)``; ``d`` as for
    ``planes``."""
    if scale not in SCALES:
        raise ValueError(f"scale 1, 2, 4 or 8, got {scale!r}")
    h, w, comps, P, sizes = planes(d, scale)
    if len(comps) == 1:
        return P[0][:h, :w].astype(np.uint8)
    m = 8 // scale
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    up = []
    for plane, c, s in zip(P, comps, sizes):
        hf, vf = hm * m // (c[1] * s), vm * m // (c[2] * s)
        if m > 1:
            up.append(M.upsample(plane, w, h, hf, vf))
        else:
            up.append(np.repeat(np.repeat(plane, vf, axis=0), hf, axis=1)[:h, :w])
    Y, Cb, Cr = up
    cb, cr = Cb - 128, Cr - 128
    F = lambda x: int(x * 65536 + 0.5)                      # noqa: E731
    R = Y + ((F(1.40200) * cr + 32768) >> 16)
    G = Y + ((-F(0.34414) * cb - F(0.71414) * cr + 32768) >> 16)
    B = Y + ((F(1.77200) * cb + 32768) >> 16)
    return np.clip(np.dstack([R, G, B]), 0, 255).astype(np.uint8)


def pillow_scaled(d, scale):
    """Pillow's array of the file at this scale.  ``draft`` is asked where it grants the scale (both sides at least
    ``scale``); a smaller picture gets the same decoder settings written the way ``draft`` writes them."""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(bytes(d)))
    w, h = im.size
    if scale == 1:
        return np.asarray(im)
    if w >= scale and h >= scale:
        im.draft(None, (w // scale, h // scale))
    else:
        dec, ext, off, args = im.tile[0]
        im._size = (-(-w // scale), -(-h // scale))
        im.tile = [(dec, (0, 0) + im._size, off, args)]
        im.decoderconfig = (scale, 0)
    assert im.decoderconfig == (scale, 0) and im.size == (-(-w // scale), -(-h // scale)), (im.decoderconfig, im.size)
    return np.asarray(im)
