"""NumPy model of the baseline JPEG encoder the device code is written against (helper, not collected): libjpeg's forward
path as Pillow drives it by default -- colour conversion, edge repetition, downsampling, ``jfdctint`` (ISLOW), quantisation,
dummy blocks -- up to the quantised coefficients in scan order.  ``test_jpeg_encode_cpu.py`` pins it to the installed Pillow
through the coefficients read back from Pillow's own files (``jpeg_model``), and ``jpeg_writer.write`` turns its coefficients
into the whole file.  The tables are read out of files Pillow writes here; nothing is typed in.
"""
import io
import struct

import numpy as np
from PIL import Image

import jpeg_model as jm

SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}


def pillow_file(arr, **save):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG", **save)
    return f.getvalue()


def segments(d):
    """[(marker, whole segment bytes)] up to and including SOS, and the offset of the entropy data."""
    p, out = 2, []
    while True:
        m = d[p + 1]
        (n,) = struct.unpack(">H", d[p + 2:p + 4])
        out.append((m, d[p:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out, p


_STD = {}


def standard_tables():
    """({id: base quantisation table, natural order}, {(class, id): (counts, values)}) of a quality-50 file: at quality 50
    libjpeg's scale factor is 100 %, so the file holds the annex K.1 tables themselves, next to the annex K.3 Huffman tables."""
    if not _STD:
        d = pillow_file(np.zeros((8, 8, 3), np.uint8), quality=50)
        _frame, q, _ht, _ri, _scan, _p = jm.parse(d)
        hts = {}
        for m, seg in segments(d)[0]:
            if m == 0xC4:
                body = seg[4:]
                hts[(body[0] >> 4, body[0] & 15)] = (list(body[1:17]), list(body[17:]))
        _STD["q"], _STD["h"] = q, hts
    return _STD["q"], _STD["h"]


def quant_tables(quality):
    """libjpeg's jpeg_set_quality: the base tables scaled by jpeg_quality_scaling(quality), forced to 1..255."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return {t: [min(max((b * s + 50) // 100, 1), 255) for b in base] for t, base in standard_tables()[0].items()}


C = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)


def fdct_1d(d, first):
    """One pass of jfdctint over the last axis: 13 constant bits, 2 pass-1 bits."""
    def ds(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        o[..., 0] = (t10 + t11) << 2
        o[..., 4] = (t10 - t11) << 2
    else:
        o[..., 0] = ds(t10 + t11, 2)
        o[..., 4] = ds(t10 - t11, 2)
    z1 = (t12 + t13) * C["c"]
    o[..., 2] = ds(z1 + t13 * C["d"], n)
    o[..., 6] = ds(z1 - t12 * C["h"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["f"]
    t4, t5, t6, t7 = t4 * C["a"], t5 * C["j"], t6 * C["l"], t7 * C["g"]
    z1, z2, z3, z4 = -z1 * C["e"], -z2 * C["k"], -z3 * C["i"], -z4 * C["b"]
    z3, z4 = z3 + z5, z4 + z5
    o[..., 7] = ds(t4 + z1 + z3, n)
    o[..., 5] = ds(t5 + z2 + z4, n)
    o[..., 3] = ds(t6 + z2 + z3, n)
    o[..., 1] = ds(t7 + z1 + z4, n)
    return o


def fdct_quant(plane, qt):
    """plane [8 * bh, 8 * bw] samples -> [bh, bw, 64] quantised coefficients, natural order."""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.astype(np.int64).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
    b = fdct_1d(b, True)                                      # rows
    b = fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)   # columns: 8 x the DCT
    div = np.array(qt, np.int64).reshape(8, 8) << 3
    mag = (np.abs(b) + (div >> 1)) // div
    return (np.sign(b) * mag).reshape(bh, bw, 64)


def forward(arr, quality=75, subsampling="4:2:0"):
    """Quantised coefficients [blocks in scan order, 64] (natural order, DC as the value itself) of the file Pillow writes for
    ``arr`` ([H, W] or [H, W, 3] uint8), and the sampling of the luminance (``None`` for one component)."""
    a = np.asarray(arr).astype(np.int64)
    h, w = a.shape[:2]
    q = quant_tables(quality)
    if a.ndim == 2:
        planes, hm, vm = [a], 1, 1
        comps = [(1, 1, 0)]                                   # (h sampling, v sampling, quantisation table)
    else:
        hm, vm = SUBSAMPLING[subsampling]
        R, G, B = a[..., 0], a[..., 1], a[..., 2]
        Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
        Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
        Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
        planes = [Y, Cb, Cr]
        comps = [(hm, vm, 0), (1, 1, 1), (1, 1, 1)]
    mw, mh = -(-w // (8 * hm)), -(-h // (8 * vm))
    H, W = mh * vm * 8, mw * hm * 8
    hg = -(-h // vm) * vm                                     # pixel rows repeat up to a whole row group before downsampling ...
    planes = [np.pad(p, ((0, hg - h), (0, W - w)), mode="edge") for p in planes]
    out = []
    for p, (ch, cv, tq) in zip(planes, comps):
        fh, fv = hm // ch, vm // cv
        if (fh, fv) == (2, 2):
            s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
            p = (s + np.tile([1, 2], s.shape[1] // 2 + 1)[:s.shape[1]]) >> 2
        elif (fh, fv) == (2, 1):
            s = p[:, 0::2] + p[:, 1::2]
            p = (s + np.tile([0, 1], s.shape[1] // 2 + 1)[:s.shape[1]]) >> 1
        p = np.pad(p, ((0, H // fv - p.shape[0]), (0, 0)), mode="edge")   # ... and the DOWNSAMPLED rows up to the MCU row
        co = fdct_quant(p, q[tq]).reshape(mh, cv, mw, ch, 64).transpose(0, 2, 1, 3, 4).copy()   # [mh, mw, cv, ch, 64]
        # a block beyond the component's own size in blocks is a dummy: AC zero, DC of the block before it in the MCU
        wb, hb = -(-(-(-w // fh)) // 8), -(-(-(-h // fv)) // 8)
        for my in range(mh):
            for mx in range(mw):
                last = None
                for y in range(cv):
                    for x in range(ch):
                        if mx * ch + x < wb and my * cv + y < hb:
                            last = co[my, mx, y, x, 0]
                        else:
                            co[my, mx, y, x, :] = 0
                            co[my, mx, y, x, 0] = last
        out.append(co.reshape(mh, mw, cv * ch, 64))
    coefs = np.concatenate(out, axis=2).reshape(-1, 64)
    return coefs, (None if a.ndim == 2 else (hm, vm))


def pillow_coefs(d):
    """The quantised coefficients of a baseline file, [blocks in scan order, 64], DC as the value itself: the entropy decoder of
    ``jpeg_model`` with the DC differences summed up."""
    (h, w, comps), q, ht, ri, scan, p = jm.parse(d)
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
    mw, mh = -(-w // (8 * hm)), -(-h // (8 * vm))
    tables, owner = [], []
    for ci, (cid, ch, cv, _tq) in enumerate(comps):
        td, ta = [(x[1], x[2]) for x in scan if x[0] == cid][0]
        tables += [(ht[td], ht[16 + ta])] * (ch * cv)
        owner += [ci] * (ch * cv)
    bpm, nmcu = len(tables), mw * mh
    assert ri == 0
    (data,) = jm.entropy_intervals(d, p)
    coefs = np.zeros((nmcu * bpm, 64), np.int64)
    assert jm.decode_interval(data, tables, bpm, coefs, 0) == nmcu * bpm
    coefs = coefs.reshape(nmcu, bpm, 64)
    for ci in range(len(comps)):
        idx = [b for b in range(bpm) if owner[b] == ci]
        seg = coefs[:, idx, 0]
        coefs[:, idx, 0] = np.cumsum(seg.reshape(-1)).reshape(seg.shape)
    return coefs.reshape(-1, 64), q


def one_over_f(h, w, c, seed):
    """A 1/f scene: the spectrum of photographs.  [h, w] for c = 1, else [h, w, c]; clipped a little at both ends."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1
    out = []
    for _ in range(c):
        s = np.fft.ifft2(np.fft.fft2(rng.standard_normal((h, w))) / f).real
        span = s.max() - s.min()
        out.append((s - s.min()) / (span if span > 0 else 1.0))
    a = np.dstack(out) if c > 1 else out[0]
    return (a * 300 - 20).clip(0, 255).astype(np.uint8)
