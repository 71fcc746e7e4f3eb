"""Hand-built JPEG files (tests/jpeg_writer.py) on the CPU: the NumPy model against the installed Pillow on every file, jpeg_info,
what each group is there to pin (tables routed per component), and the sanitizer build replaying the files.

Every JPEG file of test_jpeg_decode_cpu.py comes from Pillow's encoder: two Huffman table pairs with ids 0 / 1, Cb and Cr
sharing every table, 8-bit DQT, JFIF, no fill bytes, coefficients of a forward DCT.  The files here are everything else the
host parser accepts.  HANDMADE maps a name to a function that builds the file (built on first use, then kept); the GPU tests
import it.  Pillow is the oracle and the model the explanation: a file on which they differ is a bug in the model.
"""
import functools
import hashlib
import io
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image, features

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_model  # noqa: E402
import jpeg_writer as W  # noqa: E402
from test_jpeg_decode_cpu import asan_bin, find, lib_jpeg_info, want  # noqa: E402,F401

MODES = ("L", "444", "422", "420")
FUZZ_SEED, FUZZ_N = 20261016, 48


def nblocks(w, h, mode):
    mcux, mcuy, layout = W.geometry(w, h, W.SAMPLING[mode])
    return mcux * mcuy, layout


def content(rng, w, h, mode, kind, dc=200):
    """Seeded coefficients [block][64] for a frame: "flat", "sparse", "dense", "large" (+-300, dense), "huge" (+-1023, dense),
    "mixed" (each block one of them); chroma gets its own statistics so that no two components want the same tables."""
    nmcu, layout = nblocks(w, h, mode)
    n = nmcu * len(layout)
    comp = np.array(layout * nmcu)
    c = np.zeros((n, 64), np.int64)
    kinds = np.full(n, ["flat", "sparse", "dense", "large", "huge"].index(kind)) if kind != "mixed" else rng.choice(5, n, p=[.3, .3, .2, .1, .1])
    sparse = rng.integers(-6, 7, (n, 64)) * (rng.random((n, 64)) < 0.08)
    dense = rng.integers(-20, 21, (n, 64))
    large = rng.integers(-300, 301, (n, 64))
    huge = rng.integers(-1023, 1024, (n, 64))
    for k, src in ((1, sparse), (2, dense), (3, large), (4, huge)):
        c[kinds == k] = src[kinds == k]
    c[comp == 1] = c[comp == 1] // 2 + (c[comp == 1] != 0)      # Cb: smaller, shifted up
    c[comp == 2, 32:] = 0                                       # Cr: upper half of the natural order only
    c[:, 0] = np.where(kinds == 0, 0, rng.integers(-dc, dc + 1, n))
    c[kinds == 0, 0] = (np.arange(n)[kinds == 0] % 7 == 0) * 40 - 20 * (comp[kinds == 0] == 2)
    return c


def qtable(rng, lo, hi):
    return [int(x) for x in rng.integers(lo, hi + 1, 64)]


def build(w, h, mode, coefs, qts=None, dc_shape=None, ac_shape=None, **kw):
    ids = {k: kw.get(k, (0, 1, 1)) for k in ("td", "ta")}
    ri = kw.get("ri", 0)
    hts = W.tables_for(coefs, W.SAMPLING[mode], ri, w, h, ids["td"], ids["ta"], dc_shape, ac_shape)
    qts = qts or {t: [1 + (3 * k + 5 * t) % 11 for k in range(64)] for t in range(4)}
    return W.write(w, h, W.SAMPLING[mode], coefs, qts, hts, **kw)


def single(symbols):
    assert len(symbols) == 1, symbols
    return W.shape_single(symbols[0])


def pattern_blocks(n, comp):
    """The coefficient patterns a Huffman block decoder has branches for, block after block."""
    zz = np.zeros((n, 64), np.int64)                        # in zigzag order first
    for i in range(n):
        k = i % 16
        if k == 0:
            pass                                            # only EOB
        elif k in (1, 2, 3):
            zz[i, 16 * k + 1] = 3                           # k ZRLs in a row, then a coefficient
        elif k == 4:
            zz[i, 63] = -1                                  # ends in a nonzero coefficient 63: no EOB (three ZRLs before it)
        elif k == 5:
            zz[i, 16], zz[i, 32], zz[i, 48] = 1, -2, 5      # runs of 15 without ZRL
        elif k == 6:
            zz[i, 1:11] = [(-1) ** s * ((1 << s) - 1) for s in range(1, 11)]   # AC sizes 1-10, largest magnitudes
        elif k == 7:
            zz[i, 1:11] = [(-1) ** s * (1 << (s - 1)) for s in range(1, 11)]   # AC sizes 1-10, smallest magnitudes
        elif k == 8:
            zz[i, 1:] = 1                                   # all 63 coefficients
        elif k == 9:
            zz[i, 62] = 7                                   # three ZRLs and a run, EOB after coefficient 62
        elif k == 10:
            zz[i, 1], zz[i, 63] = -512, 1023
        else:
            zz[i, 1 + (i * 7) % 63] = (i % 5) - 2
    dc = np.zeros(n, np.int64)
    for c in range(3):                                      # per component: every difference category 0-11, swings of +-2047
        idx = np.flatnonzero(comp == c)
        seq = [0, 0, 1, -1, 3, -4, 11, -20, 43, -84, 171, -340, 683, -1023, 1024, -1023, 1024, 0, 2047 - 1023, -1023]
        dc[idx] = [seq[j % len(seq)] for j in range(len(idx))]
    out = np.zeros((n, 64), np.int64)
    out[:, W.ZIGZAG] = zz
    out[:, 0] = dc
    return out


def fuzz_file(k):
    rng = np.random.default_rng([FUZZ_SEED, k])
    w, h = int(rng.integers(1, 201)), int(rng.integers(1, 201))
    mode = MODES[int(rng.integers(4))]
    nmcu, layout = nblocks(w, h, mode)
    coefs = content(rng, w, h, mode, ["mixed", "sparse", "dense", "large", "huge", "flat"][int(rng.integers(6))], dc=int(rng.choice([30, 500, 1023])))
    three = lambda: tuple(int(x) for x in rng.integers(0, 4, 3))   # noqa: E731
    ids = [(1, 2, 3), (0, 1, 2), (7, 40, 200), (82, 71, 65)][int(rng.integers(4))]
    header = ["jfif", "adobe", None][int(rng.integers(3))]
    if ids == (82, 71, 65) and header is None:              # "RGB" with no header would mean RGB stored: not decoded here
        header = "adobe"
    ac_shape = [None, None, W.shape_long, W.shape_all_16, W.shape_256, W.shape_staircase][int(rng.integers(6))]
    dc_shape = [None, None, W.shape_long, W.shape_all_16, W.shape_staircase][int(rng.integers(5))]
    big_q = bool(rng.integers(2))
    qts = {t: qtable(rng, 1, 2000 if big_q else 255) for t in range(4)}
    ri = int(rng.choice([0, 0, 1, 2, 3, 5, max(nmcu - 1, 1), nmcu, nmcu + 9, -(-w // 8)]))
    return build(w, h, mode, coefs, qts, dc_shape, ac_shape, tq=three(), td=three(), ta=three(), ids=ids, header=header, ri=ri,
                 pq=int(big_q), sof=int(rng.choice([0xC0, 0xC1])), split=bool(rng.integers(2)), redefine=bool(rng.integers(2)),
                 dri_twice=bool(rng.integers(2)), fill=int(rng.integers(3)), fill_rst=int(rng.integers(4)), extras=bool(rng.integers(2)),
                 trailer=b"after EOI \xff\xd8" * int(rng.integers(2)))


def handmade():
    """name -> function building the file.  The name starts with the group."""
    out = {}

    def add(name, fn, *a, **k):
        assert name not in out
        out[name] = functools.lru_cache(maxsize=None)(lambda: fn(*a, **k))

    def rng_of(name):
        return np.random.default_rng(list(name.encode()))

    # --- distinct tables per component
    def distinct(mode, tq, td, ta):
        rng = rng_of(f"distinct {mode}")
        qts = {0: qtable(rng, 1, 8), 1: qtable(rng, 9, 30), 2: qtable(rng, 31, 90), 3: qtable(rng, 91, 200)}
        return build(37, 29, mode, content(rng, 37, 29, mode, "dense", dc=60), qts, tq=tq, td=td, ta=ta)

    for mode in MODES[1:]:
        add(f"tables {mode} ids 0 1 2", distinct, mode, (0, 1, 2), (0, 1, 2), (0, 1, 2))
        add(f"tables {mode} ids permuted", distinct, mode, (3, 0, 2), (2, 0, 1), (3, 1, 0))
    add("tables L ids 3 2 3", lambda: build(37, 29, "L", content(rng_of("dl"), 37, 29, "L", "dense"), tq=(3,), td=(2,), ta=(3,)))

    # --- Huffman shapes
    def shaped(mode, dc_shape, ac_shape, kind, w=45, h=23, ri=0):
        rng = rng_of(f"shape {mode} {kind}")
        if kind == "eob only":                              # a one-code AC table can only say EOB; a one-code DC table only 0
            coefs = np.zeros((len(nblocks(w, h, mode)[1]) * nblocks(w, h, mode)[0], 64), np.int64)
            if dc_shape is not single:
                coefs[:, 0] = rng.integers(-50, 51, len(coefs))
        elif kind == "31-bit symbols":                      # AC size 15 behind a 16-bit code, DC category 11 behind one too
            coefs = rng.choice([-32767, -16384, 16384, 32767], (len(nblocks(w, h, mode)[1]) * nblocks(w, h, mode)[0], 64))
            coefs[:, 0] = rng.choice([-1023, 1024], len(coefs))
            coefs[::3, 5:] = 0
        else:
            coefs = content(rng, w, h, mode, kind)
        qts = {t: [1] * 64 for t in range(4)} if kind == "31-bit symbols" else None
        return build(w, h, mode, coefs, qts, dc_shape, ac_shape, ri=ri, td=(0, 1, 2), ta=(0, 1, 2))

    for mode in MODES:
        add(f"huffman {mode} all 16 bits but two", shaped, mode, W.shape_long, W.shape_long, "mixed")
        add(f"huffman {mode} all 16 bits", shaped, mode, W.shape_all_16, W.shape_all_16, "dense")
        add(f"huffman {mode} single code", shaped, mode, single, single, "eob only")
        add(f"huffman {mode} single AC code", shaped, mode, None, single, "eob only")
        add(f"huffman {mode} 255 codes of 8 bits", shaped, mode, None, W.shape_255x8, "mixed")
        add(f"huffman {mode} 256 values", shaped, mode, W.shape_staircase, W.shape_256, "mixed")
        add(f"huffman {mode} staircase", shaped, mode, W.shape_staircase, W.shape_staircase, "dense")
        add(f"huffman {mode} 31-bit symbols", shaped, mode, W.shape_all_16, W.shape_all_16, "31-bit symbols")
        add(f"huffman {mode} 31-bit symbols restarts", shaped, mode, W.shape_all_16, W.shape_long, "31-bit symbols", ri=2)
        add(f"huffman {mode} from statistics huge", shaped, mode, None, None, "huge", w=120, h=64)

    # --- coefficient patterns
    def patterns(mode, ri):
        nmcu, layout = nblocks(61, 50, mode)
        coefs = pattern_blocks(nmcu * len(layout), np.array(layout * nmcu))
        return build(61, 50, mode, coefs, {t: [1] * 64 for t in range(4)}, ri=ri, td=(0, 1, 2), ta=(0, 1, 2))

    for mode in MODES:
        add(f"patterns {mode}", patterns, mode, 0)
        add(f"patterns {mode} restart 3", patterns, mode, 3)

    # --- 16-bit DQT, SOF1
    def wide(mode, sof, pq):
        rng = rng_of(f"wide {mode}")
        coefs = content(rng, 40, 24, mode, "sparse", dc=3) // 3
        qts = {t: qtable(rng, 256, 2000) if pq == 1 or t in pq else qtable(rng, 1, 255) for t in range(4)}
        return build(40, 24, mode, coefs, qts, sof=sof, pq=pq, tq=(0, 1, 2))

    for mode in MODES:
        add(f"dqt16 {mode} SOF0", wide, mode, 0xC0, 1)
        add(f"dqt16 {mode} SOF1", wide, mode, 0xC1, 1)
        add(f"dqt16 {mode} SOF1 tables 0 and 2 wide", wide, mode, 0xC1, (0, 2))

    # --- header variants
    def headed(mode, **kw):
        rng = rng_of(f"header {mode}")
        return build(33, 47, mode, content(rng, 33, 47, mode, "mixed", dc=100), ri=kw.pop("ri", 0), **kw)

    for mode in MODES:
        add(f"header {mode} adobe", headed, mode, header="adobe")
        add(f"header {mode} none ids 1 2 3", headed, mode, header=None)
        add(f"header {mode} none ids 0 1 2", headed, mode, header=None, ids=(0, 1, 2))
        add(f"header {mode} none ids 7 40 200", headed, mode, header=None, ids=(7, 40, 200))
        add(f"header {mode} tables redefined", headed, mode, redefine=True)
        add(f"header {mode} tables split", headed, mode, split=True, td=(0, 1, 2), ta=(2, 1, 0))
        add(f"header {mode} extras everywhere", headed, mode, extras=True, split=True, ri=4, trailer=b"\xff\xd8 bytes after EOI")
        add(f"header {mode} fill 2", headed, mode, fill=2, fill_rst=0, ri=4)

    # --- restart variants
    def restarts(mode, which, **kw):
        w, h = 75, 41
        nmcu, layout = nblocks(w, h, mode)
        mcux = W.geometry(w, h, W.SAMPLING[mode])[0]
        ri = {"1": 1, "row-1": mcux - 1, "row+1": mcux + 1, "count-1": nmcu - 1, "count": nmcu, "count+7": nmcu + 7, "65535": 65535}[which]
        rng = rng_of(f"restart {mode}")
        coefs = content(rng, w, h, mode, "mixed")
        if kw.pop("flat_runs", False):                      # intervals of one flat MCU (two bytes) between long ones
            mcu = np.arange(len(coefs)) // len(layout)
            coefs[(mcu % 5 != 0)] = 0
        return build(w, h, mode, coefs, ri=ri, **kw)

    for mode in MODES:
        for which in ("1", "row-1", "row+1", "count-1", "count", "count+7", "65535"):
            add(f"restart {mode} DRI {which}", restarts, mode, which)
        add(f"restart {mode} DRI twice", restarts, mode, "row+1", dri_twice=True)
        add(f"restart {mode} DRI twice then none", restarts, mode, "count", dri_twice=True)
        for n in (1, 2, 3):
            add(f"restart {mode} {n} fill before RSTn and EOI", restarts, mode, "1" if n == 2 else "row-1", fill=n)
        add(f"restart {mode} flat MCUs", restarts, mode, "1", flat_runs=True)
        add(f"restart {mode} flat MCUs fill 1", restarts, mode, "1", flat_runs=True, fill_rst=1)

    # --- thin and large frames: a small coefficient set repeated
    def framed(w, h, mode, ri):
        nmcu, layout = nblocks(w, h, mode)
        base = content(rng_of(f"frame {mode}"), 64, 16, mode, "sparse", dc=80)
        base = base[:len(base) // len(layout) * len(layout)]
        coefs = np.tile(base, (-(-nmcu * len(layout) // len(base)), 1))[:nmcu * len(layout)]
        return build(w, h, mode, coefs, ri=ri)

    for mode in ("L", "444", "420"):                        # 65500 is the most libjpeg (the oracle) takes
        add(f"frame {mode} 1 x 65500", framed, 1, 65500, mode, 0)
        add(f"frame {mode} 65500 x 1", framed, 65500, 1, mode, 100)
        add(f"frame {mode} 8 x 30000", framed, 8, 30000, mode, 1)
        add(f"frame {mode} 30000 x 8", framed, 30000, 8, mode, 0)
    add("frame 422 65500 x 2", framed, 65500, 2, "422", 7)
    add("frame 420 16 x 16", framed, 16, 16, "420", 0)
    add("frame 420 16 x 16 restart 1", framed, 16, 16, "420", 1)
    add("frame 420 17 x 17", framed, 17, 17, "420", 0)

    # --- blocks whose IDCT output leaves the 10-bit window, between normal ones
    def outside(mode, kind, where):
        w, h = 56, 40
        rng = rng_of(f"outside {mode} {kind} {where}")
        nmcu, layout = nblocks(w, h, mode)
        comp = np.array(layout * nmcu)
        coefs = content(rng, w, h, mode, "sparse", dc=60)
        hot = (np.arange(len(coefs)) % 5 == 0) & ((comp == 0) if where == "Y" else (comp > 0))
        n = int(hot.sum())
        q = 1
        if kind == "single AC":                             # one large coefficient: exact output up to about +-2300
            blk = np.zeros((n, 64), np.int64)
            blk[np.arange(n), rng.integers(1, 64, n)] = rng.choice([-1023, -700, 600, 1023], n)
            blk[:, 0] = rng.integers(-300, 301, n)
            q = 9
        elif kind == "dense 300":
            blk = rng.integers(-300, 301, (n, 64))
        elif kind == "dense 1023":
            blk = rng.integers(-1023, 1024, (n, 64))
        elif kind == "just outside":                        # DC alone: exact output +-513 ... +-640
            blk = np.zeros((n, 64), np.int64)
            blk[:, 0] = rng.choice([-1, 1], n) * rng.integers(513, 641, n)
            q = 8
        elif kind == "DC alone, large":                     # the column pass's short cut, where DC * 4 leaves 16 bits
            blk = np.zeros((n, 64), np.int64)
            blk[:, 0] = rng.choice([-1, 1], n) * rng.integers(500, 1024, n)
            q = 17
        elif kind == "zero quantiser":                      # rows 1-7 hold coefficients that a quantiser of 0 wipes out: the
            blk = rng.integers(-5, 6, (n, 64))              # short cut looks at the coefficients, so it is not taken
            blk[:, 1:8] = 0
            blk[:, 8] = 1
            blk[:, 0] = rng.choice([-1, 1], n) * rng.integers(500, 1024, n)
            q = 17
        else:                                               # "DC row": row 0 only, the short cut with AC terms
            blk = np.zeros((n, 64), np.int64)
            blk[:, :8] = rng.integers(-1023, 1024, (n, 8))
            q = 13
        coefs[hot] = blk
        qts = {t: [q] * 8 + [0 if kind == "zero quantiser" else q] * 56 for t in range(4)}
        return build(w, h, mode, coefs, qts)

    for mode in MODES:
        for kind in ("single AC", "dense 300", "dense 1023", "just outside", "DC alone, large", "DC row", "zero quantiser"):
            add(f"outside {mode} {kind} in Y", outside, mode, kind, "Y")
            if mode != "L":
                add(f"outside {mode} {kind} in chroma", outside, mode, kind, "chroma")

    for k in range(FUZZ_N):
        add(f"fuzz {k:02d}", fuzz_file, k)
    return out


HANDMADE = handmade()


@functools.lru_cache(maxsize=None)
def beyond_the_oracle(name):
    """Frames of 65535 samples, the most a frame header can say: libjpeg stops at 65500, so Pillow refuses these files and
    only the model (equal to Pillow on every file above) can say what is in them."""
    w, h, mode, ri = {"L 1 x 65535": (1, 65535, "L", 0), "L 65535 x 1": (65535, 1, "L", 64), "420 1 x 65535": (1, 65535, "420", 3),
                      "420 65535 x 1": (65535, 1, "420", 0), "444 65535 x 1": (65535, 1, "444", 1)}[name]
    nmcu, layout = nblocks(w, h, mode)
    base = content(np.random.default_rng(65535), 64, 16, mode, "sparse", dc=80)
    base = base[:len(base) // len(layout) * len(layout)]
    return build(w, h, mode, np.tile(base, (-(-nmcu * len(layout) // len(base)), 1))[:nmcu * len(layout)], ri=ri)


BEYOND = ("L 1 x 65535", "L 65535 x 1", "420 1 x 65535", "420 65535 x 1", "444 65535 x 1")
GROUPS = ("tables", "huffman", "patterns", "dqt16", "header", "restart", "frame", "outside", "fuzz")


def files_of(*groups):
    return [n for n in sorted(HANDMADE) if n.split()[0] in groups]


def test_every_group_is_there():
    assert {n.split()[0] for n in HANDMADE} == set(GROUPS)
    assert len(files_of("fuzz")) == FUZZ_N


def test_the_oracle_is_a_simd_build_of_libjpeg_turbo():
    """The bit-exactness claim is for Pillow on libjpeg-turbo with its SIMD code in use (every x86-64 and arm64 wheel): outside
    the 10-bit window around the sample centre the SIMD IDCT saturates where the C code wraps."""
    assert features.check_feature("libjpeg_turbo"), f"Pillow's JPEG library is libjpeg {features.version('jpg')}, not libjpeg-turbo"
    assert not os.environ.get("JSIMD_FORCENONE"), "libjpeg-turbo's SIMD code is switched off: the C IDCT wraps out-of-range samples"


@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_model_equals_pillow(name):
    b = HANDMADE[name]()
    ref = want(b)
    got = jpeg_model.decode(b)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes(), f"{int((got != ref).sum())} of {ref.size} samples differ"


def test_sse2_and_avx2_code_of_the_oracle_agree():
    """libjpeg-turbo picks its IDCT by the host's CPU; its SSE2 and AVX2 code must give the same samples outside the 10-bit
    window too, or the claim would depend on the machine.  A fresh interpreter with JSIMD_FORCESSE2 decodes the group."""
    names = files_of("outside")
    code = ("import sys, io, hashlib; sys.path[:0] = sys.argv[1:3]; import numpy as np; from PIL import Image\n"
            "from test_jpeg_handmade_cpu import HANDMADE, files_of\n"
            "for n in files_of('outside'): print(hashlib.sha256(np.asarray(Image.open(io.BytesIO(HANDMADE[n]()))).tobytes()).hexdigest())")
    env = dict(os.environ, JSIMD_FORCESSE2="1")
    here = Path(__file__).resolve().parent
    run = subprocess.run([sys.executable, "-c", code, str(here), str(here.parent)], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.split() == [hashlib.sha256(want(HANDMADE[n]()).tobytes()).hexdigest() for n in names], \
        "libjpeg-turbo's SSE2 and AVX2 IDCT differ on this host: the oracle depends on the SIMD path"


def test_out_of_range_group_leaves_the_window():
    """The group is what it says: in every file some exact IDCT output (jidctint.c's arithmetic before its range-limit
    table) lies beyond +-512, where a wrap at 10 bits and a saturation part ways."""
    real = jpeg_model.idct_blocks
    for name in files_of("outside"):
        peak = []

        def spy(c, q):
            peak.append(int(np.abs(exact_idct(c * q)).max()))
            return real(c, q)

        try:
            jpeg_model.idct_blocks = spy
            jpeg_model.decode(HANDMADE[name]())
        finally:
            jpeg_model.idct_blocks = real
        assert max(peak) > 512, (name, peak)


def exact_idct(c):
    """jidctint.c's two passes in exact integers, centred on 0, no range limit."""
    F = jpeg_model.FIX

    def one(x, shift):
        x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., i, :] for i in range(8))
        z1 = (x2 + x6) * F["f0_541"]
        t2, t3 = z1 - x6 * F["f1_847"], z1 + x2 * F["f0_765"]
        t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        z1, z2, z3, z4 = x7 + x1, x5 + x3, x7 + x3, x5 + x1
        z5 = (z3 + z4) * F["f1_175"]
        z3, z4 = z5 - z3 * F["f1_961"], z5 - z4 * F["f0_390"]
        a0 = x7 * F["f0_298"] - z1 * F["f0_899"] + z3
        a1 = x5 * F["f2_053"] - z2 * F["f2_562"] + z4
        a2 = x3 * F["f3_072"] - z2 * F["f2_562"] + z3
        a3 = x1 * F["f1_501"] - z1 * F["f0_899"] + z4
        rows = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
        return np.stack([(r + (1 << (shift - 1))) >> shift for r in rows], axis=-2)

    return one(one(c, 11).swapaxes(-1, -2), 18).swapaxes(-1, -2)


def test_beyond_the_oracle_files_are_refused_by_pillow_and_taken_by_jpeg_info():
    for name in BEYOND:
        b = beyond_the_oracle(name)
        with pytest.raises(OSError):
            Image.open(io.BytesIO(b)).load()
        info = lars.jpeg_info(b)
        assert info["supported"] is True and 65535 in info["size"]
        assert b[info["entropy_offset"] + info["entropy_bytes"]:] == b"\xff\xd9"


@pytest.mark.parametrize("mode", MODES[1:])
def test_every_component_needs_its_own_tables(mode):
    """In the "tables" group no two components can share a table: the same coefficients written with the contents of two
    quantisation tables exchanged decode to another picture, and with two Huffman tables exchanged to another picture or
    to an error."""
    rng = np.random.default_rng(list(f"distinct {mode}".encode()))
    qts = {0: qtable(rng, 1, 8), 1: qtable(rng, 9, 30), 2: qtable(rng, 31, 90), 3: qtable(rng, 91, 200)}
    coefs = content(rng, 37, 29, mode, "dense", dc=60)
    tq, td, ta = (3, 0, 2), (2, 0, 1), (3, 1, 0)
    hts = W.tables_for(coefs, W.SAMPLING[mode], 0, 37, 29, td, ta)
    good = W.write(37, 29, W.SAMPLING[mode], coefs, qts, hts, tq=tq, td=td, ta=ta)
    assert good == HANDMADE[f"tables {mode} ids permuted"]()
    ref = jpeg_model.decode(good)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        swapped = list(tq)
        swapped[a], swapped[b] = tq[b], tq[a]
        other = patch_ids(good, tq=swapped)
        assert jpeg_model.decode(other).tobytes() != ref.tobytes(), ("tq", a, b)
        for key, ids in (("td", td), ("ta", ta)):
            swapped = list(ids)
            swapped[a], swapped[b] = ids[b], ids[a]
            try:
                assert jpeg_model.decode(patch_ids(good, **{key: swapped})).tobytes() != ref.tobytes(), (key, a, b)
            except ValueError:
                pass


def patch_ids(b, tq=None, td=None, ta=None):
    """The file with other table ids in its frame and scan headers: the decoder is pointed at the wrong tables."""
    b = bytearray(b)
    (_h, _w, comps), _q, _ht, _ri, scan, eoff = jpeg_model.parse(bytes(b))
    sof, sos = find(bytes(b), 0xC0)[0], find(bytes(b), 0xDA)[0]   # a walk over the segments, not a search for bytes
    assert sos + 8 + 2 * len(scan) == eoff
    for c in range(len(comps)):
        if tq:
            b[sof + 12 + 3 * c] = tq[c]
        cur = b[sos + 6 + 2 * c]
        b[sos + 6 + 2 * c] = ((td[c] if td else cur >> 4) << 4) | (ta[c] if ta else cur & 15)
    return bytes(b)


# ---------------------------------------------------------------------------------------------------------------------
# jpeg_info
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_jpeg_info_on_handmade_files(monkeypatch, name):
    monkeypatch.setattr(_ffi, "call", lambda *_a, **_k: (_ for _ in ()).throw(AssertionError("the library was called")))
    b = HANDMADE[name]()
    im = Image.open(io.BytesIO(b))
    info = lars.jpeg_info(b)
    assert info["supported"] is True and info["reason"] is None, info
    assert info["size"] == im.size and info["mode"] == im.mode
    (_h, _w, comps), _q, _ht, ri, _scan, eoff = jpeg_model.parse(b)
    assert info["restart_interval"] == ri
    assert info["entropy_offset"] == eoff
    if im.mode == "RGB":
        assert tuple(info["sampling"][0]) == (comps[0][1], comps[0][2])
    end = info["entropy_offset"] + info["entropy_bytes"]    # the entropy data ends where EOI (with its fill bytes) begins
    rest = b[end:]
    assert rest.lstrip(b"\xff")[:1] == b"\xd9" and rest[:1] == b"\xff", rest[:8]


# ---------------------------------------------------------------------------------------------------------------------
# the sanitizer build
# ---------------------------------------------------------------------------------------------------------------------
def test_sanitizer_replays_handmade_files(asan_bin, tmp_path):
    names = sorted(HANDMADE)
    cases = []
    for n in names:
        b = HANDMADE[n]()
        cases.append(b)
        if not n.startswith("frame") or len(b) <= 8000:
            cases += [b[:cut] for cut in range(0, len(b), 97)]           # truncated at every 97th byte
        else:                                                            # the long frame files: the head and the tail
            cases += [b[:cut] for cut in list(range(0, 4000, 97)) + list(range(len(b) - 2000, len(b), 97))]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for b in cases:
            f.write(struct.pack("<4I", 4, 0, 0, len(b)) + b)
    run = subprocess.run([asan_bin, str(path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == f"done {len(cases)} cases"
    ok = 0
    for line, b in zip(lines, cases):
        rc, h = lib_jpeg_info(b)
        assert line.split(" ", 1)[1] == f"jpeg rc={rc} h={h:016x}", line
        ok += rc == 0
    assert ok >= len(names)
