"""CPU checks of the Deflate side of the TIFF decoder: the model of k_td_inflate (tiff_inflate_model.py) against
tiffio._chunk -- zlib, the specification -- on hand-built streams and on a seeded fuzz, lars_tiff_info_deflate against
lars_tiff_info, and the routing of deflate=True / "device+deflate".  test_gpu_tiff_deflate.py sends the same streams to the
kernel."""
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import deflate_writer as dw
import tiff_cases as tc
import tiff_inflate_model as model
from lars_image_processing_amd import _ffi, api, tiffio
from test_tiff_decode_cpu import asan_bin, files_of_every_kind, fnv  # noqa: F401  (asan_bin is a fixture)
from test_tiffio import sample


def chunk_outcome(stream, want):
    """tiffio._chunk on one chunk, in the words of model.outcome."""
    try:
        return ("bytes", tiffio._chunk(memoryview(bytes(stream)), 0, len(stream), 8, want))
    except tiffio.TiffError as e:
        text = str(e)
        if "corrupt Deflate data" in text:
            return ("corrupt",)
        if "inflates past" in text:
            return ("past",)
        n, m = (int(x) for x in text.replace("strip / tile holds ", "").replace(" bytes,", "").replace(" expected", "").split())
        return ("short", n, m)


def deflate_strip_tiff(stream, nbytes, compression=8):
    """tc.one_strip_tiff with the Deflate tag: a 1 x nbytes 8-bit picture whose only strip is ``stream``."""
    return tc.build_tiff({256: [nbytes], 257: [1], 258: [8], 259: [compression], 262: [1], 277: [1], 278: [1]}, [stream])


def with_compression(blob, value):
    """A little-endian file with its Compression tag set to ``value``."""
    out = bytearray(blob)
    ifd = struct.unpack_from("<I", out, 4)[0]
    for i in range(struct.unpack_from("<H", out, ifd)[0]):
        if struct.unpack_from("<H", out, ifd + 2 + 12 * i)[0] == tiffio.COMPRESSION:
            struct.pack_into("<H", out, ifd + 2 + 12 * i + 8, value)
    return bytes(out)


def restreamed(blob, streams):
    """The Deflate file ``blob`` with the streams of some strips / tiles replaced: {chunk: bytes}, as tc.lzw_tiff's ``streams``."""
    endian = "<" if blob[:2] == b"II" else ">"
    tags = tiffio._read_ifd(memoryview(blob), endian)
    tiled = tiffio.TILE_WIDTH in tags
    t_off, t_cnt = (tiffio.TILE_OFFSETS, tiffio.TILE_BYTE_COUNTS) if tiled else (tiffio.STRIP_OFFSETS, tiffio.STRIP_BYTE_COUNTS)
    blobs = [blob[o:o + c] for o, c in zip(tags[t_off], tags[t_cnt])]
    for k, s in streams.items():
        blobs[k] = s
    return tc.build_tiff({t: v for t, v in tags.items() if t not in (t_off, t_cnt)}, blobs, endian, t_off, t_cnt)


def header(cmf, fdict=False):
    flg = 32 if fdict else 0
    rest = ((cmf << 8) | flg) % 31
    return bytes([cmf, flg + (31 - rest if rest else 0)])


def lits(data):
    return [("lit", x) for x in data]


def corpus():
    """[(name, stream, want)]: the hand-built streams, each with the `want` it was made for, one less and three more."""
    rng = np.random.default_rng(5)
    made = []

    def add(name, blocks, plain, pad=0, wants=None, cut=None, **kw):
        sink = dw.BitSink()
        for b in blocks:
            b(sink)
        s = dw.zlib_stream(sink.getvalue(pad), plain, **kw)
        if cut is not None:
            s = s[:cut] if cut >= 0 else s[:len(s) + cut]
        made.append((name, s, wants, len(plain)))

    def stored(data, **kw):
        return lambda sink: dw.stored_block(sink, data, **kw)

    def fixed(symbols, **kw):
        return lambda sink: dw.fixed_block(sink, symbols, **kw)

    def dynamic(symbols, **kw):
        return lambda sink: dw.dynamic_block(sink, symbols, **kw)

    def raw_bits(v, n):
        return lambda sink: sink.put(v, n)

    text = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    big = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    # ---- stored blocks
    add("stored-0", [stored(b"", final=True)], b"")
    add("stored-0-then-data", [stored(b""), stored(b""), stored(b"abc", final=True)], b"abc")
    add("stored-65535", [stored(big, final=True)], big)
    add("stored-row", [stored(text[:100]), stored(text[100:101]), stored(text[101:], final=True)], text)
    add("stored-padding", [stored(text, final=True, pad=0b11111)], text)
    add("stored-nlen", [stored(text, final=True, nlen=0x1234)], text)
    add("stored-cut", [stored(text, final=True)], text, cut=-40)
    # ---- fixed blocks, lengths and distances
    mixed = lits(b"abcabcabd") + [("copy", 10, 1), ("copy", 11, 2), ("copy", 13, 3), ("copy", 3, 9)] + lits(text[:40]) + [("copy", 30, 40)]
    add("fixed", [fixed(mixed, final=True)], dw.plaintext(mixed))
    both258 = lits(b"xy") + [("copy", 258, 1), ("copy", 258, 2, "284+31"), ("copy", 258, 300), ("copy", 257, 258)]
    add("len-258", [fixed(both258, final=True)], dw.plaintext(both258))
    window = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    far = [("copy", 258, 32768), ("copy", 5, 32768), ("copy", 100, 32767)]
    add("dist-32768", [stored(window), fixed(far, final=True)], window + dw.plaintext(far, window))
    add("dist-too-far", [fixed(lits(b"ab") + [("copy", 3, 3)], final=True)], b"ab", wants=[2, 3, 9])  # full at 2: "past"
    add("dist-too-far-later", [stored(text), fixed([("copy", 3, 301)], final=True)], text, wants=[len(text), len(text) + 1, len(text) + 9])
    # ---- batches of records: one fewer, exactly one, one more; matches whose sources lie in the batch before and across it
    for n in (model.BATCH - 1, model.BATCH, model.BATCH + 1):
        syms = lits((text * 2)[:n])
        add(f"batch-{n}", [fixed(syms, final=True)], dw.plaintext(syms))
        syms = lits((text * 2)[:n - 1]) + [("copy", 100, 200), ("copy", 50, 120), ("copy", 258, 1)] + lits(b"end")
        add(f"batch-{n}-copies", [fixed(syms, final=True)], dw.plaintext(syms))
    # ---- dynamic blocks
    many = lits(bytes(range(40)) * 3 + text) + [("copy", 20, 7), ("copy", 90, 300), ("copy", 4, 400)]
    add("dynamic", [dynamic(many, final=True)], dw.plaintext(many))
    add("dynamic-15-bit", [dynamic(many, final=True, skew=True, d_skew=False)], dw.plaintext(many))
    spread = lits(text) + [("copy", 5, d) for d in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 300, 290)]
    add("dynamic-15-bit-distances", [dynamic(spread, final=True, skew=True, d_skew=True)], dw.plaintext(spread))
    one = lits(b"abcdefgh") + [("copy", 4, 5), ("copy", 9, 6), ("copy", 3, 5)]
    add("dynamic-one-distance-code", [dynamic(one, final=True)], dw.plaintext(one))
    add("dynamic-no-distance-codes", [dynamic(lits(text[:90]), final=True)], text[:90])
    add("dynamic-untrimmed", [dynamic(many, final=True, trim=False)], dw.plaintext(many))
    add("dynamic-hlit", [dynamic(lits(b"abc"), final=True, hlit=30)], b"abc")
    add("dynamic-hdist", [dynamic(lits(b"abc"), final=True, hdist=30)], b"abc")
    add("dynamic-cl-incomplete", [dynamic(lits(b"abc"), final=True, cl_lens=[2, 2, 2] + [0] * 16, cl_syms=[(0, 0)] * 259)], b"abc")
    add("dynamic-repeat-first", [dynamic(lits(b"abc"), final=True, cl_syms=[(16, 0)] + [(1, 0)] * 260)], b"abc")
    add("dynamic-repeat-past", [dynamic(lits(b"abc"), final=True, hlit=0, hdist=0, cl_syms=[(8, 0)] * 250 + [(18, 127)])], b"abc")
    add("dynamic-no-eob", [dynamic(lits(b"\0\1\0"), final=True, ll_lens=[1, 1] + [0] * 284, eob=False)], b"\0\1\0")
    add("dynamic-over", [dynamic([], final=True, ll_lens=[1, 1] + [0] * 254 + [1], eob=False)], b"")
    add("dynamic-incomplete-distances", [dynamic(lits(b"abc"), final=True, d_lens=[2, 2] + [0] * 28)], b"abc")
    # ---- symbols without a meaning
    add("length-286", [fixed(lits(b"ab") + [("raw", 286, 0, 0)], final=True)], b"ab")
    add("distance-30", [fixed(lits(b"ab") + [("raw", 257, 0, 0), ("rawdist", 30, 0, 0)], final=True)], b"ab")
    # ---- several blocks, a last block that is not final
    later = [("copy", 40, 300), ("copy", 7, 340)] + lits(b"tail")
    first = window[:300] + dw.plaintext(mixed, window[:300])
    add("three-blocks", [stored(window[:300]), fixed(mixed), dynamic(later + many, final=True)],
        first + dw.plaintext(later + many, first))
    add("not-final", [fixed(mixed)], dw.plaintext(mixed), adler=4)
    add("not-final-stored", [stored(text)], text, adler=4)
    # ---- the zlib header
    body = [fixed(lits(text[:256]) + [("copy", 20, 256)], final=True)]
    plain = text[:256] + text[:20]
    add("cinfo-0-distance-256", body, plain, header=header(0x08))
    add("cm-7", body, plain, header=header(0x77))
    add("cinfo-8", body, plain, header=header(0x88))
    add("check", body, plain, header=b"\x78\x00")
    add("fdict", body, plain, header=header(0x78, True))
    add("fdict-cut", body, plain, header=header(0x78, True), cut=5)
    add("raw-deflate", body, plain, header=b"")
    add("one-byte", body, plain, cut=1)
    add("header-only", body, plain, cut=2)
    # ---- the trailer
    add("adler-wrong", body, plain, adler="wrong")
    for k in (1, 2, 3, 4):
        add(f"adler-cut-{k}", body, plain, adler=k)
    add("trailing", body, plain, trailing=b"\xff\x00junk")
    add("adler-wrong-trailing", body, plain, adler="wrong", trailing=b"junk")
    # ---- after the chunk is full: `wants` is the plain text of the first block alone
    full = [len(text)]
    head = fixed(lits(text))
    add("after-empty-blocks", [head, stored(b""), fixed([]), dynamic([]), stored(b"", final=True)], text, wants=full)
    add("after-type-3", [head, raw_bits(0b110, 3)], text, wants=full, adler=4)
    add("after-nlen", [head, stored(b"", nlen=5)], text, wants=full, adler=4)
    add("after-hlit", [head, dynamic([], hlit=30)], text, wants=full, adler=4)
    add("after-literal", [head, fixed(lits(b"x"), final=True)], text + b"x", wants=full)
    add("after-literal-last-byte", [head, fixed(lits(b"x"), eob=False)], text, wants=full, adler=4)
    add("after-literal-and-a-byte", [head, fixed(lits(b"x"), eob=False)], text, wants=full, adler=4, trailing=b"\0")
    add("after-copy", [head, fixed([("copy", 3, 1)], final=True)], text + text[-1:] * 3, wants=full)
    add("after-copy-too-far", [head, fixed([("copy", 3, 400)], final=True)], text, wants=full)
    add("after-copy-last-byte", [head, fixed([("copy", 3, 1)], eob=False)], text, wants=full, adler=4)
    add("after-length-286", [head, fixed([("raw", 286, 0, 0)], final=True)], text, wants=full)
    add("after-distance-31", [head, fixed([("raw", 257, 0, 0), ("rawdist", 31, 0, 0)], final=True)], text, wants=full)
    add("after-stored-byte", [head, stored(b"x", final=True)], text + b"x", wants=full)
    add("after-stored-byte-missing", [head, stored(b"x", final=True)], text + b"x", wants=full, cut=-5)
    add("copy-over-the-end", [fixed(lits(text) + [("copy", 10, 5)], final=True)], text + (text[-5:] * 2), wants=[len(text) + 4])
    add("copy-over-the-end-last-byte", [fixed(lits(text) + [("copy", 10, 5)], eob=False)], text, wants=[len(text) + 4], adler=4)
    cases = []
    for name, s, wants, n in made:
        for w in wants or sorted({n, max(n - 1, 1), n + 3}):
            cases.append((name, s, max(w, 1)))
    return cases


def fuzz_bases():
    """Valid streams to mutate: zlib's own at several levels, and hand-built ones with every block type."""
    rng = np.random.default_rng(11)
    pays = [rng.integers(0, 256, 200, dtype=np.uint8).tobytes(), bytes(500), (np.arange(900) // 3 % 7).astype(np.uint8).tobytes(),
            rng.integers(0, 4, 1200, dtype=np.uint8).tobytes(), b"\x05", (bytes(range(64)) * 9)[:570]]
    out = []
    for i, p in enumerate(pays):
        out.append((zlib.compress(p, (0, 1, 6, 9)[i % 4]), len(p)))
        co = zlib.compressobj(6, zlib.DEFLATED, 9 + i % 7)
        half = len(p) // 2
        out.append((co.compress(p[:half]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(p[half:]) + co.flush(), len(p)))
    keep = ("fixed", "len-258", "dynamic", "dynamic-15-bit-distances", "dynamic-one-distance-code", "three-blocks", "stored-row",
            "after-empty-blocks", "batch-257-copies")
    seen = set()
    for name, s, want in corpus():
        if name in keep and name not in seen and chunk_outcome(s, want)[0] == "bytes":
            seen.add(name)
            out.append((s, want))
    assert seen == set(keep)
    return out


def fuzz():
    """[(kind, stream, want)], the kinds in turn so that any prefix holds all of them: bit flips anywhere, cuts (every byte
    of the short streams, then random ones), a changed want, and damage that zlib does not look at (behind the end of the
    stream, or a trailer cut short)."""
    rng = np.random.default_rng(20260)
    bases = fuzz_bases()
    for s, n in bases:
        assert chunk_outcome(s, n)[0] == "bytes"
    cuts = [(s[:c], n) for s, n in bases if len(s) <= 140 for c in range(len(s))]
    kinds = {"flip": [], "cut": [], "want": [], "blind": []}
    for it in range(700):
        s, n = bases[it % len(bases)]
        bad = bytearray(s)
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        kinds["flip"].append((bytes(bad), n))
        if it < len(cuts):
            kinds["cut"].append(cuts[(it * 37) % len(cuts)])
        else:
            kinds["cut"].append((s[:int(rng.integers(0, len(s) + 1))], n))
        kinds["want"].append((s, max(1, n + int(rng.integers(-3, 4)))))
        junk = rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8).tobytes()
        blind = s[:len(s) - int(rng.integers(1, 5))] if it % 2 else s + junk
        kinds["blind"].append((blind, n))
    out = []
    for it in range(700):
        for kind in ("flip", "cut", "want", "blind"):
            out.append((kind,) + kinds[kind][it])
    return out


def agree(name, stream, want):
    """The corpus rule: the same bytes, or a refusal of the same kind (short: with the same two numbers)."""
    ref = chunk_outcome(stream, want)
    got = model.outcome(stream, want)
    assert got == ref, (name, want, stream.hex()[:120], got[:1] + got[1:][:2] if got[0] != "bytes" else "bytes", ref[0])
    return ref[0]


def test_model_equals_zlib_on_hand_built_streams():
    every = {}
    for name, stream, want in corpus():
        every.setdefault(name, []).append(agree(name, stream, want))
    # at the `want` the stream was made for: the last but one of a name's cases, or its only one
    seen = {name: {kinds[-2] if len(kinds) > 1 else kinds[0]} for name, kinds in every.items()}
    assert sum(len(k) for k in every.values()) > 150 and {x for k in every.values() for x in k} == {"bytes", "corrupt", "past", "short"}
    assert "bytes" in seen["cinfo-0-distance-256"] and "bytes" in seen["dist-32768"] and "bytes" in seen["stored-65535"]
    assert "bytes" in seen["dynamic-15-bit"] and "bytes" in seen["dynamic-one-distance-code"] and "bytes" in seen["len-258"]
    assert "bytes" in seen["not-final"] and "bytes" in seen["adler-cut-4"] and "bytes" in seen["trailing"]
    for name in ("cm-7", "cinfo-8", "check", "fdict", "raw-deflate", "adler-wrong", "stored-nlen", "dist-too-far", "dist-too-far-later", "dynamic-hlit",
                 "dynamic-hdist", "dynamic-cl-incomplete", "dynamic-repeat-first", "dynamic-repeat-past", "dynamic-no-eob",
                 "dynamic-over", "dynamic-incomplete-distances", "length-286", "distance-30", "after-type-3", "after-nlen",
                 "after-hlit", "after-length-286", "after-distance-31", "adler-wrong-trailing"):
        assert seen[name] == {"corrupt"}, (name, seen[name])
    for name in ("after-literal", "after-copy", "after-copy-too-far", "after-stored-byte", "copy-over-the-end",
                 "after-literal-and-a-byte"):
        assert seen[name] == {"past"}, (name, seen[name])
    for name in ("after-empty-blocks", "after-literal-last-byte", "after-copy-last-byte", "after-stored-byte-missing",
                 "copy-over-the-end-last-byte"):
        assert seen[name] == {"bytes"}, (name, seen[name])
    assert every["dist-too-far"] == ["past", "corrupt", "corrupt"] and every["dist-too-far-later"] == ["past", "corrupt", "corrupt"]
    assert seen["fdict-cut"] == {"short"} and seen["header-only"] == {"short"} and seen["stored-0"] == {"short"}


def test_model_equals_zlib_on_mutated_streams():
    cases = fuzz()
    assert len(cases) >= 2000
    counts = {}
    for kind, stream, want in cases:
        ref = agree(kind, stream, want)
        counts[ref] = counts.get(ref, 0) + 1
    accepted = counts.get("bytes", 0)
    assert accepted >= len(cases) // 4 and len(cases) - accepted >= len(cases) // 4, counts
    assert counts.get("corrupt", 0) >= 200 and counts.get("past", 0) >= 50 and counts.get("short", 0) >= 200, counts
    head = [chunk_outcome(s, w)[0] for _k, s, w in cases[:300]]                # what test_gpu_tiff_deflate.py sends to the kernel
    assert head.count("bytes") >= 75 and 300 - head.count("bytes") >= 75


def test_model_reads_the_strips_pillow_and_write_tiff_make():
    rgb = sample(np.uint8, 40, 50, 3)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="TIFF", compression="tiff_adobe_deflate")
    for blob in (buf.getvalue(), tc.written(sample(np.uint16, 37, 53, 3), deflate=True, rows_per_strip=7, predictor=True)):
        tags = tiffio._read_ifd(memoryview(blob), "<")
        assert tags[tiffio.COMPRESSION][0] == 8
        for o, c in zip(tags[tiffio.STRIP_OFFSETS], tags[tiffio.STRIP_BYTE_COUNTS]):
            data = zlib.decompress(blob[o:o + c])
            assert model.outcome(blob[o:o + c], len(data)) == ("bytes", data)


# ---- the parser --------------------------------------------------------------------------------------------------------
def deflate_twins():
    """(name, Deflate file, the same picture and layout as an LZW file)."""
    out = []
    for dtype in (np.uint8, np.uint16):
        for layout in ({}, {"rows_per_strip": 7}, {"tile": (16, 16)}, {"tile": (32, 48)}):
            a = sample(dtype, 37, 53, 3)
            kw = dict(layout, byteorder=">" if dtype is np.uint16 else "<", planar=2 if "tile" in layout else 1, predictor=True)
            out.append((f"{dtype.__name__}{layout}", tc.written(a, deflate=True, **kw), tc.lzw_tiff(a, **kw)))
    return out


def test_tiff_info_with_deflate():
    for name, blob in files_of_every_kind():
        try:
            plain = api.tiff_info(blob)
        except ValueError:
            with pytest.raises(ValueError):
                api.tiff_info(blob, deflate=True)
            continue
        opted = api.tiff_info(blob, deflate=True)
        if plain["compression"] in (8, 32946):
            assert not plain["supported"] and "Deflate" in plain["reason"], name             # the default has not moved
            assert opted["supported"] and opted["reason"] is None, (name, opted)
            want = tiffio.read_tiff(blob)
            assert (opted["dtype"], opted["shape"]) == (want.dtype, want.shape)
        else:
            assert opted == plain, name
    geometry = ("width", "height", "samples", "bits", "predictor", "planar", "big_endian", "photometric", "extra_samples", "tiled",
                "chunk_w", "chunk_h", "chunks", "dtype", "shape")
    for name, z, lzw in deflate_twins():
        a, b = api.tiff_info(z, deflate=True), api.tiff_info(lzw)
        assert a["compression"] == 8 and a["supported"] and b["supported"]
        assert {k: a[k] for k in geometry} == {k: b[k] for k in geometry}, name
    # compression 32946, the tag's older number
    blob = with_compression(tc.written(sample(np.uint8, 10, 12, 3), deflate=True), 32946)
    assert api.tiff_info(blob, deflate=True)["compression"] == 32946
    assert api.tiff_info(blob, deflate=True)["supported"] and not api.tiff_info(blob)["supported"]
    assert np.array_equal(tiffio.read_tiff(blob), sample(np.uint8, 10, 12, 3))
    # the chunk table is the one the directory holds
    z = deflate_twins()[1][1]
    tags = tiffio._read_ifd(memoryview(z), "<")
    arr = np.frombuffer(z, dtype=np.uint8)
    info, table = _ffi.TiffInfo.array(), np.zeros(2 * len(tags[tiffio.STRIP_OFFSETS]), dtype=np.int64)
    assert _ffi.load().lars_tiff_info_deflate(_ffi.ptr(arr), arr.size, info, _ffi.ptr(table), table.size // 2) == 0
    assert table[0::2].tolist() == list(tags[tiffio.STRIP_OFFSETS]) and table[1::2].tolist() == list(tags[tiffio.STRIP_BYTE_COUNTS])


def test_new_entries_are_declared_everywhere():
    text = open(os.path.join(os.path.dirname(_ffi.__file__), "..", "include", "lars_hip.h")).read()
    for name in ("lars_tiff_info_deflate", "lars_h_decode_tiff_deflate", "lars_h_thumbnail_tiff_deflate_u8"):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name) and name + "(" in text
    assert _ffi.SIGNATURES["lars_tiff_info_deflate"] == _ffi.SIGNATURES["lars_tiff_info"]
    assert _ffi.SIGNATURES["lars_h_decode_tiff_deflate"] == _ffi.SIGNATURES["lars_h_decode_tiff"]
    assert _ffi.SIGNATURES["lars_h_thumbnail_tiff_deflate_u8"] == _ffi.SIGNATURES["lars_h_thumbnail_tiff_u8"]
    assert "LARS_TIFD_PAST = 3" in text and "LARS_TIFD_SHORT = 2" in text and "LARS_TIFD_CORRUPT = 1" in text


def test_parser_with_deflate_under_address_and_ub_sanitizers(asan_bin, tmp_path):  # noqa: F811
    """The sanitizer driver's kind 7 (lars_tiff_info_deflate) over the inputs test_parser_under_address_and_ub_sanitizers gives
    kind 6: no report, and the shipped library's answers."""
    rng = np.random.default_rng(1)
    cases = []
    for _name, blob in files_of_every_kind():
        cases += [(64, blob), (0, blob)]
        for cut in sorted({0, 1, 2, 7, 8, 9, len(blob) - 1, len(blob) // 2, *rng.integers(0, len(blob), 12).tolist()}):
            cases.append((64, blob[:cut]))
        for _ in range(6):
            bad = bytearray(blob)
            ifd = struct.unpack_from("<I" if blob[:2] == b"II" else ">I", blob, 4)[0]
            bad[int(rng.integers(min(ifd, len(bad) - 1), len(bad)))] = int(rng.integers(0, 256))
            cases.append((3, bytes(bad)))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for a, data in cases:
            fh.write(struct.pack("<4I", 7, a, 0, len(data)) + data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([asan_bin, str(path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == f"done {len(cases)} cases"
    lib = _ffi.load()
    supported = 0
    for i, ((a, data), line) in enumerate(zip(cases, lines)):
        words = dict(w.split("=") for w in line.split()[2:])
        arr = np.frombuffer(data or b"\0", dtype=np.uint8)
        info = _ffi.TiffInfo.array()
        table = np.zeros(a * 2 + 1, dtype=np.int64)
        rc = lib.lars_tiff_info_deflate(_ffi.ptr(arr), len(data), info, _ffi.ptr(table) if a else None, a)
        assert int(words["rc"]) == rc, (i, line)
        if rc == 0:
            assert int(words["h"], 16) == fnv(bytes(info)) and int(words["t"], 16) == fnv(table[:a * 2].tobytes()), (i, line)
            supported += _ffi.TiffInfo(*info).supported and _ffi.TiffInfo(*info).compression == 8
    assert supported >= 4


# ---- the Python side, without a device -----------------------------------------------------------------------------------
def test_decode_tiff_with_deflate_reaches_the_library(monkeypatch):
    """deflate=True gets past the refusal and asks the library for the new entry point; without the flag nothing has moved."""
    asked = []

    def library(name, *args):
        asked.append(name)
        raise _ffi.LarsError(-1, "no device in this test")

    monkeypatch.setattr(_ffi, "call", library)
    blob = tc.written(sample(np.uint8, 10, 12, 3), deflate=True)
    with pytest.raises(tiffio.TiffError, match="no device in this test"):
        api.decode_tiff(blob, deflate=True)
    assert asked == ["lars_h_decode_tiff_deflate"]
    big = tc.written(sample(np.uint8, 300, 500, 3), deflate=True)
    with pytest.raises((tiffio.TiffError, ValueError), match="no device in this test"):
        api.thumbnail_tiff(big, (100, 100), deflate=True)
    assert asked[-1] == "lars_h_thumbnail_tiff_deflate_u8" and len(asked) == 2
    with pytest.raises(NotImplementedError, match="Deflate"):
        api.decode_tiff(blob)
    with pytest.raises(NotImplementedError, match="Deflate"):
        api.decode_tiff(blob, deflate=False)
    with pytest.raises(NotImplementedError, match="Deflate"):
        api.thumbnail_tiff(big, (100, 100))
    assert len(asked) == 2
    lzw = tc.lzw_tiff(sample(np.uint8, 10, 12, 3))
    with pytest.raises(tiffio.TiffError):
        api.decode_tiff(lzw, deflate=True)                  # an LZW file with the flag: the new entry reads it as the old one does
    assert asked[-1] == "lars_h_decode_tiff_deflate"
    with pytest.raises(NotImplementedError, match="PackBits"):
        buf = io.BytesIO()
        Image.fromarray(sample(np.uint8, 10, 12, 3)).save(buf, format="TIFF", compression="packbits")
        api.decode_tiff(buf.getvalue(), deflate=True)


def test_read_image_routes_deflate_files_on_request(tmp_path, monkeypatch):
    from lars_image_processing_amd import driver
    a16 = sample(np.uint16, 45, 67, 3)
    rgb = sample(np.uint8, 30, 40, 3)
    (tmp_path / "z16.tif").write_bytes(tc.written(a16, deflate=True, predictor=True))
    (tmp_path / "z8.tiff").write_bytes(tc.written(rgb, deflate=True))
    (tmp_path / "lzw.tif").write_bytes(tc.lzw_tiff(a16))
    calls = []

    def stub(data, **kw):
        calls.append(kw)
        return tiffio.read_tiff(bytes(data))

    monkeypatch.setattr(api, "decode_tiff", stub)
    for name, full, want in (("z16.tif", True, a16), ("z8.tiff", False, rgb), ("lzw.tif", True, a16)):
        got = tiffio.read_image(tmp_path / name, full_depth=full, tiff_decoder="device+deflate")
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert calls == [{"deflate": True}] * 3
    del calls[:]
    for name, full, want in (("z16.tif", True, a16), ("z8.tiff", False, rgb)):
        got = tiffio.read_image(tmp_path / name, full_depth=full, tiff_decoder="device")
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert calls == []                                       # "device" still leaves Deflate files to the host
    tiffio.read_image(tmp_path / "lzw.tif", full_depth=True, tiff_decoder="device")
    assert calls == [{}]                                     # and calls decode_tiff as it always did
    for bad in ("device+", "deflate", "gpu", "Device+Deflate", ""):
        with pytest.raises(ValueError, match="tiff_decoder"):
            tiffio.read_image(tmp_path / "z8.tiff", tiff_decoder=bad)
    assert driver.TIFF_DECODERS == ("pillow", "device", "device+deflate")
