"""The three device encoders on the inputs of tests/encoder_hard_cases.py, which are built to reach what ordinary pictures
never do: probe sequences of the TIFF encoder's hash table that go on for dozens of steps, wrap round its end and find their
match or their empty slot deep in a cluster; Huffman code lengths that the PNG encoder has to limit to 15 and to 7 bits, and
every form of the run-length coded header; the largest DC differences, ZRL runs, blocks without EOB and a stuffed last byte in
the JPEG encoder.  The references are the ones of the encoders' own test files: lzw_writer and Pillow's (libtiff's) strips,
zlib through check_png, Pillow's file byte for byte.  tests/test_encoders_hard_cpu.py shows on the CPU that every case reaches
its path and passes its kernel's model with every index in range; the conditions are asserted again here through the models."""
import numpy as np
import pytest

import lars_image_processing_amd as lars
from lars_image_processing_amd import api, tiffio

import encoder_hard_cases as hc
import lzw_writer as lz
import png_encode_model as pm
import tiff_encode_model as tm
from test_encoders_hard_cpu import (JPEG_NAMES, PNG_NAMES, TIFF_NAMES, boundary_lengths, code_length_histogram, pillow_pictures, png_segments,
                                    raw_strips, tiff_events)
from test_gpu_jpeg_encode import device_entry_point_with_guards, same
from test_gpu_tiff_encode import check
from test_png_cpu import check_png, parse_chunks
from test_tiff_encode_cpu import RANDOM, directory

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# TIFF
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TIFF_NAMES)
def test_tiff_strips_that_cluster(name):
    ev = tiff_events(name)                                     # the model: equal to the greedy encoder, every index in range
    assert ev["max_steps"] >= 4 and ev["insert_step"] >= 3
    _blob, (codes,) = check(hc.one_strip(hc.tiff_cases()[name]))
    assert codes.count(lz.CLEAR) == 1 + ev["clears"]


def test_tiff_cases_reach_the_deep_steps():
    evs = [tiff_events(n) for n in TIFF_NAMES]
    assert max(e["max_steps"] for e in evs) >= 32 and max(e["match_step"] for e in evs) >= 2
    assert max(e["insert_step"] for e in evs) >= 2 and max(e["wrap_step"] for e in evs) >= 1


def test_tiff_rows_of_clusters_one_workgroup_each():
    pic = hc.cluster_rows(hc.SEED + 5)
    assert pic.shape[0] >= 8
    check(pic, 1)
    check(pic, 1, True)
    check(pic, 4)                                              # strips of four clusters, the last of one


@pytest.mark.parametrize("which", range(10))
def test_tiff_stream_ends_at_a_width_change_or_the_table_full_clear(which):
    """The last data code on either side of 9 -> 10, 10 -> 11 and 11 -> 12 bits; the end of input in front of the table-full
    Clear, with the code that fills the table (Clear, EOI follow), one literal and two behind it."""
    n = boundary_lengths()[which]
    _blob, (codes,) = check(hc.one_strip(RANDOM[:n]))
    if which < 6:
        assert len(codes) - 2 == (253, 254, 765, 766, 1789, 1790)[which] + 1 and codes.count(lz.CLEAR) == 1
    else:
        assert codes.count(lz.CLEAR) == (1 if which == 6 else 2)
        assert (codes[-2] == lz.CLEAR) == (which == 7)


def test_tiff_strips_equal_pillows():
    """uint8 L and RGB, with and without the predictor, the rows per strip Pillow chose: every strip is libtiff's, byte for byte."""
    seen = 0
    for name, a, predictor in pillow_pictures():
        rows, strips = hc.pillow_strips(a, predictor)
        blob = lars.encode_tiff(a, rows_per_strip=rows, predictor=predictor)
        tags, _ifd = directory(blob)
        assert tags[tiffio.ROWS_PER_STRIP][1] == (rows,), name
        offsets, counts = tags[tiffio.STRIP_OFFSETS][1], tags[tiffio.STRIP_BYTE_COUNTS][1]
        assert len(offsets) == len(strips), name
        for k, (o, n, strip, raw) in enumerate(zip(offsets, counts, strips, raw_strips(a, rows, predictor))):
            assert blob[o:o + n] == strip, (name, k, "lzw_writer agrees with " + ("Pillow" if lz.pack(lz.encode(raw, clear_at=4094)) == strip else "the device"))
            seen += 1
        if a.nbytes < 65536:                                   # at the default strip size the device chooses Pillow's rows itself
            assert lars.encode_tiff(a, predictor=predictor) == blob, name
    assert seen == 4 * len(TIFF_NAMES) + 2 + 2 * 2


# ---------------------------------------------------------------------------------------------------------------------
# PNG
# ---------------------------------------------------------------------------------------------------------------------
def device_segments(blob):
    """The bytes k_png_deflate left per segment (one IDAT chunk each), zlib header and Adler-32 taken off."""
    idat = [d for t, d in parse_chunks(blob) if t == b"IDAT"]
    idat[0] = idat[0][2:]
    idat[-1] = idat[-1][:-4]
    return idat


def first_bits(data, n):
    return int.from_bytes(data[:(n + 7) // 8], "little") & ((1 << n) - 1)


_FILES = {}


def png_file(name):
    """(the device's file, [(header read from it, the model's segment, its info)]); check_png has judged the file."""
    if name not in _FILES:
        pic = hc.png_cases()[name]
        blob = api.encode_png(pic)
        choice = check_png(blob, pic)
        assert np.array_equal(choice, hc.filtered_stream(pic)[1])
        segs = png_segments(name)
        bodies = device_segments(blob)
        assert len(bodies) == len(segs)
        out = []
        for body, (part, last, seg, info, model_body) in zip(bodies, segs):
            head = pm.read_header(body)
            assert head["end"] == seg["hdr_bits"] and first_bits(body, head["end"]) == seg["header"], "the header's bits differ from the model's"
            assert body == model_body, "the segment's bytes differ from the model's"
            assert head["final"] == last and (head["hlit"], head["hdist"]) == (257, 2)
            out.append((head, seg, info))
        _FILES[name] = (blob, out)
    return _FILES[name]


@pytest.mark.parametrize("name", PNG_NAMES)
def test_png_file_is_valid_and_its_header_is_the_models(name):
    _blob, segs = png_file(name)
    for head, seg, _info in segs:
        assert head["lens"] == seg["lens"] and head["runs"] == seg["runs"] and head["clen"] == seg["clen"]
        assert pm.kraft(head["lens"][:257]) == 1 << 15 and sum(1 << (7 - v) for v in head["clen"] if v) == 1 << 7


def test_png_literal_code_limited_to_15_bits():
    _blob, ((head, _seg, info),) = png_file(PNG_NAMES[0])
    assert info["lit_depth"] >= 18                              # what the histogram asks for without the limit (the CPU file: 20)
    assert max(head["lens"][:257]) == 15 and pm.kraft(head["lens"][:257]) == 1 << 15
    _blob, (_first, (head, _seg, info)) = png_file(PNG_NAMES[4])
    assert info["lit_depth"] > 15 and head["final"] == 1 and max(head["lens"][:257]) == 15 and pm.kraft(head["lens"][:257]) == 1 << 15


def test_png_code_length_code_limited_to_7_bits():
    _blob, ((head, _seg, _info),) = png_file(PNG_NAMES[1])
    assert pm.unlimited_depth(code_length_histogram(head["runs"])) >= 8     # from the symbols the device wrote
    assert max(head["clen"]) == 7 and (18, 127) in head["runs"]


def test_png_header_forms():
    forms, hclens = set(), set()
    for name in PNG_NAMES:
        for head, _seg, _info in png_file(name)[1]:
            forms |= {r for r in head["runs"] if r[0] >= 16}
            hclens.add(head["hclen"])
    assert {(16, 0), (16, 1), (16, 2), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)} <= forms
    _blob, ((head, _seg, _info),) = png_file(PNG_NAMES[3])
    assert len(head["runs"]) == 259 and all(s < 16 for s, _ in head["runs"]) and min(head["lens"]) >= 1
    assert hclens == {18, 19}                                  # 18 is the smallest there is: the distance codes' length 1 is the 18th sent


def test_png_decision_between_the_dynamic_block_and_the_stored_form():
    found = hc.boundary_pictures()
    assert sorted(found) == [-1, 0, 1]
    for d, pic in found.items():
        blob = api.encode_png(pic)
        check_png(blob, pic)
        stream, _ = hc.filtered_stream(pic)
        (body,) = device_segments(blob)
        assert body == pm.body_bytes(stream, True), d
        assert (body[0] & 6) == (0 if d > 0 else 4) and len(body) == len(stream) + 5 + min(d, 0)     # BTYPE 0 stored, 2 dynamic


# ---------------------------------------------------------------------------------------------------------------------
# JPEG
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", JPEG_NAMES)
def test_jpeg_files_equal_pillows(name):
    pic, quality = hc.jpeg_cases()[name]
    for mode, sub in hc.MODES:
        a = hc.as_mode(pic, mode)
        if a is not None:
            same(a, quality, sub, name)


@pytest.mark.parametrize("mode, sub", hc.MODES)
def test_jpeg_every_pad_length(mode, sub):
    found = hc.pad_pictures(mode, sub)
    assert sorted(found) == list(range(8))
    for pad, pic in found.items():
        same(hc.as_mode(pic, mode), 50, sub, f"pad {pad}")


def test_jpeg_last_byte_ff_is_stuffed_in_front_of_eoi():
    pic, quality = hc.jpeg_cases()[JPEG_NAMES[5]]
    assert same(pic, quality, "4:4:4")[-4:] == b"\xff\x00\xff\xd9"
    device_entry_point_with_guards(pic, quality, 0)
    device_entry_point_with_guards(np.dstack([pic, pic, pic]), quality, 2)
