"""decode_tiff on hand-built LZW streams (tests/lzw_writer.py, the table and the fuzz of tests/tiff_handmade_cases.py): what no
encoder writes, each stream as the only strip of a file.  Every stream has passed the model of k_td_lzw in
tests/test_tiff_handmade_cpu.py, which imports the same table and must pass on a tree before this file is run on it; the streams
under 100 KB of plaintext pass the model's assertions here once more before they are decoded.  Valid streams equal
tiffio.read_tiff and the writer's plaintext byte for byte; the others raise read_tiff's TiffError, and the next decode on the
same thread is right.  Then many streams in one launch, the order of the errors k_td_check reports, and the assembly kernel
at the widths where its 64-lane scan carries."""
import sys
from pathlib import Path

import numpy as np
import pytest

import lars_image_processing_amd as lars

sys.path.insert(0, str(Path(__file__).resolve().parent))
import lzw_writer as lw  # noqa: E402
import tiff_cases as tc  # noqa: E402
import tiff_handmade_cases as C  # noqa: E402
import tiff_lzw_model as model  # noqa: E402
from lars_image_processing_amd import tiffio  # noqa: E402

pytestmark = pytest.mark.gpu

MODEL_LIMIT = 100_000            # bytes of plaintext up to which the model is asked here as well


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.fixture(scope="module")
def good():
    c = C.case(C.GOOD)
    blob = tc.one_strip_tiff(c["stream"], c["ndst"])
    return blob, tiffio.read_tiff(blob)


def decode_like_read_tiff(blob, good):
    """decode_tiff gives read_tiff's array, or raises its TiffError: with read_tiff's own words where it counts bytes, and as
    corrupt data of the same chunk where the host decoder refuses the stream.  Returns the array or None."""
    try:
        want = tiffio.read_tiff(blob)
    except tiffio.TiffError as e:
        with pytest.raises(tiffio.TiffError) as got:
            lars.decode_tiff(blob)
        if "expected" in str(e):
            assert str(e) in str(got.value)                                  # "strip / tile holds N bytes, M expected"
        else:
            assert "corrupt" in str(e) and "corrupt LZW data in chunk" in str(got.value)
        same(lars.decode_tiff(good[0]), good[1])                             # the status was reset, the workspace is intact
        return None
    got = lars.decode_tiff(blob)
    same(got, want)
    return got


def run(c, good):
    stream, ndst = c["stream"], c["ndst"]
    if ndst <= MODEL_LIMIT:
        bytes_, bad = model.decode(stream, ndst)                             # its assertions first: nothing else goes to the device
    else:
        bytes_, bad = tc.host_lzw(stream, ndst)
    got = decode_like_read_tiff(tc.one_strip_tiff(stream, ndst), good)
    assert (got is None) == (bool(bad) or len(bytes_) < ndst)
    if got is not None:
        assert got.shape == (1, ndst) and got.tobytes() == bytes_
        if "plain" in c:
            assert got.tobytes() == c["plain"][:ndst]


@pytest.mark.parametrize("name", C.VALID + C.INVALID)
def test_table_case_equals_read_tiff(name, good):
    run(C.case(name), good)


@pytest.mark.parametrize("name", [n for n in C.SLOW if "zero chain" not in n])
def test_strings_of_half_a_stage(name, good):
    run(C.case(name), good)


def test_the_longest_string(good):
    """The zero chain to 3839 bytes: 7.4 MB from one wave, most of it copied byte by byte by one lane.  Gated by the CPU test."""
    (name,) = [n for n in C.SLOW if "zero chain" in n]
    c = C.case(name)
    assert c["ndst"] > 7_000_000
    run(c, good)


@pytest.mark.parametrize("part", range(4))
def test_seeded_fuzz_equals_read_tiff(part, good):
    raised = decoded = 0
    for k, (kind, stream, ndst, plain) in enumerate(C.fuzz_cases()):
        if k // 4 % 4 != part or C.old_style(stream):              # the kind is k % 4: every part has every kind
            continue
        try:
            run(dict(stream=stream, ndst=ndst, **({} if plain is None else {"plain": plain})), good)
        except AssertionError as e:
            raise AssertionError(f"stream {k} ({kind}, {len(stream)} bytes, ndst {ndst}): {e}") from e
        bad = tc.host_lzw(stream, ndst)
        raised += bool(bad[1]) or len(bad[0]) < ndst
        decoded += not (bad[1] or len(bad[0]) < ndst)
    print(f"fuzz on the device, part {part}: {decoded} decoded, {raised} raised")
    assert decoded >= 100 and raised >= 200


# ---- many streams in one launch, and which error is reported ---------------------------------------------------------
NDST = 777


def equal_streams(count, seed):
    """``count`` valid non-greedy streams that each fill a chunk of NDST bytes (the last code is clipped), with their rows."""
    rng = np.random.default_rng(seed)
    streams, rows = [], []
    for k in range(count):
        w = lw.Writer(leading_clear=k % 5 != 0)
        if not w.codes:
            w.lit(int(rng.integers(2, 256)))
        while w.n < NDST:
            w.random(rng, 1, p_clear=(0, 0.01, 0.1)[k % 3], literals=(3, 256)[k % 2])
        if k % 4:
            w.eoi()
        streams.append(w.stream())
        rows.append(w.plain()[:NDST])
    return streams, rows


def strips_tiff(streams):
    return tc.build_tiff({256: [NDST], 257: [len(streams)], 258: [8], 259: [5], 262: [1], 277: [1], 278: [1]}, streams)


def test_three_hundred_streams_in_one_launch(good):
    streams, rows = equal_streams(300, 11)
    for s, r in zip(streams, rows):
        assert model.decode(s, NDST) == (r, 0)
    got = decode_like_read_tiff(strips_tiff(streams), good)
    assert got is not None and got.shape == (300, NDST) and got.tobytes() == b"".join(rows)


def test_first_corrupt_strip_else_first_short_strip(good):
    """k_td_check: the first strip the host decoder would refuse, else the first that gave too few bytes."""
    streams, _rows = equal_streams(8, 12)
    short = lw.pack(lw.unpack(streams[1])[:20] + [lw.EOI])
    shorter = lw.pack(lw.unpack(streams[2])[:9] + [lw.EOI])
    corrupt = lw.pack(lw.unpack(streams[3])[:30] + [lw.FIRST + 200, 1, 2, lw.EOI])
    n_short, n_shorter = len(tc.host_lzw(short, NDST)[0]), len(tc.host_lzw(shorter, NDST)[0])
    assert 0 < n_shorter < n_short < NDST and tc.host_lzw(corrupt, NDST)[1] == 1
    for s in (short, shorter, corrupt):
        model.decode(s, NDST)

    def error_of(put):
        files = list(streams)
        for at, s in put.items():
            files[at] = s
        blob = strips_tiff(files)
        with pytest.raises(tiffio.TiffError) as want:
            tiffio.read_tiff(blob)
        with pytest.raises(tiffio.TiffError) as got:
            lars.decode_tiff(blob)
        same(lars.decode_tiff(good[0]), good[1])
        return str(want.value), str(got.value)

    want, got = error_of({2: short, 5: corrupt})                 # a short strip, a corrupt one at a higher index: corrupt wins
    assert "corrupt LZW data in chunk 5" in want and "corrupt LZW data in chunk 5" in got
    want, got = error_of({2: corrupt, 5: short})
    assert "corrupt LZW data in chunk 2" in want and "corrupt LZW data in chunk 2" in got
    want, got = error_of({1: short, 6: shorter})                 # two short strips: the first, with its own count
    assert want == f"strip / tile holds {n_short} bytes, {NDST} expected" and want in got
    want, got = error_of({1: shorter, 6: short})
    assert want == f"strip / tile holds {n_shorter} bytes, {NDST} expected" and want in got
    _want, got = error_of({3: corrupt, 7: corrupt, 0: short})    # two corrupt strips: the host's threads name either, the device the first
    assert "corrupt LZW data in chunk 3" in got


# ---- row assembly ----------------------------------------------------------------------------------------------------
WIDTHS = (1, 63, 64, 65, 127, 128, 129)
LAYOUTS = ({"rows_per_strip": 3}, {"tile": (16, 64)}, {"tile": (16, 128)})


def wrapping(rng, dtype, h, w, c):
    """Samples whose differences along a row are large: the predictor's running sums wrap many times in every row."""
    top = np.iinfo(dtype).max + 1
    step = rng.integers(top // 2 - top // 8, top - 1, (h, w, c), dtype=np.int64)
    a = (np.cumsum(step, axis=1) + rng.integers(0, top, (h, 1, c))) % top
    a[:, ::7] = rng.integers(0, top, a[:, ::7].shape)
    a = a.astype(dtype)
    return a[..., 0] if c == 1 else a


@pytest.mark.parametrize("lzw", [True, False], ids=["lzw", "raw"])
@pytest.mark.parametrize("dtype,byteorder", [(np.uint8, "<"), (np.uint8, ">"), (np.uint16, "<"), (np.uint16, ">")])
def test_predictor_scan_at_the_lane_boundaries(dtype, byteorder, lzw):
    """Predictor 2 at widths around one and two waves: chunky with 1 to 3 samples and planar, strips, and tiles of 64 and 128
    columns, whose last column is one pixel wide at widths 65 and 129."""
    rng = np.random.default_rng(41)
    for w in WIDTHS:
        for c, planar in ((1, 1), (2, 1), (3, 1), (3, 2)):
            for layout in LAYOUTS:
                a = wrapping(rng, dtype, 5, w, c)
                kw = dict(layout, byteorder=byteorder, planar=planar, predictor=True)
                blob = tc.lzw_tiff(a, **kw) if lzw else tc.written(a, **kw)
                got = lars.decode_tiff(blob)
                same(got, tiffio.read_tiff(blob))
                same(got, a)
    info = lars.tiff_info(tc.written(wrapping(rng, dtype, 5, 129, 3), tile=(16, 128), predictor=True))
    assert (info["chunk_w"], info["chunks"], info["predictor"]) == (128, 2, 2)


@pytest.mark.parametrize("lzw", [True, False], ids=["lzw", "raw"])
def test_assembly_grid_takes_a_second_step(lzw):
    """70 000 rows of one pixel in 4 planes: 280 000 row units for a grid capped at 65 536 blocks of 4 waves."""
    rng = np.random.default_rng(43)
    a = rng.integers(0, 65536, (70000, 1, 4)).astype(np.uint16)          # a row of one pixel: nothing for the predictor to add
    kw = dict(planar=2, predictor=True, byteorder=">")
    blob = tc.lzw_tiff(a, **kw) if lzw else tc.written(a, **kw)
    info = lars.tiff_info(blob)
    assert info["chunks"] == 4 and info["shape"] == (70000, 1, 4)
    got = lars.decode_tiff(blob)
    same(got, tiffio.read_tiff(blob))
    same(got, a)
