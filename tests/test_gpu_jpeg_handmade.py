"""decode_jpeg on hand-built JPEG files (tests/jpeg_writer.py, the table of test_jpeg_handmade_cpu.py): what Pillow's own encoder
never writes.  Every array equals Pillow's byte for byte; damage made with the writer is reported as ValueError."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import api

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_model  # noqa: E402
import jpeg_writer as W  # noqa: E402
from jpeg_gpu_common import device_entry_point_with_guards, get_bits, same, subseq_bits, want  # noqa: E402,F401
from test_jpeg_handmade_cpu import BEYOND, HANDMADE, beyond_the_oracle, content, files_of, nblocks  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(HANDMADE))
def test_handmade_file_equals_pillow(name):
    same(HANDMADE[name](), name)


@pytest.mark.parametrize("name", BEYOND)
def test_frames_of_65535_samples_equal_the_model(name):
    """Past libjpeg's 65500 Pillow refuses the file; the model, equal to Pillow on every file of the table, stands in."""
    b = beyond_the_oracle(name)
    got, ref = lars.decode_jpeg(b), jpeg_model.decode(b)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("bits", [32, 33, 61, 1000])
@pytest.mark.parametrize("group", ["huffman", "restart", "fuzz"])
def test_groups_do_not_depend_on_the_subsequence_length(subseq_bits, group, bits):
    """31-bit symbols, one-code tables, two-byte restart intervals and fill bytes with a border every 32, 33, 61 and 1000 bits."""
    subseq_bits(bits)
    assert get_bits() == bits
    for name in files_of(group):
        same(HANDMADE[name](), f"{name} at {bits} bits")


@pytest.mark.parametrize("name", ["frame 420 1 x 65500", "frame 444 65500 x 1", "restart 422 3 fill before RSTn and EOI",
                                  "header 420 fill 2"])
def test_device_entry_point_with_guards_on_thin_frames_and_fill_bytes(name):
    b = HANDMADE[name]()
    device_entry_point_with_guards(b, want(b))


def damaged_files():
    """good file, {name: file}: entropy data wrong in one chosen way each, made with the writer from the same coefficients."""
    w, h, mode, ri = 64, 48, "L", 6
    rng = np.random.default_rng(63)
    coefs = content(rng, w, h, mode, "sparse", dc=40)
    coefs[::4] = 0                                          # flat blocks: a DC difference of 0 is in the table
    coefs[20, W.ZIGZAG[40]] = 3
    hts = W.tables_for(coefs, None, ri, w, h, ac_shape=W.shape_256)
    hts[(0, 0)] = W.huff_from_freq({s: 1 for s in range(12)})   # all-ones prefix free in both tables
    qts = {0: [2] * 64}

    def make(**kw):
        return W.write(w, h, None, coefs, qts, hts, ri=ri, **kw)

    dc, ac = W.huff_codes(hts[(0, 0)]), W.huff_codes(hts[(1, 0)])
    beyond = [dc[0], ac[0xF0], ac[0xF0], ac[0xF0], ac[0xF1], (1, 1)]    # DC, ZRL to 49, then a run of 15: index 64
    return make(), {
        "a code of the free all-ones prefix": make(inject={14: [(0xFFFF, 16)]}),
        "a run that passes coefficient 63 behind ZRLs": make(inject={14: beyond}),
        "one block too many in an interval": make(repeat={15}),
        "one block too few in an interval": make(skip={15}),
        "a restart interval that ends inside a symbol": make(cut={2: 5}),
    }


def test_damage_made_with_the_writer_raises_value_error():
    good, files = damaged_files()
    assert jpeg_model.decode(good).tobytes() == want(good).tobytes()
    for name, b in files.items():
        assert lars.jpeg_info(b)["supported"], name         # the host sees nothing wrong with the structure
        with pytest.raises(ValueError):                     # the sequential decoder on the CPU first: damaged as the name says
            jpeg_model.decode(b)
    for name, b in files.items():                           # each file once
        with pytest.raises(ValueError, match="entropy data"):
            lars.decode_jpeg(b)
        same(good)                                          # and the next good file decodes correctly afterwards


@pytest.mark.parametrize("name,size", [("huffman 444 from statistics huge", (50, 50)), ("frame L 8 x 30000", (400, 16000)),
                                       ("outside 420 dense 1023 in chroma", (20, 20))])
def test_thumbnail_jpeg_on_handmade_files(name, size):
    b = HANDMADE[name]()
    im = Image.open(io.BytesIO(b))
    assert api.jpeg_draft_scale(im.size, size, 2.0) == 1
    im.thumbnail(size, Image.Resampling.LANCZOS, 2.0)
    assert im.decoderconfig in ((), (1, 0))                 # Pillow decoded at full scale too
    got = lars.thumbnail_jpeg(b, size, 2.0)
    assert got.shape == np.asarray(im).shape and got.tobytes() == np.asarray(im).tobytes()
