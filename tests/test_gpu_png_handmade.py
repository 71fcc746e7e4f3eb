"""decode_png on hand-built deflate streams (tests/deflate_writer.py, the table of tests/png_handmade_cases.py): what zlib's own
deflate never writes.  Every case has passed the model of the kernels in tests/test_png_handmade_cpu.py, which imports the same
table.  Valid streams equal Pillow and the writer's plaintext byte for byte; invalid ones raise ValueError with the message of
the status zlib's own verdict maps to, and the next decode on the same thread is right."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_handmade_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu


def pillow(b):
    return np.asarray(Image.open(io.BytesIO(b)))


@pytest.mark.parametrize("name", C.VALID)
def test_valid_stream_equals_pillow_and_the_plaintext(name):
    c = C.case(name)
    b = C.png_file(c)
    got, ref = lars.decode_png(b), pillow(b)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    assert got.tobytes() == ref.tobytes()
    rows = np.frombuffer(c["plain"][:c["need"]], np.uint8).reshape(c["h"], 1 + c["rb"])
    assert not rows[:, 0].any() and ref.tobytes() == rows[:, 1:].tobytes()
    if c["mode"] in ("L", "RGB", "RGBA") and min(c["w"], c["h"]) >= 32:
        assert np.array_equal(lars.thumbnail_png(b, (24, 24)), lars.thumbnail(got, (24, 24)))


@pytest.mark.parametrize("name", C.INVALID)
def test_invalid_stream_raises_the_mapped_error_and_the_thread_decodes_on(name):
    c = C.case(name)
    accept = {c["differs"][1]} if "differs" in c else C.zlib_says(c["stream"], c["need"])[1]
    with pytest.raises(ValueError, match="|".join(sorted(C.message_of(s) for s in accept))):
        lars.decode_png(C.png_file(c))
    good = C.png_file(C.case(C.GOOD))
    assert lars.decode_png(good).tobytes() == pillow(good).tobytes()
