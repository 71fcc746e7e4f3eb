"""What the GPU tests of the JPEG decoder share (helper, not collected): the comparison with Pillow, the "jpeg_subseq_bits"
fixture and the device entry point called with guard bytes round its output."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi


def want(b):
    return np.asarray(Image.open(io.BytesIO(b)))


def same(b, name=None):
    """decode_jpeg(b) is Pillow's array; ``name`` says in the failure which file of a loop it was."""
    got, ref = lars.decode_jpeg(b), want(b)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, got.shape, ref.dtype, ref.shape)
    assert got.tobytes() == ref.tobytes(), f"{name}: {int((got != ref).sum())} of {ref.size} samples differ"


def get_bits():
    return _ffi.get_tuning("jpeg_subseq_bits")


@pytest.fixture
def subseq_bits():
    """A setter of "jpeg_subseq_bits" for a test; what the knob held before the test comes back after it."""
    with _ffi.tuning(jpeg_subseq_bits=get_bits()):
        yield lambda v: _ffi.set_tuning(jpeg_subseq_bits=v)


def device_entry_point_with_guards(b, ref):
    """lars_d_decode_jpeg_u8 on a caller's stream into the middle of a buffer: the status is clean, the output is ``ref`` and
    the 4096 bytes on either side of it are untouched."""
    info = _ffi.JpegInfo.array()
    file = np.frombuffer(b, np.uint8)
    assert _ffi.load().lars_jpeg_info(_ffi.ptr(file), file.size, info) == 0
    need = _ffi.load().lars_jpeg_decode_scratch_bytes(info)
    assert need > 0
    guard, nbytes = 4096, ref.size
    d_file, d_out, d_scratch, d_status, stream = (C.c_void_p() for _ in range(5))
    _ffi.call("lars_malloc", C.byref(d_file), file.size)
    _ffi.call("lars_malloc", C.byref(d_out), nbytes + 2 * guard)
    _ffi.call("lars_malloc", C.byref(d_scratch), need)
    _ffi.call("lars_malloc", C.byref(d_status), 8)
    _ffi.call("lars_stream_create", C.byref(stream))
    try:
        _ffi.call("lars_memcpy_h2d", d_file, _ffi.ptr(file), file.size)
        _ffi.call("lars_memset", d_out, 0xA5, nbytes + 2 * guard, stream)
        head = np.ascontiguousarray(file[:_ffi.JpegInfo(*info).entropy_offset])       # only the head stays on the host
        _ffi.call("lars_d_decode_jpeg_u8", d_file, _ffi.ptr(head), info, C.c_void_p(d_out.value + guard), d_status, d_scratch, stream)
        _ffi.call("lars_synchronize", stream)
        got = np.empty(nbytes + 2 * guard, np.uint8)
        status = np.empty(2, np.int32)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(got), d_out, got.size)
        _ffi.call("lars_memcpy_d2h", _ffi.ptr(status), d_status, 8)
    finally:
        _ffi.call("lars_stream_destroy", stream)
        for p in (d_file, d_out, d_scratch, d_status):
            _ffi.call("lars_free", p)
    assert status.tolist() == [0, 0]
    assert (got[:guard] == 0xA5).all() and (got[-guard:] == 0xA5).all()
    assert got[guard:-guard].tobytes() == ref.tobytes()
