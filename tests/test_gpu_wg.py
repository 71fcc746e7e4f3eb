"""The workgroup primitives of csrc/wg_device.h and csrc/checksum_device.h, run directly through the laboratory library
(csrc/lab/wg_check.hip) at sizes the product's pictures do not reach.  Expected values: NumPy and zlib (needs a MI355X)."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "lab"))


@pytest.fixture(scope="module")
def lab():
    import lablib
    assert lablib.available(), "build the laboratory library: make -C lars_image_processing_amd/csrc lab"
    lablib.load()
    return lablib


def run(lab, prim, src, out_dtype, out_count, n, a=0, b=0, in_place=None):
    """src -> device, the primitive, out_count values of out_dtype back (in_place: the output buffer's first contents)."""
    from lars_image_processing_amd import _ffi
    din = _ffi.DeviceBuffer(max(src.nbytes, 8)) if src is not None else None
    if din and src.nbytes:
        din.upload(src)
    dout = _ffi.DeviceBuffer(out_count * np.dtype(out_dtype).itemsize)
    if in_place is not None:
        dout.upload(in_place)
    lab.wg_check(prim, din.ptr if din else None, dout.ptr, n, a, b)
    _ffi.call("lars_synchronize", None)
    got = np.array(dout.download(out_dtype, (out_count,)))
    dout.free()
    if din:
        din.free()
    return got


@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_wg_exscan(lab, threads, dtype):
    top = 1 << 20 if dtype is np.uint32 else 1 << 40            # a shuffle that drops the high word fails the 64-bit cases
    rng = np.random.default_rng(threads)
    for v in (np.zeros(threads, dtype), np.ones(threads, dtype), rng.integers(0, top + 1, threads).astype(dtype)):
        got = run(lab, lab.WG_EXSCAN32 if dtype is np.uint32 else lab.WG_EXSCAN64, v, dtype, 2 * threads + 2, threads)
        incl = np.cumsum(v, dtype=dtype)                          # unsigned: wraps as the device does
        incl2 = np.cumsum(incl, dtype=dtype)                      # the second call scans the first one's inclusive values
        want = np.concatenate([incl - v, incl[-1:], incl2 - incl, incl2[-1:]])
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3000])
def test_wg_scan_array(lab, n):
    rng = np.random.default_rng(n)
    v = rng.integers(1 << 31, 1 << 32, n).astype(np.uint32)     # two values already cross 2^32
    incl = np.cumsum(v, dtype=np.uint64)
    total = incl[-1:] if n else np.zeros(1, np.uint64)
    got = run(lab, lab.WG_SCAN_WIDEN, v, np.uint64, n + 1, n)
    assert np.array_equal(got, np.concatenate([incl - v, total]))
    # in place, as k_pd_scan_u32: the prefix passes 2^32 - 1 from the third value on and the total passes cap from the first
    cap = 1000
    want = np.concatenate([np.minimum(incl - v, 0xFFFFFFFF), np.minimum(total, cap)]).astype(np.uint32)
    got = run(lab, lab.WG_SCAN_SATURATING, None, np.uint32, n + 1, n, a=cap, in_place=np.concatenate([v, np.zeros(1, np.uint32)]))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 1000, 70001])  # below 256: threads without bytes
def test_wg_crc32(lab, n):
    for data in (np.random.default_rng(n).integers(0, 256, n).astype(np.uint8), np.zeros(n, np.uint8)):
        assert int(run(lab, lab.WG_CRC32, data, np.uint32, 1, n)[0]) == zlib.crc32(data.tobytes())


@pytest.mark.parametrize("n", [1, 5552, 5553, 65521, 200000])
def test_adler_largest_sums(lab, n):
    data = np.full(n, 0xFF, np.uint8)
    assert int(run(lab, lab.WG_ADLER, data, np.uint32, 1, n, a=n, b=n)[0]) == zlib.adler32(data.tobytes())


def test_adler_joined_from_three_segments(lab):
    data = np.random.default_rng(7).integers(0, 256, 100000).astype(np.uint8)
    assert int(run(lab, lab.WG_ADLER, data, np.uint32, 1, data.size, a=12345, b=70001)[0]) == zlib.adler32(data.tobytes())
