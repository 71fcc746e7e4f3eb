"""ctypes binding of liblars_lab.so (include/lars_lab.h): the LABORATORY library -- streaming probes and allocation
kinds.  Not part of the product; build it with ``make -C lars_image_processing_amd/csrc lab`` (``__graft_entry__.build()`` does)."""
from __future__ import annotations

import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from lars_image_processing_amd import _ffi  # noqa: E402
from lars_image_processing_amd._ffi import DeviceBuffer  # noqa: E402,F401

LIB_PATH = os.path.join(ROOT, "lars_image_processing_amd", "liblars_lab.so")
_P, _I, _I64, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


SIGNATURES = {
    "lars_lab_malloc": (_I, [C.POINTER(_P), _SZ, _I, _I, _I, _I]),
    "lars_lab_free": (_I, [_P]),
    "lars_d_probe": (_I, [_I, _I, _I, _P, _P, _I64, _P]),
    "lars_d_probe_mix3": (_I, [_P, _P, _P, _P, _I64, _I, _P]),
    "lars_lab_copy": (_I, [_I, _I, _P, _P, _SZ]),
    "lars_lab_wg_check": (_I, [_I, _P, _P, _I64, C.c_uint64, C.c_uint64, _P]),
}
_lib = None


def available():
    return os.path.exists(LIB_PATH)


def load():
    global _lib
    if _lib is None:
        _ffi.load()                                  # liblars_hip.so first (RTLD_GLOBAL): the laboratory links against it
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def call(name, *args):
    return _ffi.check(getattr(load(), name)(*args))


class LabBuffer(_ffi._DeviceRange):
    """Device memory from ``lars_lab_malloc`` (or adopted from the laboratory), freed with ``lars_lab_free``."""

    def __init__(self, nbytes, kind=0, chunk_mb=0, align_mb=0, shuffle=0, adopt=None):
        self.nbytes = int(nbytes)
        if adopt is not None:
            self.ptr = int(adopt)
            return
        p = C.c_void_p()
        call("lars_lab_malloc", C.byref(p), self.nbytes, int(kind), int(chunk_mb), int(align_mb), int(shuffle))
        self.ptr = p.value

    def free(self):
        if getattr(self, "ptr", None):
            try:
                load().lars_lab_free(C.c_void_p(self.ptr))
            finally:
                self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def probe(kind, unroll, blocks, src, dst, nbytes, stream=None):
    call("lars_d_probe", int(kind), int(unroll), int(blocks), C.c_void_p(src) if src else None, C.c_void_p(dst) if dst else None,
         int(nbytes), stream)


# load-policy probes (csrc/lab/probe.hip, kinds 200 .. 247): condition x tile-load shape x cache policy of csrc/stream_load.h
POLICY_READ, POLICY_MIX, POLICY_SHARED = range(3)                   # read only | 12 B read : 48 B written (12 B shape only) | shared readers
SHAPE_B96, SHAPE_B128_B64, SHAPE_B128 = range(3)                    # 12 B | 16 B + 8 B (the uint16 quad; not with shared readers) | 16 B per lane
LOAD_PLAIN, LOAD_NT, LOAD_SC1, LOAD_NT_SC1 = range(4)


def policy_kind(condition, shape, policy):
    return 200 + 16 * int(condition) + 4 * int(shape) + int(policy)


def probe_policy(condition, shape, policy, unroll, blocks, src, dst, nbytes, stream=None):
    """``unroll``: output slots of the mix (1 .. 64; dst holds that many x 4 x 48 MiB) or readers per chunk (1 | 2); ``blocks``:
    workgroups per chunk of one 4096 x 4096 tile's vectors, or chunks for the shared readers."""
    probe(policy_kind(condition, shape, policy), unroll, blocks, src, dst, nbytes, stream)


def probe_mix3(src, d0, d1, d2, nquads, blocks=65536, stream=None):
    call("lars_d_probe_mix3", C.c_void_p(src), C.c_void_p(d0), C.c_void_p(d1), C.c_void_p(d2), int(nquads), int(blocks), stream)


WG_EXSCAN32, WG_EXSCAN64, WG_SCAN_WIDEN, WG_SCAN_SATURATING, WG_CRC32, WG_ADLER = range(6)


def wg_check(prim, src, dst, n, a=0, b=0, stream=None):
    """One workgroup primitive on device buffers (include/lars_lab.h: lars_lab_wg_check)."""
    call("lars_lab_wg_check", int(prim), C.c_void_p(src) if src else None, C.c_void_p(dst), int(n), int(a), int(b), stream)
