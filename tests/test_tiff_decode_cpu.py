"""CPU checks of the TIFF decoder's host side: the model of the LZW kernel (tiff_lzw_model.py) against the host decoder on
valid and mutated streams, lars_tiff_info against tiffio.read_tiff, the parser under the sanitizers, the ABI tables."""
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import tiff_cases as tc
import tiff_lzw_model as model
from conftest import ROOT
from lars_image_processing_amd import _ffi, api, codecs, tiffio
from test_tiffio import lzw_encode, sample


def pillow_lzw_strips():
    """The LZW strips of files Pillow (libtiff) writes, with the bytes each should give."""
    rng = np.random.default_rng(8)
    pics = [rng.integers(0, 256, (40, 50, 3), dtype=np.uint8), np.zeros((60, 64), np.uint8),
            (np.add.outer(np.arange(70), np.arange(90)) % 256).astype(np.uint8)]
    out = []
    for a in pics:
        for extra in ({}, {"tiffinfo": {317: 2}}):
            buf = io.BytesIO()
            Image.fromarray(a).save(buf, format="TIFF", compression="tiff_lzw", **extra)
            blob = buf.getvalue()
            tags = tiffio._read_ifd(memoryview(blob), "<")
            rps = min(tags.get(tiffio.ROWS_PER_STRIP, (a.shape[0],))[0], a.shape[0])
            full = rps * a.shape[1] * (a.shape[2] if a.ndim == 3 else 1)
            for o, c in zip(tags[tiffio.STRIP_OFFSETS], tags[tiffio.STRIP_BYTE_COUNTS]):
                out.append((blob[o:o + c], full))
    return out


def test_model_equals_host_decoder_on_valid_streams():
    rng = np.random.default_rng(4)
    datas = [rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), bytes(30000), (np.arange(20000) // 7 % 251).astype(np.uint8).tobytes(),
             rng.integers(0, 3, 12000, dtype=np.uint8).tobytes(), b"\x07"]
    for data in datas:
        enc = lzw_encode(data)
        assert tc.pack(tc.unpack(enc)) == enc                      # the code-level tools of the corpus read what the encoder writes
        for ndst in (len(data), len(data) + 9, max(1, len(data) // 2), 1):
            got = model.decode(enc, ndst)
            assert got == tc.host_lzw(enc, ndst) and got == (data[:ndst], 0)
    for stream, full in pillow_lzw_strips():
        got = model.decode(stream, full)
        assert got == tc.host_lzw(stream, full) and got[1] == 0 and len(got[0]) > 0


def test_model_equals_host_decoder_on_mutated_streams():
    """Produced bytes and count, or being an error: the same for every stream of the corpus; the model's range assertions
    hold on all of them.  A stream the host decoder refuses as old-style LZW (00 and an odd byte first) never reaches the
    kernel: lars_tiff_info reports it, so the model is not asked."""
    cases = tc.corpus()
    assert sum(1 for c in cases if c[0] != "valid") >= 2000
    kinds, corrupt, old = set(), 0, 0
    for kind, stream, ndst in cases:
        want = tc.host_lzw(stream, ndst)
        if len(stream) >= 2 and stream[0] == 0 and stream[1] & 1:
            assert want[1] == 1
            old += 1
            continue
        got = model.decode(stream, ndst)
        assert got[1] == want[1] and (got[1] or got[0] == want[0]), (kind, stream.hex(), ndst)   # an error, or the same bytes
        kinds.add(kind)
        corrupt += got[1]
    assert kinds == {"valid", "truncated", "flip", "splice", "above", "no-eoi"}
    assert corrupt >= 200 and old < 50


def files_of_every_kind():
    """(name, bytes) of the layouts test_tiffio.py covers, uncompressed, LZW and Deflate, from write_tiff and from Pillow."""
    out = []
    for dtype in (np.uint8, np.uint16):
        for byteorder in ("<", ">"):
            for planar in (1, 2):
                for layout in ({}, {"rows_per_strip": 7}, {"tile": (16, 16)}, {"tile": (32, 48)}):
                    a = sample(dtype, 37, 53, 3, seed=planar)
                    out.append((f"raw-{dtype.__name__}{byteorder}{planar}{layout}", tc.written(a, byteorder=byteorder, planar=planar, **layout)))
    for c in (1, 2, 3, 4, 5):
        a = sample(np.uint16, 9, 11, c)
        out.append((f"spp{c}", tc.written(a[..., 0] if c == 1 else a, predictor=True)))
        out.append((f"lzw-spp{c}", tc.lzw_tiff(a[..., 0] if c == 1 else a, rows_per_strip=4, predictor=True)))
    out.append(("deflate", tc.written(sample(np.uint8, 10, 12, 3), deflate=True)))
    rgb = sample(np.uint8, 10, 12, 3)
    for comp in (None, "tiff_lzw", "tiff_adobe_deflate", "packbits", "jpeg"):
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, format="TIFF", **({"compression": comp} if comp else {}))
        out.append((f"pillow-{comp}", buf.getvalue()))
    buf = io.BytesIO()
    Image.fromarray(sample(np.uint16, 20, 30, 1)[..., 0]).save(buf, format="TIFF", compression="tiff_lzw")
    out.append(("pillow-g16", buf.getvalue()))
    return out


def agree(name, blob):
    """tiff_info and read_tiff on one file: the same fields where read_tiff reads it; ValueError or supported=False where it
    raises TiffError for the directory."""
    try:
        want = tiffio.read_tiff(blob)
    except tiffio.TiffError as e:
        try:
            info = api.tiff_info(blob)
        except ValueError:
            return "refused"
        assert not info["supported"] and info["reason"], (name, str(e), info)
        return info["reason"]
    info = api.tiff_info(blob)
    assert (info["dtype"], info["shape"]) == (want.dtype, want.shape), (name, info)
    deflate = info["compression"] in (8, 32946)
    assert info["supported"] == (not deflate) and (info["reason"] is None) == (not deflate), (name, info)
    return "read"


def test_tiff_info_agrees_with_read_tiff():
    files = files_of_every_kind()
    got = {name: agree(name, blob) for name, blob in files}
    assert got["deflate"] == "read" and got["pillow-packbits"] == "PackBits compression" and got["pillow-jpeg"] == "JPEG compression"
    assert got["pillow-tiff_lzw"] == "read" and got["pillow-g16"] == "read"
    info = api.tiff_info(dict(files)["lzw-spp3"])
    assert (info["width"], info["height"], info["samples"], info["bits"], info["compression"], info["predictor"], info["planar"]) == (11, 9, 3, 16, 5, 2, 1)
    assert (info["tiled"], info["chunk_w"], info["chunk_h"], info["chunks"], info["big_endian"], info["photometric"]) == (False, 11, 4, 3, False, 2)
    info = api.tiff_info(dict(files)["raw-uint8>2{'tile': (32, 48)}"])
    assert (info["tiled"], info["chunk_w"], info["chunk_h"], info["chunks"], info["big_endian"], info["planar"]) == (True, 48, 32, 12, True, 2)
    assert api.tiff_info(dict(files)["spp5"])["extra_samples"] == 2
    # the refusals of test_refuses_what_it_does_not_cover
    with pytest.raises(ValueError, match="byte-order"):
        api.tiff_info(b"PNG....not a tiff")
    big = api.tiff_info(b"II" + struct.pack("<HHHQ", 43, 8, 0, 16) + bytes(32))
    assert not big["supported"] and "BigTIFF" in big["reason"]
    blob = tc.written(sample(np.uint16, 8, 8, 3))
    for bad in (blob[: len(blob) // 2], blob[:8] + bytes(len(blob) - 8)):
        assert agree("damaged", bad) == "refused"
    huge = bytearray(blob)
    at = struct.unpack_from("<I", huge, 4)[0] + 2
    struct.pack_into("<I", huge, at + 8, 0x7FFFFFFF)
    assert agree("huge", bytes(huge)) in ("refused", "2^31 or more decoded bytes")
    # an uncompressed strip shorter than the directory says: the message is read_tiff's
    short = bytearray(blob)
    tags = tiffio._read_ifd(memoryview(blob), "<")
    ifd = struct.unpack_from("<I", blob, 4)[0]
    for i in range(struct.unpack_from("<H", blob, ifd)[0]):
        if struct.unpack_from("<H", blob, ifd + 2 + 12 * i)[0] == tiffio.STRIP_BYTE_COUNTS:
            struct.pack_into("<I", short, ifd + 2 + 12 * i + 8, tags[tiffio.STRIP_BYTE_COUNTS][0] - 1)
    with pytest.raises(tiffio.TiffError, match="holds 383 bytes, 384 expected"):
        tiffio.read_tiff(bytes(short))
    with pytest.raises(ValueError, match="holds 383 bytes, 384 expected"):
        api.tiff_info(bytes(short))
    # old-style LZW is refused where the host decoder refuses it
    old = tc.one_strip_tiff(b"\x00\x01\x02\x03", 4)
    assert agree("old", old) == "old-style (LSB-first) LZW"
    with pytest.raises(NotImplementedError, match="old-style"):
        api.decode_tiff(old)
    with pytest.raises(NotImplementedError, match="Deflate"):
        api.decode_tiff(dict(files)["deflate"])


def test_tiff_info_agrees_with_read_tiff_on_damaged_directories():
    """The byte flips of test_corrupt_files_raise_tiff_error_only, on uncompressed and LZW files."""
    rng = np.random.default_rng(0)
    a = rng.integers(0, 65536, (20, 24, 3), dtype=np.uint16)
    blobs = [tc.written(a), tc.written(a, tile=(16, 16)), tc.written(a, planar=2, byteorder=">"), tc.lzw_tiff(a, rows_per_strip=6, predictor=True)]
    outcomes = set()
    for it in range(1200):
        blob = bytearray(blobs[it % 4])
        ifd = struct.unpack_from("<I" if blob[:2] == b"II" else ">I", blob, 4)[0]
        for _ in range(int(rng.integers(1, 4))):
            blob[int(rng.integers(ifd, len(blob)))] = int(rng.integers(0, 256))
        try:
            want = tiffio.read_tiff(bytes(blob), max_bytes=1 << 24)
        except tiffio.TiffError:
            want = None
        except Exception:                                        # what read_tiff itself does not catch is not this test's
            continue
        try:
            info = api.tiff_info(bytes(blob))
        except ValueError:
            info = None
        if want is not None:
            assert info is not None and info["supported"] and (info["dtype"], info["shape"]) == (want.dtype, want.shape), it
        elif info is not None and info["supported"]:
            # the directory stands and the damage is in an LZW strip: the device's to find, as the host decoder found it
            assert info["compression"] == 5, (it, info)
        outcomes.add((want is not None, info is not None and info["supported"]))
    assert (True, True) in outcomes and (False, False) in outcomes


@pytest.fixture(scope="module")
def asan_bin():
    if _ffi.device_count() > 0:
        pytest.skip("sanitizer target is for the build container, not the GPU box")
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "lars_image_processing_amd", "csrc"), "asan"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "build", "asan", "lars_host_asan")


def fnv(data):
    h = 1469598103934665603
    for byte in bytes(data):
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_parser_under_address_and_ub_sanitizers(asan_bin, tmp_path):
    """The tiff-info mode of the sanitizer driver (kind 6) on the files above and on truncations of them: no report, and the
    shipped library's answers."""
    rng = np.random.default_rng(1)
    cases = []
    for _name, blob in files_of_every_kind():
        cases.append((6, 64, blob))
        cases.append((6, 0, blob))
        for cut in sorted({0, 1, 2, 7, 8, 9, len(blob) - 1, len(blob) // 2, *rng.integers(0, len(blob), 12).tolist()}):
            cases.append((6, 64, blob[:cut]))
        for _ in range(6):
            bad = bytearray(blob)
            ifd = struct.unpack_from("<I" if blob[:2] == b"II" else ">I", blob, 4)[0]
            bad[int(rng.integers(min(ifd, len(bad) - 1), len(bad)))] = int(rng.integers(0, 256))
            cases.append((6, 3, bytes(bad)))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for kind, a, data in cases:
            fh.write(struct.pack("<4I", kind, a, 0, len(data)) + data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([asan_bin, str(path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == f"done {len(cases)} cases"
    lib = _ffi.load()
    refused = 0
    for i, ((_kind, a, data), line) in enumerate(zip(cases, lines)):
        words = dict(w.split("=") for w in line.split()[2:])
        arr = np.frombuffer(data or b"\0", dtype=np.uint8)
        info = _ffi.TiffInfo.array()
        table = np.zeros(a * 2 + 1, dtype=np.int64)
        rc = lib.lars_tiff_info(_ffi.ptr(arr), len(data), info, _ffi.ptr(table) if a else None, a)
        assert int(words["rc"]) == rc, (i, line)
        refused += rc != 0
        if rc == 0:
            assert int(words["h"], 16) == fnv(bytes(info)) and int(words["t"], 16) == fnv(table[:a * 2].tobytes()), (i, line)
    assert refused > 100


def header_enum(prefix):
    text = open(os.path.join(ROOT, "include", "lars_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b%s([A-Z0-9_]+) = (\d+)" % prefix, text)}


def test_info_field_order_matches_header():
    """_ffi.TiffInfo's names stand at the positions of the header's LARS_TIFF_INFO_* enumerators, and api's table of reasons
    follows LARS_TIFF_REASON_*."""
    text = open(os.path.join(ROOT, "include", "lars_hip.h")).read()
    fields = header_enum("LARS_TIFF_INFO_")
    n = int(re.search(r"#define LARS_TIFF_INFO_N (\d+)", text).group(1))
    assert len(fields) == len(_ffi.TiffInfo._fields) == n == 16 == len(_ffi.TiffInfo.array())
    assert sorted(fields.values()) == list(range(n))
    for name, k in fields.items():
        assert _ffi.TiffInfo._fields[k] == name.lower(), (name, k)
    reasons = header_enum("LARS_TIFF_REASON_")
    assert sorted(reasons.values()) == list(range(len(reasons))) and len(reasons) == 12
    assert list(codecs._TIFF_REASONS) == sorted(reasons, key=reasons.get)
    for name in ("lars_tiff_info", "lars_h_decode_tiff", "lars_h_thumbnail_tiff_u8"):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name)
