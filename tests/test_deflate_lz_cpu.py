"""String matching in the device Deflate coder, without a device: the tuning knob ``deflate_matching`` and its context manager,
the stream's Python model (tests/deflate_lz_model.py) judged by zlib on the shared cases (tests/deflate_lz_cases.py), what those
cases cover, the driver's new encoder values, and the resources of the two new kernels read from the compiler's metadata."""
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_lz_cases as cases
import deflate_lz_model as lm
import lars_image_processing_amd as lars
import png_encode_model as pm
from lars_image_processing_amd import _ffi, codecs, driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SEG = lm.SEG


# ---------------------------------------------------------------------------------------------------------------------
# the knob
# ---------------------------------------------------------------------------------------------------------------------
def test_knob_default_values_and_refusals():
    assert _ffi.get_tuning("deflate_matching") == 0
    try:
        for v in (1, 0, 1):
            _ffi.set_tuning(deflate_matching=v)
            assert _ffi.get_tuning("deflate_matching") == v
        for bad in (-1, 2):
            with pytest.raises(_ffi.LarsError, match=r"lars_set_tuning: deflate_matching is 0 or 1 \(got %d\)" % bad):
                _ffi.set_tuning(deflate_matching=bad)
            assert _ffi.get_tuning("deflate_matching") == 1
    finally:
        _ffi.set_tuning(deflate_matching=0)


def test_context_manager_restores_what_it_found():
    assert lars.deflate_matching is codecs.deflate_matching and not hasattr(lars.api, "deflate_matching")
    assert _ffi.get_tuning("deflate_matching") == 0
    with codecs.deflate_matching():
        assert _ffi.get_tuning("deflate_matching") == 1
        with codecs.deflate_matching(False):
            assert _ffi.get_tuning("deflate_matching") == 0
        assert _ffi.get_tuning("deflate_matching") == 1
        with codecs.deflate_matching(True):
            assert _ffi.get_tuning("deflate_matching") == 1
        assert _ffi.get_tuning("deflate_matching") == 1
    assert _ffi.get_tuning("deflate_matching") == 0
    with pytest.raises(RuntimeError, match="inside"):
        with codecs.deflate_matching():
            raise RuntimeError("inside")
    assert _ffi.get_tuning("deflate_matching") == 0
    with _ffi.tuning(deflate_matching=1):
        with pytest.raises(RuntimeError):
            with codecs.deflate_matching(False):
                raise RuntimeError("inside")
        assert _ffi.get_tuning("deflate_matching") == 1
    assert _ffi.get_tuning("deflate_matching") == 0


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
NAMES = sorted(cases.byte_cases())


@pytest.mark.parametrize("name", NAMES)
def test_zlib_inflates_the_models_stream(name):
    data = cases.byte_cases()[name]
    stream, _ = cases.streams()[name]
    assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == data


@pytest.mark.parametrize("name", NAMES)
def test_no_segment_is_longer_than_without_matching(name):
    data = cases.byte_cases()[name]
    _, rec = cases.streams()[name]
    assert len(rec["forms"]) == -(-len(data) // SEG)
    for k, form in enumerate(rec["forms"]):
        part, last = data[k * SEG:(k + 1) * SEG], (k + 1) * SEG >= len(data)
        mine, today = lm.body_bytes(part, last), pm.body_bytes(part, last)
        assert len(mine) <= len(today)
        assert (mine == today) == (form != "matched")       # where the literal-only or the stored block wins, the bytes are today's
        assert pm.segment(part, last)["stored"] == (form == "stored") or form == "matched"


def test_symbol_tables_are_deflates():
    """RFC 1951, section 3.2.5, written out."""
    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]
    dext = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
    for length in range(3, 259):
        s = max(i for i in range(29) if lbase[i] <= length) if length < 258 else 28
        assert lm.length_symbol(length) == (257 + s, lext[s], length - lbase[s])
    for dist in range(1, 32769):
        s = max(i for i in range(30) if dbase[i] <= dist)
        assert lm.distance_symbol(dist) == (s, dext[s], dist - dbase[s])


def test_the_cases_cover_every_symbol_both_fallbacks_and_the_widest_tokens():
    """From the model's own record of the matched blocks it wrote."""
    lsyms, dsyms, forms, width, depth = set(), set(), set(), 0, 0
    for _, rec in cases.streams().values():
        lsyms |= rec.get("lsyms", set())
        dsyms |= rec.get("dsyms", set())
        forms |= set(rec["forms"])
        width = max(width, rec.get("max_token_bits", 0))
        depth = max(depth, rec.get("max_code_len", 0))
    assert lsyms == set(range(257, 286)) and dsyms == set(range(30))
    assert forms == {"matched", "literal", "stored"}
    assert width >= 40 and depth == 15


def test_the_cases_named_for_a_path_take_it():
    s = cases.streams()
    assert s["random"][1]["forms"] == ["stored", "stored"] and s["random16"][1]["forms"] == ["literal", "literal"]
    assert s["zeros32769"][1]["forms"] == ["matched", "stored"] and s["zeros65536"][1]["forms"] == ["matched", "matched"]
    assert len(s["zeros65536"][0]) == 2 * len(s["zeros32768"][0]) - 2          # two equal segments that do not see each other
    assert all(s[f"equal{n}"][1]["forms"] == ["stored"] for n in (1, 2, 3, 4, 5))
    assert lm.parse(cases.byte_cases()["equal259"]) == [(77,), (258, 1)]
    assert lm.parse(cases.byte_cases()["equal261"]) == [(77,), (258, 1), (77,), (77,)]
    assert lm.parse(cases.byte_cases()["equal262"]) == [(77,), (258, 1), (3, 1)]
    assert lm.parse(cases.byte_cases()["equal263"]) == [(77,), (258, 1), (4, 1)]
    assert lm.parse(cases.byte_cases()["far_word"])[-1] == (4, SEG - 4) and s["far_word"][1]["forms"] == ["matched"]
    across = cases.byte_cases()["repeat_across_segments"]
    first, second = lm.parse(across[:SEG]), lm.parse(across[SEG:])
    assert first[-1][0] == 40 and len(first[-1]) == 2 and all(len(t) == 1 for t in second[:10])    # the copy stops at the border
    assert s["fibonacci"][1]["forms"] == ["matched"] and s["fibonacci"][1]["max_code_len"] == 15


def test_flat_segments_cost_under_100_bytes():
    for n in (32768, 65536):
        stream, _ = cases.streams()[f"zeros{n}"]
        assert len(stream) < 100 * (n // SEG) + 6


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
def _no_device(*_a, **_k):
    raise AssertionError("the library must not be reached")


def test_driver_values(monkeypatch, tmp_path):
    assert driver.PNG_ENCODERS_MATCHING == ("device+matching",) and driver.TIFF_ENCODERS_MATCHING == ("device+deflate+matching",)
    assert driver.PNG_ENCODERS == ("pillow", "device") and driver.TIFF_ENCODERS == ("pillow", "device", "device+deflate")      # as they were
    driver._check_png_encoder("device+matching")
    driver._check_tiff_encoder("device+deflate+matching")
    monkeypatch.setattr(driver.api, "process_image", _no_device)
    for call in (lambda **kw: driver.process_image(tmp_path / "x.png", tmp_path, **kw), lambda **kw: driver.batch_process(tmp_path, tmp_path, **kw)):
        for bad in ("device+match", "matching", "device+deflate+matching"):
            with pytest.raises(ValueError, match=r"^png_encoder must be 'pillow' or 'device'"):
                call(png_encoder=bad)
        for bad in ("device+matching", "device+lzw+matching", "deflate"):
            with pytest.raises(ValueError, match=r"^tiff_encoder must be 'pillow' or 'device'"):
                call(tiff_encoder=bad)
    with pytest.raises(ValueError, match=r"^png_encoder must be 'pillow' or 'device'"):
        driver.export_zip(np.zeros((4, 4, 3), np.uint8), ["NDVI"], png_encoder="device+deflate+matching")
    for flag, value in (("--png-encoder", "device+matching"), ("--tiff-encoder", "device+deflate+matching")):
        assert driver.main([str(tmp_path / "empty_in"), str(tmp_path / "out"), flag, value, "--quiet"]) == 0      # no files: nothing to encode
    assert _ffi.get_tuning("deflate_matching") == 0


def test_batch_process_sets_the_knob_once_around_the_pool(monkeypatch, tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    for k in range(3):
        (src / f"f{k}.png").write_bytes(b"")
    seen = []

    def fake(path, out, wb, indices, full_depth, lut_format, png_encoder, png_decoder, jpeg_decoder, tiff_decoder, tiff_encoder, index_tiff):
        seen.append((_ffi.get_tuning("deflate_matching"), png_encoder, tiff_encoder))
        return {}

    sets = []
    real = _ffi.set_tuning
    monkeypatch.setattr(driver, "_process_image", fake)
    monkeypatch.setattr(_ffi, "set_tuning", lambda **kw: (sets.append(kw), real(**kw))[1])
    for workers in (1, 3):
        seen.clear()
        sets.clear()
        res = driver.batch_process(src, tmp_path / "out", workers=workers, verbose=False, png_encoder="device+matching",
                                   tiff_encoder="device+deflate+matching")
        assert sorted(res) == ["f0.png", "f1.png", "f2.png"] and seen == [(1, "device", "device+deflate")] * 3
        assert sets == [{"deflate_matching": 1}, {"deflate_matching": 0}]           # once in, once out: not per file
        assert _ffi.get_tuning("deflate_matching") == 0
    with _ffi.tuning(deflate_matching=1):
        driver.batch_process(src, tmp_path / "out", workers=1, verbose=False, png_encoder="device")
        assert _ffi.get_tuning("deflate_matching") == 1 and seen[-1] == (1, "device", "pillow")    # "device" leaves the knob alone
    seen.clear()
    driver.batch_process(src, tmp_path / "out", workers=1, verbose=False, tiff_encoder="device+deflate+matching")
    assert seen == [(1, "pillow", "device+deflate")] * 3 and _ffi.get_tuning("deflate_matching") == 0


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' resources
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,kernel", [("png.hip", "k_png_deflate_lz"), ("tiff_encode.hip", "k_tz_deflate_lz")])
def test_kernels_fit_one_compute_unit_and_use_no_scratch(tmp_path, src, kernel):
    out = tmp_path / (src + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT}/include",
           "-Wno-pass-failed", "-S", "--cuda-device-only", f"{ROOT}/lars_image_processing_amd/csrc/{src}", "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n((?:    .*\n)+)", out.read_text()):
        block = m.group(1)
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|group_segment_fixed_size|private_segment_fixed_size|max_flat_workgroup_size):\s+(\d+)", block)}
    hits = [v for k, v in meta.items() if kernel in k]
    assert len(hits) == 1, sorted(meta)
    v = hits[0]
    assert v["group_segment_fixed_size"] <= 160 * 1024 and v["private_segment_fixed_size"] == 0, v
    assert v["group_segment_fixed_size"] > 80 * 1024            # one workgroup per compute unit, as DESIGN.md says
    assert v["max_flat_workgroup_size"] == 1024 and v["vgpr_count"] <= 128, v     # 16 waves of one workgroup: 128 registers each
