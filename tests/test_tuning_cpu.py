"""lars_set_tuning / lars_get_tuning and _ffi.tuning() (no device: neither entry point touches the GPU).  The knobs are one
state per process and every route-equality test of the GPU suite leans on them, so what they hold at start, what they refuse
and what a ``with _ffi.tuning(...)`` block leaves behind are pinned here."""
import json
import os
import re
import subprocess
import sys

import pytest

from lars_image_processing_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what struct Tuning (csrc/common.h) declares
DEFAULTS = {"fused_impl": 0, "hist_impl": 2, "nt_stores": 0, "blocks_per_tile": 0, "selq_window": 1, "selq_list_wgs": 0,
            "u16_hist_impl": 5, "joint_depth": 6, "joint_win_depth": 15, "jpeg_subseq_bits": 512, "joint_window": 1,
            "out_stride_planes": 0}
READ_ONLY = ("last_fused_kernel", "jpeg_last_rounds")
ANY_INTEGER = ("fused_impl", "hist_impl", "nt_stores", "blocks_per_tile", "selq_window", "selq_list_wgs")
# knob: (every value it takes, values just outside, how the message names the domain)
DOMAINS = {
    "joint_depth": ((4, 6, 8, 12), (3, 5, 7, 9, 11, 13), "4, 6, 8 or 12"),
    "joint_window": (range(0, 6), (-1, 6), "0 .. 5"),
    "joint_win_depth": ((4, 5, 6, 12, 15), (3, 7, 11, 13, 14, 16), "4, 5, 6, 12 or 15"),
    "u16_hist_impl": ((5, 1, 3), (0, 2, 4, 6), "5, 1 or 3"),
    "jpeg_subseq_bits": (range(32, 65537), (31, 65537), "32 .. 65536"),
}


def refused(message, **knob):
    with pytest.raises(_ffi.LarsError) as e:
        _ffi.set_tuning(**knob)
    assert e.value.code == -1 and str(e.value) == f"liblars_hip error -1: {message}"


def test_every_name_in_the_header_comment_answers():
    with open(os.path.join(ROOT, "include", "lars_hip.h")) as f:
        text = f.read()
    comment = text[text.index("/* Tuning knobs (per process)"):text.index("int lars_set_tuning(")]
    names = set(re.findall(r'"([a-z0-9_]+)"', comment))
    assert names == (set(DEFAULTS) | set(READ_ONLY)) - {"out_stride_planes"}       # that one: include/lars_lab.h, DESIGN.md
    for name in names | {"out_stride_planes"}:
        assert isinstance(_ffi.get_tuning(name), int)


def test_defaults_of_a_fresh_process():
    code = ("import json\nfrom lars_image_processing_amd import _ffi\n"
            f"print(json.dumps({{k: _ffi.get_tuning(k) for k in {tuple(DEFAULTS) + READ_ONLY!r}}}))\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    assert json.loads(out) == {**DEFAULTS, "last_fused_kernel": 0, "jpeg_last_rounds": 0}


@pytest.mark.parametrize("knob", sorted(DOMAINS))
def test_validated_knobs_take_their_domain_and_nothing_next_to_it(knob):
    inside, outside, words = DOMAINS[knob]
    with _ffi.tuning(**{knob: _ffi.get_tuning(knob)}):
        for v in inside:
            _ffi.set_tuning(**{knob: v})
            assert _ffi.get_tuning(knob) == v
            for bad in outside if v == inside[0] else outside[:1]:
                refused(f"lars_set_tuning: {knob} is {words} (got {bad})", **{knob: bad})
                assert _ffi.get_tuning(knob) == v


@pytest.mark.parametrize("knob", ANY_INTEGER)
def test_unvalidated_knobs_take_any_integer(knob):
    with _ffi.tuning(**{knob: _ffi.get_tuning(knob)}):
        for v in (-2 ** 31, -1, 0, 1, 2, 3, 70000, 2 ** 31 - 1):
            _ffi.set_tuning(**{knob: v})
            assert _ffi.get_tuning(knob) == v


def test_names_that_set_refuses():
    for name in READ_ONLY + ("no_such_knob", ""):
        before = _ffi.get_tuning(name) if name in READ_ONLY else None
        refused(f"lars_set_tuning: unknown key {name}", **{name: 1})
        assert before is None or _ffi.get_tuning(name) == before
    with pytest.raises(_ffi.LarsError, match="lars_get_tuning: unknown key no_such_knob$"):
        _ffi.get_tuning("no_such_knob")
    assert _ffi.load().lars_build_flags() == 0                                       # the product build
    refused("lars_set_tuning: out_stride_planes exists in the laboratory build only (make lablayout); this library would ignore it",
            out_stride_planes=3)
    assert _ffi.get_tuning("out_stride_planes") == 0
    lib = _ffi.load()
    assert lib.lars_set_tuning(None, 1) == -1 and lib.lars_last_error() == b"lars_set_tuning: NULL key"
    assert lib.lars_get_tuning(None, None) == -1 and lib.lars_last_error() == b"lars_get_tuning: NULL"
    assert lib.lars_get_tuning(b"joint_depth", None) == -1 and lib.lars_last_error() == b"lars_get_tuning: NULL"


def held(*names):
    return {k: _ffi.get_tuning(k) for k in names}


def test_tuning_block_restores_what_it_found():
    _ffi.set_tuning(joint_window=3, blocks_per_tile=7)                               # not the defaults
    try:
        with _ffi.tuning(joint_window=0, blocks_per_tile=2, fused_impl=1):
            assert held("joint_window", "blocks_per_tile", "fused_impl") == {"joint_window": 0, "blocks_per_tile": 2, "fused_impl": 1}
        assert held("joint_window", "blocks_per_tile", "fused_impl") == {"joint_window": 3, "blocks_per_tile": 7, "fused_impl": 0}
    finally:
        _ffi.set_tuning(joint_window=DEFAULTS["joint_window"], blocks_per_tile=DEFAULTS["blocks_per_tile"])


def test_tuning_block_restores_on_an_exception():
    with pytest.raises(ZeroDivisionError):
        with _ffi.tuning(joint_depth=12, selq_window=2):
            assert held("joint_depth", "selq_window") == {"joint_depth": 12, "selq_window": 2}
            1 / 0
    assert held("joint_depth", "selq_window") == {"joint_depth": 6, "selq_window": 1}


def test_tuning_block_restores_after_a_half_applied_failure():
    ran = False
    with _ffi.tuning(nt_stores=1):
        with pytest.raises(_ffi.LarsError, match=r"joint_depth is 4, 6, 8 or 12 \(got 5\)$"):
            with _ffi.tuning(nt_stores=0, hist_impl=1, joint_depth=5, joint_window=0):      # applied in this order: the third is refused
                ran = True
        assert not ran
        assert held("nt_stores", "hist_impl", "joint_depth", "joint_window") == {"nt_stores": 1, "hist_impl": 2, "joint_depth": 6, "joint_window": 1}
    with pytest.raises(_ffi.LarsError, match="lars_get_tuning: unknown key no_such_knob$"):  # refused before anything is set
        with _ffi.tuning(nt_stores=1, no_such_knob=1):
            ran = True
    assert not ran and _ffi.get_tuning("nt_stores") == 0


def test_tuning_blocks_nest():
    with _ffi.tuning(joint_window=2, u16_hist_impl=1):
        with _ffi.tuning(joint_window=4):
            with _ffi.tuning(joint_window=0, u16_hist_impl=3):
                assert held("joint_window", "u16_hist_impl") == {"joint_window": 0, "u16_hist_impl": 3}
            assert held("joint_window", "u16_hist_impl") == {"joint_window": 4, "u16_hist_impl": 1}
        assert held("joint_window", "u16_hist_impl") == {"joint_window": 2, "u16_hist_impl": 1}
    assert held("joint_window", "u16_hist_impl") == {"joint_window": 1, "u16_hist_impl": 5}
