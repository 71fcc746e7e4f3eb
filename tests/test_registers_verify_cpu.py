"""The verifying forms of the plane-writing kernel (k_fused_u8c3<uint8, MASK, WB, STATS, 3, VERIFY = 1, POLICY>, csrc/fused.hip) carry a
table of dwords, a packed counter per channel and twelve counts on top of what the plain forms hold.  The headline form (three planes +
basic statistics) must still leave TWO resident waves per SIMD -- 256 registers -- and none of them may spill: a spilled register in
the quad loop is a scratch access per pixel quad.  Compiles csrc/fused.hip to assembly for gfx950 (no GPU needed), as
tests/test_registers_cpu.py does, and reads the counts back."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_verifying_forms_keep_two_waves_and_do_not_spill(tmp_path):
    out = tmp_path / "fused.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT}/include",
           "-Wno-pass-failed", "-S", "--cuda-device-only", f"{ROOT}/lars_image_processing_amd/csrc/fused.hip", "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n((?:    .*\n)+)", out.read_text()):
        name = re.search(r"\.name:\s+(\S+)", m.group(1))
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size):\s+(\d+)", m.group(1))}
    # k_fused_u8c3<unsigned char, MASK, true, STATS, 3, 1, POLICY>: masks 1, 2, 4, 7 x statistics 0, 1 x two load policies
    verifying = {}
    for name, v in meta.items():
        m = re.search(r"k_fused_u8c3IhLj(\d)ELb1ELi([01])ELi3ELi1ELi(\d+)EEEv", name)
        if m:
            verifying[tuple(int(x) for x in m.groups())] = v
    assert sorted(verifying) == sorted((mask, stats, policy) for mask in (1, 2, 4, 7) for stats in (0, 1) for policy in (0, 2)), sorted(verifying)
    for key, v in verifying.items():
        assert v["vgpr_count"] <= 256 and v["private_segment_fixed_size"] == 0, (key, v)
    # the product holds no laboratory form
    assert not [n for n in meta if re.search(r"k_fused_u8c3IhLj\dELb1ELi[01]ELi3ELi([2-9]|\d\d)ELi", n)]
