"""The cache policy of the streaming tile loads is a template parameter (csrc/stream_load.h).  This compiles csrc/fused_v2.hip and
csrc/fused.hip to assembly for gfx950 (no GPU needed) and checks that the tile loads of k_chan_hist_u8c3_v2 and k_fused_u8c3 carry the
alternative policy's modifier in the instantiations built for it and in no other.  The modifier is the one the probe's ISA record
(profiles/load_policy_probe.txt) shows for that value of the immediate.  Nothing is asserted about any other instruction."""
import os
import re
import shutil
import subprocess

import pytest

from lars_image_processing_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lars_image_processing_amd", "csrc")
# a tile load: a vector load of 8 bytes or more through the tile's buffer descriptor, or of 12 / 16 bytes through a pointer
TILE_LOAD = re.compile(r"^\s*(buffer_load_dwordx[234]|global_load_dwordx[34])\s")


def alternative():
    """(value of the policy immediate, its modifier words in the ISA) of the one alternative the kernels are instantiated for."""
    with open(os.path.join(CSRC, "stream_load.h")) as f:
        value = int(re.search(r"\bLOAD_NT = (\d+)", f.read()).group(1))
    with open(os.path.join(ROOT, "profiles", "load_policy_probe.txt")) as f:
        record = f.read()
    m = re.search(rf"k_probe_policyILi0ELi{value}ELb0EEE\w*\n\s+buffer_load_dwordx3 .*? offen(.*)\n", record)
    assert m, "the probe's ISA record has no 12-byte read-only variant of that policy"
    words = m.group(1).split()
    assert words, "the alternative policy carries no modifier"
    return value, words


def kernels(src, tmp_path):
    out = tmp_path / (src + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT}/include",
           "-Wno-pass-failed", "-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", out.read_text(), re.S | re.M)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,kernel", [("fused_v2.hip", "k_chan_hist_u8c3_v2"), ("fused.hip", "k_fused_u8c3")])
def test_tile_loads_carry_the_policy_they_were_built_for(tmp_path, src, kernel):
    value, words = alternative()
    seen = {0: 0, value: 0}
    for name, body in kernels(src, tmp_path).items():
        m = re.search(rf"\d+{kernel}I\w*?Li(\d+)EEEv", name)              # the policy is the last template argument
        if not m:
            continue
        policy = int(m.group(1))
        assert policy in seen, name
        loads = [line.split(";")[0].split() for line in body.split("\n") if TILE_LOAD.match(line)]
        assert loads, f"{name}: no tile load found"
        for ops in loads:
            has = all(w in ops for w in words)
            assert has == (policy == value), (name, " ".join(ops))
        seen[policy] += 1
    assert seen[0] and seen[0] == seen[value], seen                         # every instantiation exists for both policies


def test_the_knob_takes_0_1_2():
    assert _ffi.get_tuning("load_policy") == 0
    with _ffi.tuning(load_policy=0):
        for v in (0, 1, 2):
            _ffi.set_tuning(load_policy=v)
            assert _ffi.get_tuning("load_policy") == v
        for bad in (-1, 3):
            with pytest.raises(_ffi.LarsError, match=r"load_policy is 0 \.\. 2 \(got -?\d\)$"):
                _ffi.set_tuning(load_policy=bad)
    assert _ffi.get_tuning("load_policy") == 0
