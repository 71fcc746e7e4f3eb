"""Sampled white-balance tables, the parts that need no GPU: the condition by which counts below and up to a predicted value
prove a percentile (tests/wb_predict_model.py == csrc/wb_predict_device.h) against the oracle's np.percentile; the CDF margins
of the bench's vegetation tiles, which decide how large the sample must be; the register budget of the verifying kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wb_predict_model as model
from oracle import index_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def histograms():
    rng = np.random.default_rng(7)
    out = []
    for n in range(1, 41):                                      # every small N, a handful of values each
        out.append(np.bincount(rng.integers(0, 4, n) * 60, minlength=256))
        out.append(np.bincount(rng.integers(0, 256, n), minlength=256))
    for _ in range(60):                                         # random: dense, sparse, skewed
        n = int(rng.integers(41, 200000))
        vals = int(rng.integers(1, 257))
        p = rng.dirichlet(np.full(vals, float(rng.choice([0.05, 1.0, 20.0]))))
        h = np.zeros(256, np.int64)
        h[np.sort(rng.choice(256, vals, replace=False))] = rng.multinomial(n, p)
        out.append(h)
    for v in (0, 1, 128, 254, 255):                             # constant channels
        for n in (1, 2, 51, 65536):
            h = np.zeros(256, np.int64)
            h[v] = n
            out.append(h)
    # two values with the ranks of a mark on, one before and one after the boundary between them -- also where (N-1) * q is an integer
    for n in (7, 40, 51, 101, 1000, 65535, 65536, 255 * 257, 4096 * 4096):
        for k in range(2):
            lo, hi, _ = model.mark_ranks(n, k)
            for first in {lo, lo + 1, hi, hi + 1, lo - 1}:
                if 0 < first < n:
                    for a, b in ((0, 255), (10, 11), (10, 200)):
                        h = np.zeros(256, np.int64)
                        h[a], h[b] = first, n - first
                        out.append(h)
    return out


def test_counts_prove_a_percentile_exactly_when_it_is_the_value():
    """"The condition holds" is equivalent to "the oracle's percentile == v" -- with the one exception counts at v cannot see: a percentile
    interpolated between two DIFFERENT order statistics that happens to be a whole number (two pixels 148 and 198: p2 = 148 + 50 * 0.02 =
    149.0, a value no pixel has).  There the condition must say no for every v, like for any other interpolated percentile: a miss, repaired
    on the exact route to the same number."""
    checked = fractional = coincidences = 0
    for h in histograms():
        cum = np.cumsum(h)
        for k, q in ((0, 2), (1, 98)):
            p = float(orc.percentile_from_hist(h, q))
            lo, hi, t = model.mark_ranks(int(h.sum()), k)
            a, b = int(np.searchsorted(cum, lo, side="right")), int(np.searchsorted(cum, hi, side="right"))
            interpolated = a != b and t != 0.0
            v0, _, _ = model.mark_value(h, k)
            for v in sorted({0, 255, v0, max(v0 - 1, 0), min(v0 + 1, 255), int(np.floor(p)), int(np.ceil(p))}):
                want = False if interpolated else p == v
                assert model.mark_exact(h, k, v) == want, (h.nonzero()[0], h[h.nonzero()[0]], k, v, p)
                checked += 1
            fractional += p != int(p)
            coincidences += interpolated and p == int(p)
    assert checked > 2000 and fractional > 10 and coincidences >= 1     # fractional percentiles are among the cases: always a miss


def test_margins_of_the_bench_tiles():
    """The 98 % marks of red and NIR of the bench's vegetation tiles lie 0.045-0.053 % of the pixels from a bin edge: a sample of n
    pixels places a 2 % mark with sigma = sqrt(0.0196 / n), so 65536 pixels (0.00055) cannot decide them and an eighth of a tile
    (2.1 million: 0.0001) can, at 4.5 sigma and more.  The other four marks have 0.0034 and more."""
    want = {0: (0.00049, 0.00053), 1: (0.00045, 0.00049), 777: (0.00047, 0.00045)}
    for tile, (red, nir) in want.items():
        img = orc.synth_tile_u8(1234, tile, 4096, 4096, profile="vegetation")
        got = {}
        for c in range(3):
            h = np.bincount(img[..., c].ravel(), minlength=256)
            for k in range(2):
                got[c, k] = model.cdf_margin(h, k)
        assert got[0, 1] == (113, pytest.approx(red, abs=5.1e-6)) and got[2, 1] == (247, pytest.approx(nir, abs=5.1e-6)), (tile, got)
        assert all(round(m, 4) >= 0.0034 for key, (_, m) in got.items() if key not in ((0, 1), (2, 1))), (tile, got)
        sigma = np.sqrt(0.0196 / (4096 * 4096 / 8))
        assert min(red, nir) / sigma > 4.4 and min(red, nir) / np.sqrt(0.0196 / 65536) < 1.0


def test_the_gate_passes_decisive_samples_and_refuses_close_ones():
    rng = np.random.default_rng(3)
    coarse = np.stack([np.bincount(rng.integers(0, 8, 1365) * 32 + 7, minlength=256) for _ in range(model.GROUPS)])
    assert model.predict(coarse) == ((7, 231), True)
    noise = np.stack([np.bincount(rng.integers(0, 256, 1365), minlength=256) for _ in range(model.GROUPS)])
    values, confident = model.predict(noise)
    assert not confident and abs(values[0] - 5) <= 2 and abs(values[1] - 250) <= 2
    const = np.zeros((model.GROUPS, 256), np.int64)
    const[:, 77] = 1365
    assert model.predict(const) == ((77, 77), True)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_verifying_kernel_keeps_two_waves_per_simd(tmp_path):
    """The verifying form of the headline instantiation (k_fused_u8c3<uint8, 7, true, 1, 3, 1, POLICY>) within 256 registers and
    without scratch, compiled as tests/test_registers_cpu.py compiles it."""
    out = tmp_path / "fused.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT}/include",
           "-Wno-pass-failed", "-S", "--cuda-device-only", f"{ROOT}/lars_image_processing_amd/csrc/fused.hip", "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n((?:    .*\n)+)", out.read_text()):
        name = re.search(r"\.name:\s+(\S+)", m.group(1))
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size):\s+(\d+)", m.group(1))}
    hits = {k: v for k, v in meta.items() if re.search(r"k_fused_u8c3IhLj7ELb1ELi1ELi3ELi1ELi\dE", k)}
    assert len(hits) == 2, sorted(hits)                         # plain and nt tile loads
    for name, v in hits.items():
        assert v["vgpr_count"] <= 256 and v["private_segment_fixed_size"] == 0, (name, v)
