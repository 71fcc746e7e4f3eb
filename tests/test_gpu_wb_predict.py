"""White-balance tables predicted from a sample and proven while the planes are written (csrc/wb_predict.hip, k_fused_u8c3's
verifying form, lars_d_fused_verified): whatever the predictor says -- right (wb_predict 1), one value off everywhere (2), or
trusted without a confidence gate (3) -- planes, statistics records, tables, percentiles and channel histograms are the bytes
of the exact route (0).  The pixel threshold is lowered by its knob so that small tiles reach the predictor; the shapes are the
smallest with several tiles per ring and several launches (8 tiles of 256 x 256, ring 4), more than one sample segment per
group (1024 x 1024) and a pixel count that is no multiple of 4 (255 x 257: the tail pixels are counted too)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TYPES = ("NDVI", "GNDVI", "NDWI")


@pytest.fixture(scope="module")
def mods():
    import lars_image_processing_amd as lars
    from lars_image_processing_amd import _ffi
    assert _ffi.device_count() >= 1
    return lars, _ffi


def coarse(shape, seed):
    """Eight values of 12.5 % each per channel: both marks lie 10 % of the samples away from the edges of their bins -- decisive."""
    return (np.random.default_rng(seed).integers(0, 8, shape) * 32 + 7).astype(np.uint8)


def noise(shape, seed):
    """256 values of 0.4 % each: a sample of a small tile cannot place the marks -- refused under an honest gate."""
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def boundary_tile(h, w):
    """The 2 % rank of red falls exactly between two values: order statistic floor((N-1) * 0.02) is 10, the next one 200."""
    n = h * w
    k0 = int(np.floor(np.float64(n - 1) * (np.float64(2.0) / np.float64(100.0))))
    t = coarse((1, h, w, 3), 5)
    red = np.full(n, 200, np.uint8)
    red[np.random.default_rng(6).permutation(n)[:k0 + 1]] = 10
    t[0, :, :, 0] = red.reshape(h, w)
    return t


def run(mods, tiles, ring, mode, indices=TYPES, stats=True, hist_first=False):
    """compute_wb_tables + the launches of run_fused_chunks, chunk by chunk with a copy of every chunk's ring slots taken between the
    launches (what a consumer of the ring sees), then tables, percentiles and histograms."""
    lars, _ffi = mods
    with _ffi.tuning(wb_predict=mode, wb_predict_min_pixels=1):
        b = lars.TileBatch.from_host(tiles)
        outs = b.make_outputs(indices=indices, index=True, ring=ring, arena="plain")
        got = {}
        b.compute_wb_tables()
        if hist_first:
            got["hist_first"] = b.host_hist().tobytes()             # settles the predicted tiles; the launches then run as ever
        verify = b._provisional
        rec = b.new_stats() if stats else None
        mask = lars.batch.index_mask(indices)
        if stats:
            rec.zero()
            _ffi.call("lars_d_stats_begin", C.c_void_p(rec.ptr), b.ntiles, mask, None)
        planes = {t: [] for t in indices}
        for start in range(0, b.ntiles, outs.slots):
            count = min(outs.slots, b.ntiles - start)
            b.run_fused(b.fused_args(indices, True, rec, False, outs, None, start, count, raw=stats, settle=not verify), start if verify else None)
            for t in indices:
                planes[t].append(outs.host_index(t, 0, count))
        if stats:
            _ffi.call("lars_d_stats_end", C.c_void_p(rec.ptr), b.ntiles, mask, b.npix, None)
        b._verified_pass_done(verify)
        _ffi.call("lars_synchronize", None)
        report = b.wb_predict_report()
        for t in indices:
            got[t] = np.concatenate(planes[t]).tobytes()
        if stats:
            got["rec"] = rec.download(_ffi.STATS_DTYPE, (b.ntiles, 3)).tobytes()
            rec.free()
        got["tables"] = b.host_tables().tobytes()
        got["pcts"] = b.host_percentiles().tobytes()
        got["hist"] = b.host_hist().tobytes()
        # and the public route: process() over the same batch gives the same records and ring
        if stats:
            got["process_rec"] = b.process(indices=indices, outputs=outs, route="classic").tobytes()
            got["process_ring"] = outs.host_index(indices[0], 0, outs.slots).tobytes()
        outs.free()
        b.free()
    return got, report, verify


def same(got, ref, what):
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k] == ref[k], (what, k)


SHAPES = {"ring": ((8, 256, 256, 3), 4), "one_large": ((1, 1024, 1024, 3), 1), "tail": ((1, 255, 257, 3), 1)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("content", ["coarse", "noise"])
def test_every_predictor_mode_gives_the_exact_bytes(mods, shape, content):
    dims, ring = SHAPES[shape]
    tiles = (coarse if content == "coarse" else noise)(dims, 11)
    ref, report0, verify0 = run(mods, tiles, ring, 0)
    assert report0 == (0, 0) and not verify0
    with np.errstate(all="ignore"):
        from oracle import index_oracle as orc
        want = orc.index_app(orc.wb_app(tiles[-1]), "NDVI")
    assert np.frombuffer(ref["NDVI"], np.float32).reshape(dims[0], -1)[-1].tobytes() == want.astype(np.float32).tobytes()
    for mode in (1, 2, 3):
        got, (confident, missed), verify = run(mods, tiles, ring, mode)
        assert verify, "the predictor did not run"
        same(got, ref, (shape, content, mode))
        if mode == 2:
            assert missed == confident, (confident, missed)         # one value off: every confident tile is missed and repaired
        if content == "coarse":
            assert confident == dims[0] and missed == (dims[0] if mode == 2 else 0), (mode, confident, missed)
        if mode == 3:
            assert confident == dims[0]                             # no gate: every tile runs on its prediction


def test_settling_before_the_launches_counts_the_histograms(mods):
    tiles = coarse((8, 256, 256, 3), 12)
    ref, _, _ = run(mods, tiles, 4, 0, hist_first=True)
    for mode in (1, 2, 3):
        got, _, verify = run(mods, tiles, 4, mode, hist_first=True)
        assert not verify                                           # host_hist settled the tables: nothing left to prove
        same(got, ref, mode)


def test_mixed_constant_and_boundary_tiles(mods):
    """Refused and confident tiles in one ring; a constant channel (p98 == p2); a tile whose 2 % rank lies between two values, which no
    predicted value can serve: it must end exact under every mode."""
    tiles = np.concatenate([coarse((2, 256, 256, 3), 1), noise((2, 256, 256, 3), 2), coarse((2, 256, 256, 3), 3), boundary_tile(256, 256),
                            noise((1, 256, 256, 3), 4)])
    tiles[4, :, :, 1] = 77
    ref, _, _ = run(mods, tiles, 4, 0)
    for mode in (1, 2, 3):
        got, (confident, missed), _ = run(mods, tiles, 4, mode)
        same(got, ref, mode)
        if mode == 1:
            assert 3 <= confident < 8 and missed == 0, (confident, missed)      # the coarse tiles at least, the noise tiles never
        if mode == 3:
            assert confident == 8 and missed >= 1, (confident, missed)          # the boundary tile cannot be proven


@pytest.mark.parametrize("indices,stats", [(("NDVI",), True), (("GNDVI", "NDWI"), True), (TYPES, False)])
def test_other_launch_forms(mods, indices, stats):
    """One index (its launch does not read green: the verifying form counts it all the same), two indices, planes without statistics."""
    tiles = coarse((3, 256, 256, 3), 21)
    ref, _, _ = run(mods, tiles, 2, 0, indices, stats)
    for mode in (1, 2):
        got, (confident, missed), _ = run(mods, tiles, 2, mode, indices, stats)
        same(got, ref, (indices, mode))
        assert confident == 3 and missed == (3 if mode == 2 else 0)


def test_knobs_and_readers_that_settle(mods):
    lars, _ffi = mods
    assert _ffi.get_tuning("wb_predict") == 1 and _ffi.get_tuning("wb_predict_k") == 3
    tiles = coarse((2, 256, 256, 3), 31)
    with _ffi.tuning(wb_predict=0):
        b0 = lars.TileBatch.from_host(tiles).compute_wb_tables()
        want = (b0.host_tables().tobytes(), b0.host_percentiles().tobytes(), b0.tile_medians().tobytes())
        b0.free()
    with _ffi.tuning(wb_predict=2, wb_predict_min_pixels=1):            # every prediction wrong: a reader that did not settle would show it
        b = lars.TileBatch.from_host(tiles).compute_wb_tables()
        assert b._provisional
        assert b.tile_medians().tobytes() == want[2] and not b._provisional
        b.compute_wb_tables()
        assert (b.host_tables().tobytes(), b.host_percentiles().tobytes()) == want[:2]
        assert b.wb_predict_report() == (2, 0)                          # settled, not missed
        b.free()
    b = lars.TileBatch.from_host(tiles).compute_wb_tables()             # 65536 pixels: below the default threshold
    assert not b._provisional and b.wb_predict_report() == (0, 0)
    b.free()
