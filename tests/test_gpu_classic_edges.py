"""The per-pixel ("classic") statistics kernels at the edges of their tile walker and of the npix % 4 tail (needs a MI355X).

k_fused_v2 and k_selq_pass walk a tile in quads, four grid strides in flight (csrc/v2_device.h: for_each_quad_ring), and hand the
last npix % 4 pixels to a scalar tail.  Single tiles of N pixels, with one 1024-thread workgroup:
    N = 3       no quad at all: only the tail runs, the walker returns early
    N = 4097    exactly one full stride + 1 tail pixel
    N = 8214    3 iterations with a ragged last one + 2 tail pixels
    N = 16384   exactly 4 iterations: the main loop is skipped, the remainder does all
    N = 20483   5 iterations: one round of the main loop + 1 remainder, + 3 tail pixels
    N = 36869   10 iterations: two rounds + 2 remainder, + 1 tail pixel
blocks_per_tile = 3 gives a stride that is no power of two."""
import warnings

import numpy as np
import pytest

from oracle import index_oracle as orc

pytestmark = pytest.mark.gpu
TYPES = ("NDVI", "GNDVI", "NDWI")
SIZES = (3, 4097, 8214, 16384, 20483, 36869)
_REFERENCE = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def reference(n, tile):
    """Per white-balance setting: the image the indices are taken of, and per index its plane, partial statistics and median.
    Computed once per size; nobody writes to it."""
    if n not in _REFERENCE:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            images = {True: orc.wb_app(tile), False: tile}
        ref = {}
        for wb, img in images.items():
            planes = {t: orc.index_app(img, t) for t in TYPES}
            ref[wb] = {"image": img, "planes": planes, "partials": {t: orc.tile_partials(planes[t], t) for t in TYPES},
                       "medians": np.array([float(np.median(planes[t])) for t in TYPES])}
        _REFERENCE[n] = ref
    return _REFERENCE[n]


def check_records(rec, ref, hist, sumsq):
    for k, t in enumerate(TYPES):
        r, part = rec[0, k], ref["partials"][t]
        assert int(r["count"]) == part["count"] and int(r["above"]) == part["above"], t
        assert float(r["min"]) == part["min"] and float(r["max"]) == part["max"], t
        assert float(r["sum"]) == part["sum"], t                             # exact fixed-point sum
        if sumsq:
            assert float(r["sumsq"]) == pytest.approx(part["sumsq"], rel=1e-9), t
        if hist:
            np.testing.assert_array_equal(np.array(r["hist"], dtype=np.int64), part["hist"])


def same_records(a, b):
    """Bit for bit, but for the sum of squares (per pixel on one route, per counted cell on the other: batch.py)."""
    a, b = a.copy(), b.copy()
    np.testing.assert_allclose(a["sumsq"], b["sumsq"], rtol=1e-12, atol=2.0 ** -26)
    a["sumsq"] = b["sumsq"] = 0
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("blocks", [0, 3])
@pytest.mark.parametrize("n", SIZES)
def test_walker_and_tail_edges(n, blocks):
    import lars_image_processing_amd as lars
    from lars_image_processing_amd import _ffi
    assert _ffi.device_count() >= 1
    b = lars.TileBatch.synthetic(1, 1, n, seed=77 + n, profile="vegetation")
    tile = b.host_tiles()[0]
    both = reference(n, tile)
    with _ffi.tuning(blocks_per_tile=blocks):
        for wb in (True, False):
            ref = both[wb]
            # statistics only: k_fused_v2 without outputs, with and without the histograms and the sums of squares
            for hist in (False, True):
                rec = b.process(route="classic", white_balance=wb, hist=hist, sumsq=hist)
                assert b.last_route == "per-pixel" and _ffi.get_tuning("last_fused_kernel") == 2
                check_records(rec, ref, hist, hist)
                same_records(rec, b.process(route="joint", white_balance=wb, hist=hist, sumsq=hist))
            # medians: the predicted windows inside the statistics kernel (SEL = 2) and, with the histograms, its bucket pass
            # (SEL = 1); k_selq_predict, k_selq_pass
            for hist in (False, True):
                rec, med = b.process(route="classic", white_balance=wb, hist=hist, medians=True)
                assert b.last_route == "select"
                check_records(rec, ref, hist, False)
                np.testing.assert_array_equal(med[0], ref["medians"])
                rec_j, med_j = b.process(route="joint", white_balance=wb, hist=hist, medians=True)
                assert b.last_route == "one-read"
                assert rec.tobytes() == rec_j.tobytes() and med.tobytes() == med_j.tobytes()
            # planes: the second-generation kernel with outputs
            outs = b.make_outputs(index=True, wb=wb, rgba=True, arena="plain")
            with _ffi.tuning(fused_impl=2):
                rec = b.process(route="classic", white_balance=wb, hist=True, sumsq=True, outputs=outs)
                assert b.last_route == "per-pixel" and _ffi.get_tuning("last_fused_kernel") == 2
            check_records(rec, ref, True, True)
            if wb:
                np.testing.assert_array_equal(outs.host_wb(0, 1)[0], ref["image"])
            for t in TYPES:
                np.testing.assert_array_equal(bits(outs.host_index(t, 0, 1)[0]), bits(ref["planes"][t]))
                lut = lars.colormap_lut("RdYlBu" if t == "NDWI" else "RdYlGn")
                np.testing.assert_array_equal(outs.host_rgba(t, 0, 1)[0], orc.colormap_closed_form(ref["planes"][t], lut))
            outs.free()
    b.free()
