"""TileBatch.process launches the same entry points in the same order on each of its six routes (needs a MI355X).

The sequences below were recorded from ``process()`` before it was split into a planner and one runner per route;
``lars_malloc`` / ``lars_free`` are left out (where a buffer is allocated or released may move)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOOKKEEPING = ("lars_malloc", "lars_free")


def _u8(lars, ntiles=2):
    return lars.TileBatch.synthetic(ntiles, 32, 32, seed=1234, profile="vegetation")


def _u16(lars, ntiles=2):
    rng = np.random.default_rng(5)
    return lars.TileBatch.from_host(rng.integers(0, 65536, (ntiles, 32, 32, 3), dtype=np.uint16))


# name -> (batch maker, make_outputs kwargs or None, process kwargs, route process() takes)
CASES = {
    "one-read": (_u8, None, dict(medians=True, route="joint"), "one-read"),
    "one-read-stats": (_u8, None, dict(hist=True, route="auto"), "one-read"),
    "one-read+planes": (_u8, dict(index=True), dict(medians=True, route="auto"), "one-read+planes"),
    "select": (_u8, None, dict(medians=True, route="classic"), "select"),
    "per-pixel+select": (_u8, None, dict(indices=("NDVI", "GNDVI"), medians=True, route="classic"), "per-pixel+select"),
    "per-pixel": (_u8, None, dict(hist=True, route="classic"), "per-pixel"),
    "per-pixel-ring": (lambda lars: _u8(lars, 3), dict(index=True, ring=2), dict(sumsq=True, route="classic"), "per-pixel"),
    "per-pixel+radix": (_u16, None, dict(medians=True), "per-pixel+radix"),
    "per-pixel+radix-planes": (_u16, dict(index=True), dict(indices=("NDVI", "NDWI"), medians=True), "per-pixel+radix"),
}

EXPECTED = {
    "one-read": ["lars_memset", "lars_memset", "lars_memset", "lars_d_stats_joint", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h", "lars_memcpy_d2h"],
    "one-read+planes": ["lars_memset", "lars_memset", "lars_memset", "lars_d_stats_joint", "lars_d_fused", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h", "lars_memcpy_d2h"],
    "one-read-stats": ["lars_memset", "lars_memset", "lars_memset", "lars_d_stats_joint", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h"],
    "per-pixel": ["lars_d_channel_hist", "lars_d_wb_table", "lars_memset", "lars_d_fused", "lars_synchronize", "lars_memcpy_d2h"],
    "per-pixel+radix": ["lars_d_wb_prepare", "lars_memset", "lars_memset", "lars_d_fused", "lars_d_median_pair_batch_f32", "lars_d_median_pair_batch_f32", "lars_d_median_pair_batch_f32", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h"],
    "per-pixel+radix-planes": ["lars_d_wb_prepare", "lars_memset", "lars_memset", "lars_d_fused", "lars_d_median_pair_batch_f32", "lars_d_median_pair_batch_f32", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h"],
    "per-pixel+select": ["lars_d_channel_hist", "lars_d_wb_table", "lars_memset", "lars_d_fused", "lars_d_quotient_median_pairs", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h"],
    "per-pixel-ring": ["lars_d_channel_hist", "lars_d_wb_table", "lars_memset", "lars_d_stats_begin", "lars_d_fused", "lars_d_fused", "lars_d_stats_end", "lars_synchronize", "lars_memcpy_d2h"],
    "select": ["lars_d_channel_hist", "lars_d_wb_table", "lars_memset", "lars_d_stats_medians", "lars_synchronize", "lars_memcpy_d2h", "lars_memcpy_d2h"],
}


def record(lars, name):
    """Entry points ``process()`` calls for case ``name``, in order (lars_malloc / lars_free left out), and the batch."""
    from lars_image_processing_amd import _ffi
    make, outs_kw, kw, _ = CASES[name]
    b = make(lars)
    outs = b.make_outputs(**outs_kw) if outs_kw is not None else None
    _ffi.call("lars_synchronize", None)
    seen, real = [], _ffi.call

    def spy(entry, *args):
        seen.append(entry)
        return real(entry, *args)

    _ffi.call = spy
    try:
        b.process(outputs=outs, **kw)
    finally:
        _ffi.call = real
    if outs is not None:
        outs.free()
    return [e for e in seen if e not in BOOKKEEPING], b


@pytest.fixture(scope="module")
def lars():
    import lars_image_processing_amd as mod
    from lars_image_processing_amd import _ffi
    assert _ffi.device_count() >= 1
    return mod


@pytest.mark.parametrize("name", sorted(CASES))
def test_process_call_order(lars, name):
    calls, b = record(lars, name)
    assert calls == EXPECTED[name], calls
    assert b.last_route == CASES[name][3]
    b.free()
