"""The value-window pre-pass of uint16 tiles (lars_d_wb_prepare, csrc/u16.hip) on inputs built to make its prediction fail in
every way it can (tests/u16_window_cases.py), against the line-by-line model of its kernels (tests/u16_window_model.py) and
np.percentile (needs a MI355X).  Every comparison is bit for bit."""
import ctypes as C
import warnings

import numpy as np
import pytest

import u16_window_cases as cases
import u16_window_model as model
from oracle import index_oracle as orc

pytestmark = pytest.mark.gpu
USED = 196608 + 3 * 260 * 4 + 48           # tables, thresholds, percentiles: the part of a tile's blob the pre-pass writes


@pytest.fixture(scope="module")
def lars():
    import lars_image_processing_amd as mod
    from lars_image_processing_amd import _ffi
    assert _ffi.device_count() >= 1
    before = _ffi.get_tuning("u16_hist_impl")
    assert before == 5
    yield mod
    assert _ffi.get_tuning("u16_hist_impl") == before       # the knob is back at its default


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def reference():
    """np.percentile(channel.astype(float32), (2, 98)) per case, tile and channel, and the model's windows and flags: computed once."""
    memo = {}

    def of(case):
        if case.name not in memo:
            pcts = np.zeros((len(case.tiles), 3, 2))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for i, tile in enumerate(case.tiles):
                    for c in range(3):
                        pcts[i, c] = np.percentile(tile[:, :, c].astype(np.float32), (2, 98))
            memo[case.name] = {
                "pcts": pcts,
                "windows": {w: np.stack([model.tile_windows(t, test_wrong=w) for t in case.tiles]) for w in (False, True)},
                "flags": {w: np.array([model.tile_flag(t, test_wrong=w) for t in case.tiles], np.uint32) for w in (False, True)},
            }
            assert memo[case.name]["flags"][False].tolist() == case.flags
        return memo[case.name]
    return of


def upload_repeated(lars, tiles, ntiles):
    """A batch of ntiles tiles: tile i is tiles[i % len(tiles)], copied on the device from one upload of the distinct ones."""
    from lars_image_processing_amd import _ffi
    k = len(tiles)
    b = lars.TileBatch(ntiles, tiles.shape[1], tiles.shape[2], 3, np.uint16)
    b.tiles.upload(tiles)
    have = k
    while have < ntiles:
        count = min(have, ntiles - have)                        # `have` is a multiple of k: the pattern i % k goes on
        _ffi.call("lars_memcpy_d2d", C.c_void_p(b.tiles.ptr + have * b.tile_bytes), C.c_void_p(b.tiles.ptr), count * b.tile_bytes, None)
        have += count
    _ffi.call("lars_synchronize", None)
    return b


def run_three_ways(lars, b, ref, which):
    """compute_wb_tables() under u16_hist_impl 5, 1 and 3 on zeroed buffers: the report against the model under 5 and 3, no report
    under 1, and the used part of every blob and all percentiles byte-identical.  Returns (percentiles, blobs) of impl 5.
    which: the distinct tile behind each tile of the batch."""
    from lars_image_processing_amd import _ffi
    b.compute_wb_tables()                                           # allocates the blobs (their padding is never written)
    got = {}
    for impl in (5, 1, 3):
        with _ffi.tuning(u16_hist_impl=impl):
            b.table.zero(); b.percentiles.zero()
            b.compute_wb_tables()
            _ffi.call("lars_synchronize", None)
            if impl == 1:
                with pytest.raises(_ffi.LarsError, match="value-window") as e:
                    b.u16_window_report()
                assert e.value.code == -1
            else:
                flags, windows = b.u16_window_report()
                assert flags.shape == (b.ntiles,) and windows.shape == (b.ntiles, 3, 4)
                want_w, want_f = ref["windows"][impl == 3][which], ref["flags"][impl == 3][which]
                wrong = np.flatnonzero((windows != want_w).any(axis=(1, 2)))
                assert wrong.size == 0, (f"impl {impl}: the windows of {wrong.size} tiles differ from the model's, first tile {wrong[0]}: "
                                         f"{windows[wrong[0]].tolist()} against {want_w[wrong[0]].tolist()}")
                np.testing.assert_array_equal(flags, want_f, err_msg=f"impl {impl}")
        blob = b.table.download(np.uint8, (b.ntiles, b.table_bytes))[:, :USED]
        got[impl] = (b.host_percentiles(), blob)
    for impl in (1, 3):
        assert got[impl][0].tobytes() == got[5][0].tobytes(), impl
        np.testing.assert_array_equal(got[impl][1], got[5][1], err_msg=f"blobs of impl {impl} and 5")
    return got[5]


def check_against_numpy(case, ref, pcts, blobs, which):
    """Percentiles equal np.percentile and the table rows equal the oracle's on the values present, per tile and channel -- the
    flagged tiles' unflagged channels included."""
    tables = {}
    for i, d in enumerate(which):
        for c in range(3):
            lo, hi = ref["pcts"][d, c]
            assert pcts[i, c, 0] == lo and pcts[i, c, 1] == hi, (case.name, i, c, pcts[i, c].tolist(), (lo, hi))
            if (d, c) not in tables:
                present = np.unique(case.tiles[d][:, :, c])
                tables[(d, c)] = (present, orc.wb_lut_from_percentiles(lo, hi, 65536)[present])
            present, want = tables[(d, c)]
            np.testing.assert_array_equal(blobs[i, c * 65536:(c + 1) * 65536][present], want, err_msg=f"{case.name} tile {i} channel {c}")
    for (i, c, k), value in case.expect.items():
        assert round(float(pcts[i, c, k]), 6) == value


def check_product(lars, case, b):
    """process() with an NDVI plane and the 50-bin histogram: plane and record equal the oracle's on the reference white balance."""
    n = b.ntiles
    outs = b.make_outputs(indices=("NDVI",), index=True)
    rec = b.process(indices=("NDVI",), hist=True, outputs=outs)
    assert b.last_route == "per-pixel"
    for i in range(n):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = orc.index_app(orc.wb_app(case.tiles[i]), "NDVI")
        np.testing.assert_array_equal(bits(outs.host_index("NDVI", i, 1)[0]), bits(want), err_msg=f"{case.name} tile {i}")
        part = orc.tile_partials(want, "NDVI")
        r = rec[i, 0]
        assert int(r["count"]) == part["count"] and int(r["above"]) == part["above"], (case.name, i)
        assert float(r["min"]) == part["min"] and float(r["max"]) == part["max"] and float(r["sum"]) == part["sum"], (case.name, i)
        np.testing.assert_array_equal(np.array(r["hist"], dtype=np.int64), part["hist"])
    outs.free()


@pytest.mark.parametrize("name", cases.SMALL_NAMES)
def test_value_windows_against_the_model_and_numpy(lars, reference, name):
    from lars_image_processing_amd import _ffi
    case = cases.small_case(name)
    ref = reference(case)
    b = lars.TileBatch.from_host(case.tiles)
    which = np.arange(b.ntiles)
    pcts, blobs = run_three_ways(lars, b, ref, which)
    check_against_numpy(case, ref, pcts, blobs, which)
    if case.planes:
        check_product(lars, case, b)
        b.compute_wb_tables()
        _ffi.call("lars_synchronize", None)
        np.testing.assert_array_equal(b.u16_window_report()[0], ref["flags"][False])
    b.free()


def test_two_sampled_stretches_in_flight(lars, reference):
    """The smallest batch in which a workgroup of k_u16_sample12 holds two sampled stretches at once (1024 tiles of 512 x 513, 1.6 GB):
    a wrong stretch index there never gives a wrong percentile, only a wrong window -- so the windows of EVERY tile are compared."""
    case = cases.case_h()
    ref = reference(case)
    npix = case.tiles.shape[1] * case.tiles.shape[2]
    grid_x, nsampled = model.launch_geometry(case.repeat, npix)
    assert nsampled > grid_x and model.takes_window_route(case.repeat, npix)
    b = upload_repeated(lars, case.tiles, case.repeat)
    which = np.arange(case.repeat) % len(case.tiles)
    np.testing.assert_array_equal(b.host_tiles(case.repeat - 1, 1)[0], case.tiles[which[-1]])
    pcts, blobs = run_three_ways(lars, b, ref, which)
    k = len(case.tiles)
    check_against_numpy(case, ref, pcts[:k], blobs[:k], which[:k])              # NumPy sees the distinct tiles ...
    assert pcts.tobytes() == pcts[which].tobytes()                             # ... and every repeat equals its first copy
    assert np.array_equal(blobs, blobs[which])
    b.free()


def test_no_report_without_the_window_route(lars):
    """uint8 batches, tiles below the route's floor, and a batch of another size than the last pre-pass covered: the report raises."""
    from lars_image_processing_amd import _ffi
    u8 = lars.TileBatch.synthetic(2, 64, 64, seed=3)
    u8.compute_wb_tables()
    _ffi.call("lars_synchronize", None)
    with pytest.raises(_ffi.LarsError, match="value-window"):
        u8.u16_window_report()
    rng = np.random.default_rng(9)
    small = lars.TileBatch.from_host(rng.integers(0, 65536, (2, 96, 128, 3), dtype=np.uint16))      # cap < 64: the two radix passes
    small.compute_wb_tables()
    _ffi.call("lars_synchronize", None)
    with pytest.raises(_ffi.LarsError, match="value-window"):
        small.u16_window_report()
    one = lars.TileBatch.from_host(cases.small_case("a-hidden-tails").tiles)
    two = lars.TileBatch.from_host(cases.small_case("b-straddle").tiles[:2])
    one.compute_wb_tables()
    _ffi.call("lars_synchronize", None)
    assert one.u16_window_report()[0].tolist() == [1]
    with pytest.raises(_ffi.LarsError, match="another number of tiles"):
        two.u16_window_report()
    # a uint8 pre-pass through the same entry point in between: the last pre-pass on this thread is no longer the uint16 one
    _ffi.call("lars_d_wb_prepare", C.c_void_p(u8.tiles.ptr), u8.ntiles, u8.npix, 3, _ffi.U8, C.c_void_p(u8.table.ptr),
              C.c_void_p(u8.percentiles.ptr), 0, None)
    _ffi.call("lars_synchronize", None)
    with pytest.raises(_ffi.LarsError, match="took another route"):
        one.u16_window_report()
    for x in (u8, small, one, two):
        x.free()
