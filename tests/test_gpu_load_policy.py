"""The ``load_policy`` knob only changes the cache policy of the kernels' streaming tile loads (csrc/stream_load.h): the loads return
the same bytes, so every result is identical bit for bit under 1 (plain everywhere), 2 (nt everywhere) and 0 (each kernel's own
choice).  The shapes are the smallest that still reach every load site and every tail of the load pipelines."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TYPES = ("NDVI", "GNDVI", "NDWI")
# the windowed one-read kernel serves tiles of at least 2^20 pixels (JW_MIN_PIXELS, csrc/joint_device.h): 128 x 128 is below that, and
# 1024 x 1024 is the smallest tile for which joint_window_report() says windowed under the default joint_window setting
WINDOWED_EDGE = 1024
# the uint16 value-window pre-pass serves tiles of at least 64 steps of 1024 quads per workgroup row (u16.hip: cap >= 64): 64 x 64 takes the
# radix passes under either u16_hist_impl, 512 x 512 is the smallest square tile on value windows
U16_WINDOW_EDGE = 512


@pytest.fixture(scope="module")
def mods():
    import lars_image_processing_amd as lars
    from lars_image_processing_amd import _ffi
    assert _ffi.device_count() >= 1
    return lars, _ffi


def _rgn(shape, seed, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    hi = 256 if dtype == np.uint8 else 65536
    return rng.integers(0, hi, shape).astype(dtype)


def _classic_planes(lars, tiles, ring):
    """Pre-pass + plane-writing kernel with statistics: ring planes, records, tables, percentiles, channel histograms."""
    b = lars.TileBatch.from_host(tiles)
    outs = b.make_outputs(index=True, ring=ring, arena="plain")
    rec = b.process(outputs=outs, route="classic")
    assert b.last_route == "per-pixel"
    got = {"rec": rec.tobytes(), "tables": b.host_tables().tobytes(), "pcts": b.host_percentiles().tobytes(),
           "hist": b.host_hist().tobytes()}
    for t in TYPES:
        got[t] = outs.host_index(t, 0, outs.slots).tobytes()
    outs.free()
    b.free()
    return got


def _one_read(lars, b, want_windowed):
    rec, med = b.process(medians=True, route="joint")
    assert b.last_route == "one-read"
    windowed, recounted = b.joint_window_report()
    assert (windowed, recounted) == ((b.ntiles, 0) if want_windowed else (0, 0)), (windowed, recounted)
    got = {"rec": rec.tobytes(), "med": med.tobytes(), "tables": b.host_tables().tobytes(), "pcts": b.host_percentiles().tobytes()}
    rec1 = b.process(indices=("NDVI",), route="joint")            # one value stream: the one-reader form of the full tables
    got["rec1"] = rec1.tobytes()
    got["tables1"] = b.host_tables(partial=True)[:, [0, 2]].tobytes()
    return got


def case_classic_ring(lars, _ffi):
    return _classic_planes(lars, _rgn((3, 64, 40, 3), 1), ring=2)          # two launches, the second one partial


def case_pipeline_tail(lars, _ffi):
    return _classic_planes(lars, _rgn((1, 72, 60, 3), 2), ring=1)          # npix / 4 = 1080: not a multiple of 1024


def case_rgba(lars, _ffi):
    tiles = _rgn((1, 64, 64, 4), 3)
    got = _classic_planes(lars, tiles, ring=1)
    b = lars.TileBatch.from_host(tiles)
    got.update({"joint_" + k: v for k, v in _one_read(lars, b, False).items()})
    b.free()
    return got


def case_one_read_windowed(lars, _ffi):
    b = lars.TileBatch.synthetic(2, WINDOWED_EDGE, WINDOWED_EDGE, seed=1234, profile="vegetation")
    got = _one_read(lars, b, True)
    b.free()
    return got


def case_one_read_full_tables(lars, _ffi):
    b = lars.TileBatch.synthetic(2, 128, 128, seed=1234, profile="uniform")
    got = _one_read(lars, b, False)
    b.free()
    return got


def _u16(lars, _ffi, edge, windows):
    tiles = _rgn((2, edge, edge, 3), 4, np.uint16)
    got = {}
    for impl in (5, 1):
        b = lars.TileBatch.from_host(tiles)
        with _ffi.tuning(u16_hist_impl=impl):
            b.compute_wb_tables()
            _ffi.call("lars_synchronize", None)
            if windows and impl == 5:
                flags, _ = b.u16_window_report()                            # raises unless the value-window route served the pass
                got["flags"] = flags.tobytes()
            got[f"tables{impl}"] = b.host_tables().tobytes()
            got[f"pcts{impl}"] = b.host_percentiles().tobytes()
            outs = b.make_outputs(indices=("NDVI",), index=True, arena="plain")
            rec = b.process(indices=("NDVI",), outputs=outs)
        got[f"rec{impl}"] = rec.tobytes()
        got[f"ndvi{impl}"] = outs.host_index("NDVI", 0, 2).tobytes()
        outs.free()
        b.free()
    assert got["tables5"] == got["tables1"] and got["ndvi5"] == got["ndvi1"]
    return got


def case_u16_radix(lars, _ffi):
    return _u16(lars, _ffi, 64, False)


def case_u16_value_windows(lars, _ffi):
    return _u16(lars, _ffi, U16_WINDOW_EDGE, True)


def case_medians(lars, _ffi):
    b = lars.TileBatch.from_host(_rgn((3, 64, 40, 3), 1))
    glob = b.global_medians()
    rec, med = b.process(medians=True, route="classic")                     # the per-tile select passes
    assert b.last_route == "select"
    b.free()
    return {"global": np.array([glob[t] for t in TYPES]).tobytes(), "rec": rec.tobytes(), "med": med.tobytes()}


CASES = [case_classic_ring, case_pipeline_tail, case_rgba, case_one_read_windowed, case_one_read_full_tables, case_u16_radix,
         case_u16_value_windows, case_medians]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__[5:] for c in CASES])
def test_results_do_not_depend_on_the_load_policy(mods, case):
    lars, _ffi = mods
    ref = None
    for policy in (1, 2, 0):
        with _ffi.tuning(load_policy=policy):
            got = case(lars, _ffi)
        if ref is None:
            ref = got
        assert got.keys() == ref.keys()
        for k in ref:
            assert got[k] == ref[k], (policy, k)
    assert _ffi.get_tuning("load_policy") == 0
