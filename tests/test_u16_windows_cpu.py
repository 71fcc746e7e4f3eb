"""The model of the uint16 value-window pre-pass (tests/u16_window_model.py) and the inputs built from it
(tests/u16_window_cases.py), checked without a GPU: the inputs are what they claim to be before a device sees them."""
import warnings

import numpy as np
import pytest

import u16_window_cases as cases
import u16_window_model as model


@pytest.mark.parametrize("shape,nsampled", [((511, 513), 1), ((509, 513), 1), ((510, 513), 1), ((512, 513), 2), ((512, 768), 2),
                                             ((1024, 513), 3), ((1023, 515), 3)])
def test_sampled_pixels_are_what_the_kernels_loop_reads(shape, nsampled):
    """k_u16_sample12: sampled stretch i covers quads i * 64 * 1024 + (0..1023), those below npix >> 2 only."""
    npix = shape[0] * shape[1]
    nquads = npix >> 2
    pos = model.sampled_pixels(npix)
    want = []                                                   # the loop as written, quad by quad
    for sidx in range(nsampled + 2):
        for tid in range(1024):
            q = sidx * 64 * 1024 + tid
            if q < nquads:
                want += [4 * q, 4 * q + 1, 4 * q + 2, 4 * q + 3]
    assert pos.tolist() == want
    assert model.launch_geometry(1, npix)[1] == nsampled
    full = (nsampled - 1) * 4096
    last = min(nquads - (nsampled - 1) * 65536, 1024) * 4
    assert pos.size == full + last and pos[0] == 0 and pos[-1] == (nsampled - 1) * 262144 + last - 1
    assert pos[-1] < nquads * 4 <= npix                          # the npix & 3 tail pixels are never sampled
    assert model.takes_window_route(1, npix)
    assert model.takes_window_route(2, npix) == (npix % 4 == 0)


def test_window_route_floor_and_the_two_in_flight_batch():
    assert not model.takes_window_route(1, 64512) and model.takes_window_route(1, 4 * 64513)      # cap = ceil(npix / 4 / 1024) >= 64
    assert not model.takes_window_route(1, 4 * 64512)
    npix = cases.H_SHAPE[0] * cases.H_SHAPE[1]
    assert cases.smallest_two_in_flight() == 1024                 # one workgroup per tile, two sampled stretches
    assert model.launch_geometry(1024, npix) == (1, 2) and model.launch_geometry(1023, npix) == (2, 2)
    assert model.launch_geometry(512, 524288 + 4) == (2, 3) and model.launch_geometry(10, 512 * 768) == (96, 2)
    assert model.launch_geometry(32, 8192 * 8192) == (32, 256)    # the benchmark's batch is the other one that reaches the branch


def test_windows_of_the_three_level_design():
    """The arithmetic of k_u16_window on a subsample of 8192 with 10 % / 80 % / 10 % on three values."""
    npix = cases.H * cases.W
    seen = cases.levels(cases.nseen(npix), 10000, 30000, 50000, np.random.default_rng(0))
    assert cases.seen_windows(npix, seen) == ((9984, 48), (49984, 48))
    ch = cases.compose(npix, seen, np.zeros(npix - seen.size, np.int64))
    assert model.windows(ch, test_wrong=True) == ((0, 16), (0, 16))
    assert model.ranks(npix) == ([7864, 7865, 385350, 385351], [393215 * 0.02 - 7864, 393215 * 0.98 - 385350])


def all_cases():
    return [cases.small_case(n) for n in cases.SMALL_NAMES] + [cases.case_h()]


@pytest.fixture(scope="module")
def built():
    return {c.name: c for c in all_cases()}


@pytest.mark.parametrize("name", cases.SMALL_NAMES + ("h-two-in-flight",))
def test_case_yields_the_verdict_it_claims(built, name):
    case = built[name]
    assert len(case.claims) == len(case.tiles)
    for i, tile in enumerate(case.tiles):
        assert model.tile_verdicts(tile) == tuple(case.claims[i]), (name, i)
        assert model.tile_flag(tile) == case.flags[i]
        assert model.takes_window_route(case.repeat or len(case.tiles), tile.shape[0] * tile.shape[1])


@pytest.mark.parametrize("name", cases.SMALL_NAMES + ("h-two-in-flight",))
def test_case_percentiles_from_its_order_statistics_equal_numpy(built, name):
    case = built[name]
    for i, tile in enumerate(case.tiles):
        for c in range(3):
            ch = tile[..., c].ravel()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = [float(v) for v in np.percentile(tile[:, :, c].astype(np.float32), (2, 98))]
            assert model.percentiles(ch) == want, (name, i, c)
    for (i, c, k), value in case.expect.items():
        # what the case's description states, to the digits it states (the weight of rank 7864 is 0.3 + 2e-13, not 0.3)
        assert round(model.percentiles(case.tiles[i][..., c].ravel())[k], 6) == value


def test_what_the_cases_say_about_themselves(built):
    """The properties the constructions rest on, beyond the verdicts."""
    a = built["a-hidden-tails"].tiles[0]
    for c in range(3):
        (l0, w0), (l1, w1) = model.windows(a[..., c].ravel())
        vals = model.order_statistics(a[..., c].ravel())
        assert l0 == 0 and w0 and vals[0] >= l0 + w0 and vals[3] >= l1 + w1        # both marks lie above what the subsample saw
    b = built["b-straddle"]
    assert model.order_statistics(b.tiles[0][..., 0].ravel()) == [10000, 30000, 50000, 50000]
    assert model.order_statistics(b.tiles[1][..., 0].ravel())[:2] == [10000, 10000]
    assert int((b.tiles[1][..., 0] == 10000).sum()) - int((b.tiles[0][..., 0] == 10000).sum()) == 1      # ONE more 10000
    assert int((b.tiles[3][..., 0] == 50000).sum()) - int((b.tiles[2][..., 0] == 50000).sum()) == 1
    assert b.flags == [1, 0, 1, 0]
    e = built["e-mixed-batch"]
    assert e.flags == [0, 1, 0, 1, 0, 1] and model.windows(e.tiles[3][..., 1].ravel())[0] == (0, 0)
    d = built["d-one-channel"]
    assert all(d.flags) and sorted(sum(all(v) for v in tile) for tile in d.claims) == [2] * len(d.tiles)   # one channel only, every time
    nowin = [model.windows(d.tiles[i][..., c].ravel()) for i, c in ((-2, 0), (-1, 2))]
    assert nowin[0][0][1] == 0 and nowin[0][1][1] == 48 and nowin[1][1][1] == 0 and nowin[1][0][1] == 48
    # the windowless 2 % mark's order statistics lie where the 98 % mark's width, measured from 0, would catch them
    assert model.order_statistics(d.tiles[-2][..., 0].ravel())[:2] == [20, 20]
    h = built["h-two-in-flight"]
    assert h.repeat == 1024 and h.flags == [1, 0, 0, 1, 0]
    first, second = model.sampled_pixels(h.tiles.shape[1] * h.tiles.shape[2])[[0, 4096]]
    assert second == 262144 and (h.tiles[1].reshape(-1, 3)[first] != h.tiles[1].reshape(-1, 3)[second]).all()


@pytest.mark.parametrize("shape", cases.RAGGED)
def test_ragged_tile_is_a_hit_only_with_its_tail_counted(built, shape):
    npix = shape[0] * shape[1]
    k = npix & 3
    assert k == {511: 3, 509: 1, 510: 2}[shape[0]] and (npix // 4 + 1023) // 1024 == 64
    ch = built["f-ragged-%dx%d-hit" % shape].tiles[0][..., 1].ravel()
    (lo, wd), _ = model.windows(ch)
    tail, body = ch[npix - k:], ch[:npix - k]
    assert tail.max() < body.min()                              # the tail pixels hold the channel's smallest samples
    r0, r1 = model.ranks(npix)[0][:2]
    s = np.sort(ch)
    assert lo <= s[r0] == s[r1] == lo + wd - 1                    # inside, on the window's last value
    assert s[r1 + 1] >= lo + wd                                  # ... and the window's samples end there:
    dropped = np.sort(body)                                      # without the tail every rank reads k samples further up
    assert dropped[r0 + 1 - k] == lo + wd - 1 and dropped[r1] >= lo + wd and dropped[r1 - k + 1] >= lo + wd


def test_existing_ten_tiles_mix_hits_and_misses_by_the_model():
    """What the model says about the ten tiles of test_uint16_percentiles_one_pass_and_its_recount (tests/test_gpu_batch.py): which
    are flagged with the predicted windows, and which are NOT flagged with the windows [0, 16) of u16_hist_impl = 3."""
    tiles = cases.existing_ten_tiles()
    flags = [model.tile_flag(t) for t in tiles]
    assert flags == [1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    # tile 0 (uniform random): its green 2 % mark gets no window -- the subsample's ranks around it span more than 1024 values -- while
    # red and NIR get windows 880 and 976 wide; tile 9 (half the samples on one value): no window for any mark
    assert [model.windows(tiles[0][..., c].ravel())[0][1] for c in range(3)] == [880, 0, 976]
    assert all(model.windows(tiles[9][..., c].ravel()) == ((0, 0), (0, 0)) for c in range(3))
    assert [model.tile_flag(t, test_wrong=True) for t in tiles] == [1] * 10      # no tile has all its marks in [0, 16)
