"""Zone margins on the device (DESIGN.md "Zone margins", csrc/zone_margin.hip): lars_d_zone_shrink at its device entry and
``shrink_zones`` against the model (zone_margin_model.py), bytes for bytes, and ``zonal_statistics`` and
``process_image_zones`` of ``Shrunk(zones, margin)`` against the same call on ``shrink_zones``'s raster, for the three kinds of zones.

The sizes follow the kernels' own constants, restated here: a column segment is ZM_SEG rows, or r = floor(margin) rows where that is
more; a row stretch is ZM_TILE columns with r columns of halo on either side."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import lars_image_processing_amd as lars
import masked_cases as mc
import zone_margin_model as zm
from lars_image_processing_amd import _ffi

pytestmark = pytest.mark.gpu

ZM_SEG = 32
ZM_TILE = 256
MARGINS = (1, math.sqrt(2), 2.9, 3, 7.1, 31, 254)
WIDTHS = {1: np.uint8, 2: np.uint16, 4: np.int32}


class Device:
    """The three device buffers of lars_d_zone_shrink, kept and grown between calls."""

    def __init__(self):
        self.room, self.labels, self.g, self.out = 0, None, None, None

    def load(self, lab):
        lab = np.ascontiguousarray(lab)
        assert lab.dtype in WIDTHS.values()
        if lab.nbytes > self.room:
            for buf in (self.labels, self.g, self.out):
                if buf:
                    buf.free()
            self.room = max(lab.nbytes, 1 << 16)
            self.labels, self.g, self.out = (_ffi.DeviceBuffer(self.room) for _ in range(3))
        self.labels.upload(lab)
        self.lab = lab

    def run(self, m2):
        """The labels loaded last, shrunk by ``m2``."""
        (h, w), lab = self.lab.shape, self.lab
        _ffi.call("lars_d_zone_shrink", C.c_void_p(self.labels.ptr), lab.dtype.itemsize, h, w, int(m2), C.c_void_p(self.g.ptr), C.c_void_p(self.out.ptr), None)
        return np.array(self.out.download(lab.dtype, (h, w)))

    def shrink(self, lab, m2):
        self.load(lab)
        got = self.run(m2)
        assert self.labels.download(self.lab.dtype, self.lab.shape).tobytes() == self.lab.tobytes()       # the labels themselves are only read
        return got


@pytest.fixture(scope="module")
def device():
    return Device()


def both_ways(device, lab, margin, d2=None, n_zones=None):
    """The model's shrunk labels, after the device entry and ``shrink_zones`` have both been held against them."""
    m2 = zm.margin2(margin)
    want = zm.shrink(lab, m2, d2)
    assert device.shrink(lab, m2).tobytes() == want.tobytes(), ("lars_d_zone_shrink", lab.shape, margin)
    got = lars.shrink_zones(lab, margin, n_zones=n_zones)
    assert got.dtype == lab.dtype and got.tobytes() == want.tobytes(), ("shrink_zones", lab.shape, margin)
    return want


# ---------------------------------------------------------------------------
# D2 itself: every small size, every m2 of 0 .. 50
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("h", range(1, 41))
def test_every_size_and_every_margin2_up_to_50(device, h):
    """H x W for every W of 1 .. 40, pixel noise and blocks of labels 0 .. 3, the label width taking turns: the device entry at every
    m2 of 0 .. 50, ``shrink_zones`` at a margin with that m2."""
    rng = np.random.default_rng(4100 + h)
    for w in range(1, 41):
        for blocky in (False, True):
            lab = zm.fuzz_labels(rng, h, w, blocky).astype(WIDTHS[(1, 2, 4)[(h + w + blocky) % 3]])
            if not lab.any():
                lab[0, 0] = 1
            d2 = zm.d2_scipy(lab)
            device.load(lab)
            for m2 in range(51):
                want = zm.shrink(lab, m2, d2)
                assert device.run(m2).tobytes() == want.tobytes(), (h, w, blocky, m2)
                margin = math.sqrt(m2)
                assert zm.margin2(margin) == m2
                assert lars.shrink_zones(lab, margin).tobytes() == want.tobytes(), (h, w, blocky, margin)


# ---------------------------------------------------------------------------
# the kernels' tiles, segments and halos
# ---------------------------------------------------------------------------
def patchwork(rng, h, w, r, dtype):
    """Blocks of labels 0 .. 3 of r + 1 to 3 r + 9 pixels on a side, cut by the raster's edge, with a sprinkle of single pixels of
    another label, fewer the larger the margin: something goes at every margin and, raster permitting, something stays."""
    by, bx = (int(v) for v in rng.integers(r + 1, 3 * r + 10, 2))
    coarse = rng.integers(0, 4, (-(-h // by) + 1, -(-w // bx) + 1))
    oy, ox = int(rng.integers(0, by)), int(rng.integers(0, bx))
    lab = np.kron(coarse, np.ones((by, bx), dtype=np.int64))[oy:oy + h, ox:ox + w]
    dots = rng.random((h, w)) < min(0.002, 0.1 / (r * r + 1))
    lab = np.where(dots, (lab + 1) % 4, lab).astype(dtype)
    if not lab.any():
        lab[0, 0] = 1
    return lab


def straddling(size, r):
    return (size - 1, size, size + 1, size + r, 2 * size + 1)


@pytest.mark.parametrize("margin", MARGINS, ids=lambda m: f"{m:.3g}")
@pytest.mark.parametrize("axis", ["width", "height"])
def test_sizes_that_straddle_tiles_segments_and_halos(device, margin, axis):
    r = int(margin)
    size = ZM_TILE if axis == "width" else max(ZM_SEG, r)
    rng = np.random.default_rng(1000 * r + len(axis))
    for k, n in enumerate(straddling(size, r)):
        shape = (37, n) if axis == "width" else (n, 41)
        lab = patchwork(rng, *shape, r, WIDTHS[(1, 2, 4)[k % 3]])
        both_ways(device, lab, margin)


@pytest.mark.parametrize("margin", [2.9, 7.1, 31])
def test_several_tiles_and_segments_at_once(device, margin):
    r = int(margin)
    rng = np.random.default_rng(20 + r)
    lab = patchwork(rng, 2 * max(ZM_SEG, r) + 1, 2 * ZM_TILE + 1, r, np.uint16)
    want = both_ways(device, lab, margin)
    assert 0 < np.count_nonzero(want) < np.count_nonzero(lab)


# ---------------------------------------------------------------------------
# named shapes
# ---------------------------------------------------------------------------
def test_margins_below_1_remove_nothing_and_1_and_root_2_the_border_layers(device):
    from scipy.ndimage import binary_erosion
    rng = np.random.default_rng(5)
    lab = patchwork(rng, 60, 70, 6, np.uint8)
    for margin in (0, 0.5, math.nextafter(1.0, 0.0)):
        assert both_ways(device, lab, margin).tobytes() == lab.tobytes()
    cross, full = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool), np.ones((3, 3), bool)
    for margin, structure in ((1, cross), (math.nextafter(math.sqrt(2), 0.0), cross), (math.sqrt(2), full), (1.99, full)):
        layers = np.zeros_like(lab)
        for z in range(1, 4):                                      # border_value 1: the raster's edge is no border
            layers[binary_erosion(lab == z, structure, border_value=1)] = z
        assert both_ways(device, lab, margin).tobytes() == layers.tobytes(), margin


@pytest.mark.parametrize("label, dtype", [(255, np.uint8), (255, np.uint16), (256, np.uint16), (65535, np.uint16), (65535, np.int32), (65536, np.int32),
                                          (0x7FFFFFFF, np.int32)])
def test_large_labels_at_every_width(device, label, dtype):
    lab = np.zeros((21, 300), dtype=dtype)
    lab[2:19, 3:140] = label
    lab[4:19, 140:290] = label - 1                                  # shares an edge with the first, no background between
    for margin in (1, 3, 7.1):
        m2 = zm.margin2(margin)
        want = zm.shrink(lab, m2)
        assert device.shrink(lab, m2).tobytes() == want.tobytes()
        assert want.max() == label and (want == label - 1).any()
        if label <= 65535:
            assert lars.shrink_zones(lab, margin).tobytes() == want.tobytes()


def test_two_zones_that_share_an_edge_erode_each_other(device):
    lab = np.zeros((30, 40), dtype=np.uint8)
    lab[:, :20], lab[:, 20:] = 1, 2
    want = both_ways(device, lab, 3)
    assert (want[:, 17:23] == 0).all() and (want[:, :17] == 1).all() and (want[:, 23:] == 2).all()


def test_a_zone_with_a_hole_a_checkerboard_and_one_pixel_zones(device):
    ring = np.zeros((50, 60), dtype=np.uint16)
    ring[5:45, 5:55] = 7
    ring[20:30, 25:35] = 0
    want = both_ways(device, ring, 4)
    assert (want[16:34, 25:35] == 0).all() and (want[20:30, 21:39] == 0).all() and want[16, 21] == 7 and want[12, 12] == 7 and want[8, 30] == 0
    yy, xx = np.mgrid[0:33, 0:47]
    board = (1 + (yy + xx) % 2).astype(np.uint8)
    assert both_ways(device, board, 0.99).tobytes() == board.tobytes()
    assert not both_ways(device, board, 1).any()
    dots = np.zeros((19, 23), dtype=np.int32)
    dots[::3, ::4] = np.arange(1, 7 * 6 + 1).reshape(7, 6)
    assert both_ways(device, dots, 0.5).tobytes() == dots.tobytes()
    assert not both_ways(device, dots, 1).any()
    lone = np.array([[5]], dtype=np.uint8)                          # alone on its raster: nothing differs
    assert both_ways(device, lone, 254).tobytes() == lone.tobytes()


def test_a_zone_that_fills_the_raster_loses_nothing_at_254(device):
    for shape in ((1, 1), (1, 700), (300, 1), (270, 530)):
        full = np.full(shape, 3, dtype=np.uint8)
        assert both_ways(device, full, 254).tobytes() == full.tobytes()


def test_the_rasters_edge_is_no_border(device):
    lab = np.zeros((40, 50), dtype=np.uint8)
    lab[:25, :30] = 1                                               # in the corner: eroded on its two inner sides only
    want = both_ways(device, lab, 5)
    assert (want[:20, :25] == 1).all() and np.count_nonzero(want) == 20 * 25


def test_one_large_zone_at_254_saturates_the_column_distance(device):
    """600 x 300 inside 700 x 400: rows further than 254 from the zone's top and bottom do not exist, columns do; g saturates at
    255 only where the model's distance does not matter."""
    lab = np.zeros((400, 700), dtype=np.uint8)
    lab[50:350, 50:650] = 1
    assert not both_ways(device, lab, 254).any()
    want = both_ways(device, lab, 140)
    assert np.count_nonzero(want) == (300 - 280) * (600 - 280)
    tall = np.zeros((700, 900), dtype=np.uint8)
    tall[10:690, 20:880] = 2                                        # 680 x 860: a core further than 254 from every side survives
    want = both_ways(device, tall, 254)
    assert np.count_nonzero(want) == (680 - 508) * (860 - 508)


def test_a_column_300_tall(device):
    lab = np.zeros((300, 9), dtype=np.uint8)
    lab[:, 4] = 1
    assert both_ways(device, lab, 0.99).tobytes() == lab.tobytes()
    assert not both_ways(device, lab, 1).any()
    wide = np.zeros((300, 9), dtype=np.uint8)
    wide[:, 2:7] = 1
    want = both_ways(device, wide, 2)
    assert (want[:, 4] == 1).all() and np.count_nonzero(want) == 300


def test_labels_above_z_are_reported_as_today_and_erode_their_neighbours(device):
    lab = np.zeros((20, 30), dtype=np.uint8)
    lab[2:18, 2:15] = 1
    lab[2:18, 15:28] = 9                                            # above Z = 2
    lab[10, 20] = 2
    want = zm.shrink(lab, 4)
    assert device.shrink(lab, 4).tobytes() == want.tobytes() and (want[:, 13:17] == 0).all() and (want == 9).any()
    plane = np.linspace(-1, 1, lab.size, dtype=np.float32).reshape(lab.shape)
    img = mc.image(20, 30, 3)
    bad = int(np.count_nonzero(lab > 2))
    for margin in (None, 2, 254):                                   # at 254 every bad label would be gone before a later count
        zones = lab if margin is None else lars.Shrunk(lab, margin)
        with pytest.raises(ValueError, match=f"zonal_statistics: {bad} pixels have a label outside 0 .. 2"):
            lars.zonal_statistics(plane, zones, "NDVI", n_zones=2)
        with pytest.raises(ValueError, match=f"process_image_zones: {bad} pixels have a label outside 0 .. 2"):
            lars.process_image_zones(img, zones, n_zones=2)
    with pytest.raises(ValueError, match=f"shrink_zones: {bad} pixels have a label outside 0 .. 2"):
        lars.shrink_zones(lab, 254, n_zones=2)


def test_shrink_zones_of_polygons_is_the_shrunk_raster_of_rasterize_zones():
    polygons, shape = field_polygons(), FIELD
    raster = lars.rasterize_zones(polygons, shape)
    for margin in (0, 1, 2.9):
        got = lars.shrink_zones(polygons, margin, shape=shape)
        assert got.dtype == raster.dtype and got.tobytes() == zm.shrink(raster, zm.margin2(margin)).tobytes()
    t = (100.0, 0.5, 0.0, 2000.0, 0.0, -0.5)
    world = [[lars.to_world(np.asarray(ring, dtype=np.float64), t) for ring in (p if np.ndim(p[0]) == 2 else [p])] for p in polygons]
    assert lars.shrink_zones(world, 2.9, shape=shape, transform=t).tobytes() == zm.shrink(raster, 8).tobytes()


# ---------------------------------------------------------------------------
# through the calls
# ---------------------------------------------------------------------------
FIELD = (97, 130)


def field_polygons():
    """Plots with alleys between them, two that share an edge, one so thin that a margin of 2 leaves nothing of it."""
    plots = [[(6.0 + 30 * c, 5.0 + 22 * r), (31.0 + 30 * c, 6.5 + 22 * r), (30.0 + 30 * c, 23.5 + 22 * r), (5.0 + 30 * c, 22.0 + 22 * r)]
             for r in range(4) for c in range(4)]
    plots.append([(2.0, 93.2), (120.0, 93.2), (120.0, 96.4), (2.0, 96.4)])          # three rows thick
    plots.append([(31.0, 5.0), (35.0, 5.0), (35.0, 23.5), (30.0, 23.5)])            # fills the alley beside plot 0
    return plots


@functools.lru_cache(maxsize=None)
def field():
    """The three kinds of zones of one picture, the labels they stand for, and the picture and a plane whose zone sums are exact in
    any order: the plane's values are multiples of 2^-12, the picture's index values quotients of uint8 sums, multiples of 2^-33
    below 1 in float32 -- either way a zone of fewer than 2^14 pixels adds up without rounding in float64, so the mean, too, has
    the same bytes whichever order the device placed the values in."""
    polygons = field_polygons()
    raster = lars.rasterize_zones(polygons, FIELD)
    mask = raster > 0
    rng = np.random.default_rng(9)
    plane = (rng.integers(-4096, 4097, FIELD) / 4096).astype(np.float32)
    for a in (raster, mask, plane):
        a.setflags(write=False)
    return {"polygons": polygons, "raster": raster, "mask": mask, "plane": plane, "img": mc.image(*FIELD, 3)}


def kinds(valid=None):
    """name -> (zones of the call with labels wanted back, the labels they stand for, Z).  Regions are those of the mask under
    ``valid``: a pixel that does not count is never foreground."""
    f = field()
    regions = lars.label_regions(f["mask"] if valid is None else f["mask"] & valid)
    return {"raster": (f["raster"], f["raster"], len(f["polygons"])),
            "polygons": (lars.Polygons(f["polygons"], want_labels=True), f["raster"], len(f["polygons"])),
            "regions": (lars.Regions(mask=f["mask"], want_labels=True), regions["labels"], regions["n_regions"])}


def same_bytes(a, b, path=""):
    """Two results of the calls: every array and number with the same bytes, every dict with the same keys."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (path, set(a) ^ set(b))
        for key in a:
            same_bytes(a[key], b[key], f"{path}/{key}")
    elif isinstance(a, lars.Polygons):
        same_bytes(vars(a), vars(b), path)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            same_bytes(x, y, f"{path}[{k}]")
    elif a is None:
        assert b is None, path
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), path


def without(result, *keys):
    return {k: v for k, v in result.items() if k not in keys}


@pytest.mark.parametrize("margin", [1, 2.9])
@pytest.mark.parametrize("kind", ["raster", "polygons", "regions"])
def test_zonal_statistics_with_a_margin_is_the_call_on_the_shrunk_raster(kind, margin):
    f = field()
    valid = mc.image(*FIELD, 4, seed=3)[:, :, 3] > 40
    for kw in ({}, {"valid": valid, "want_hist": True}):
        zones, labels, nz = kinds(kw.get("valid"))[kind]
        shrunk = lars.shrink_zones(labels, margin, n_zones=nz)
        assert shrunk.tobytes() == zm.shrink(labels, zm.margin2(margin)).tobytes()
        want = lars.zonal_statistics(f["plane"], shrunk, "NDVI", n_zones=nz, **kw)
        got = lars.zonal_statistics(f["plane"], lars.Shrunk(zones, margin), "NDVI", **({"n_zones": nz} if kind == "raster" else {}), **kw)
        same_bytes(without(got, "labels", "regions"), want)
        if kind != "raster":
            assert got["labels"].tobytes() == shrunk.tobytes() and got["labels"].dtype == labels.dtype
        if kind == "regions":
            same_bytes(got["regions"], lars.zonal_statistics(f["plane"], zones, "NDVI", **kw)["regions"])
            assert (got["regions"]["area"] >= got["pixels"]).all()
    if margin == 2.9 and kind != "regions":
        gone = len(f["polygons"]) - 2                               # the thin plot: an empty zone, not a missing one
        assert got["pixels"][gone] == 0 and np.isnan([got[k][gone] for k in ("mean", "median", "min", "max", "coverage")]).all()
        assert len(got["zone"]) == nz and got["pixels"].sum() > 1000


@pytest.mark.parametrize("kind", ["raster", "polygons", "regions"])
def test_process_image_zones_with_a_margin_is_the_call_on_the_shrunk_raster(kind):
    f = field()
    margin = 2.9
    for kw in ({}, {"nodata": 9, "want_hist": True, "indices": ["NDVI", "NDWI"]}):
        img = f["img"].copy()
        img[:7] = 9
        zones, labels, nz = kinds(~(img == 9).all(axis=2) if "nodata" in kw else None)[kind]
        shrunk = lars.shrink_zones(labels, margin, n_zones=nz)
        want = lars.process_image_zones(img, shrunk, n_zones=nz, **kw)
        got = lars.process_image_zones(img, lars.Shrunk(zones, margin), **({"n_zones": nz} if kind == "raster" else {}), **kw)
        same_bytes(without(got, "zones"), without(want, "zones"))
        same_bytes(without(got["zones"], "labels", "regions"), want["zones"])
        if kind != "raster":
            assert got["zones"]["labels"].tobytes() == shrunk.tobytes()
        if kind == "regions":
            same_bytes(got["zones"]["regions"], lars.process_image_zones(img, zones, **kw)["zones"]["regions"])
    assert (got["zones"]["pixels"] == 0).any() and np.isnan(got["zones"]["NDVI"]["mean"][got["zones"]["pixels"] == 0]).all()


@pytest.mark.parametrize("kind", ["raster", "polygons", "regions"])
def test_no_margin_and_margin_0_change_nothing(kind):
    f = field()
    zones, _, nz = kinds()[kind]
    extra = {"n_zones": nz} if kind == "raster" else {}
    plain = lars.zonal_statistics(f["plane"], zones, "NDVI", want_hist=True, **extra)
    picture = lars.process_image_zones(f["img"], zones, want_hist=True, **extra)
    for margin in (None, 0, 0.0):
        same_bytes(lars.zonal_statistics(f["plane"], lars.Shrunk(zones, margin), "NDVI", want_hist=True, **extra), plain)
        same_bytes(lars.process_image_zones(f["img"], lars.Shrunk(zones, margin), want_hist=True, **extra), picture)
    # and a margin below 1 runs the kernels and removes nothing
    same_bytes(lars.zonal_statistics(f["plane"], lars.Shrunk(zones, 0.5), "NDVI", want_hist=True, **extra), plain)


def test_the_library_refuses_outlines_with_a_margin_and_a_margin_out_of_range():
    """Behind the host checks of ``zones.py``: the C entry points answer the same, and shrink nothing."""
    f = field()
    lab, out = np.ascontiguousarray(f["raster"]), np.zeros_like(f["raster"])
    h, w = lab.shape
    for m2 in (-1, -2, 64517):
        with pytest.raises(_ffi.LarsError, match="margin2 must be 0 to 64516"):
            _ffi.call("lars_h_shrink_zones", _ffi.ptr(lab), 1, h, w, 18, m2, _ffi.ptr(out), None)
    assert not out.any()
    dev = Device()
    with pytest.raises(_ffi.LarsError, match="margin2 must be 0 to 64516"):
        dev.shrink(lab, 64517)
    _ffi.call("lars_h_shrink_zones", _ffi.ptr(lab), 1, h, w, 18, 64516, _ffi.ptr(out), None)
    assert out.tobytes() == zm.shrink(lab, 64516).tobytes()
