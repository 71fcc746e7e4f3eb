"""Device PNG encoder (csrc/png.hip: api.encode_png, process_image(want_png=...), the driver's png_encoder="device").

Every file is checked by test_png_cpu.check_png, which does not rely on Pillow alone: chunk CRCs, zlib inflate (stream +
Adler-32), filter bytes and filtered rows against libpng's heuristic in NumPy, the rows un-filtered in NumPy, then
Image.open must give the input back.
"""
import io
import zipfile

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api, driver, tiffio
from test_png_cpu import SEG, bound, check_png, deflate_blocks, filter_rows

pytestmark = pytest.mark.gpu


def field_1f(n, beta, seed):
    """Seeded 1/f^beta field in [-1, 1] (a stand-in for an NDVI map: smooth for large beta, rough for small)."""
    rng = np.random.default_rng(seed)
    fy = np.fft.fftfreq(n)[:, None]
    fx = np.fft.rfftfreq(n)[None, :]
    f = np.sqrt(fx * fx + fy * fy)
    f[0, 0] = 1.0
    spec = (rng.normal(size=f.shape) + 1j * rng.normal(size=f.shape)) / f ** beta
    spec[0, 0] = 0
    x = np.fft.irfft2(spec, s=(n, n))
    return (x / np.abs(x).max()).astype(np.float32)


def colormap_picture(n, beta, seed=7, index_type="NDVI"):
    return lars.colorize_index(field_1f(n, beta, seed), index_type)


def pic(h, w, c, kind="random", seed=0):
    rng = np.random.default_rng(seed)
    shape = (h, w) if c == 1 else (h, w, c)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "constant":
        return np.full(shape, 77, dtype=np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        base = (xx * 3 + yy * 5) % 256
        return (base if c == 1 else np.stack([(base + 40 * k) % 256 for k in range(c)], axis=-1)).astype(np.uint8)
    raise ValueError(kind)


PALETTE = np.random.default_rng(11).integers(0, 256, (256, 4), dtype=np.uint8)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 300), (300, 1), (1, 5000), (5000, 1)])
def test_degenerate_shapes(h, w, c):
    for kind in ("random", "constant", "ramp"):
        a = pic(h, w, c, kind, seed=h * 7 + w)
        check_png(api.encode_png(a), a)


def test_every_width_1_to_67_every_mode():
    for w in range(1, 68):
        for c in (1, 3, 4):
            a = pic(5, w, c, "ramp" if w % 2 else "random", seed=w)
            check_png(api.encode_png(a), a)
        e = pic(3, w, 1, "random", seed=1000 + w)
        check_png(api.encode_png(e, PALETTE), e, palette=PALETTE)


@pytest.mark.parametrize("h,w,c", [(40, 3000, 4),      # 12001-byte rows: segment boundaries fall inside rows
                                   (9, 10000, 4),      # one row (40001 bytes) longer than a segment
                                   (33, 993, 1),       # exactly one segment of filtered bytes (33 * 994 = 32802 > SEG)
                                   (32, 1023, 1)])     # 32 * 1024 = 32768: exactly one segment
def test_rows_and_segments(h, w, c):
    for kind in ("ramp", "random", "constant"):
        a = pic(h, w, c, kind, seed=h + w)
        b = api.encode_png(a)
        check_png(b, a)
        assert len(b) <= bound(h, w, c)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_random_noise_takes_the_stored_blocks(c):
    a = pic(300, 257, c, "random", seed=c)
    b = api.encode_png(a)
    check_png(b, a)
    assert len(b) <= bound(300, 257, c)
    blocks = deflate_blocks(b)
    assert blocks and set(blocks) == {0}, blocks              # every segment stored: at most raw size + a small bound
    nseg = -(-300 * (257 * c + 1) // SEG)
    assert len(b) <= 300 * (257 * c + 1) + 17 * nseg + 6 + 33 + 12


def test_runs_longer_than_258_bytes():
    a = np.zeros((50, 700, 3), dtype=np.uint8)
    a[:, 300:] = (10, 200, 30)
    a[20:30] = 255
    b = api.encode_png(a)
    check_png(b, a)
    assert len(b) < a.nbytes // 7                             # literal-only coding: about one bit per filtered byte


def every_filter_image():
    yy, xx = np.mgrid[0:32, 0:61]
    parts = [np.zeros((4, 61)), (xx * 7 + yy * 3) % 256, 128 + 100 * np.sin(xx / 5.0) * np.cos(yy / 7.0),
             xx * 2 + yy * 2 + np.random.default_rng(1).integers(0, 20, (32, 61))]
    return np.concatenate(parts).astype(np.uint8)


def test_every_filter_wins_some_row():
    a = every_filter_image()
    choice = check_png(api.encode_png(a), a)
    assert set(choice.tolist()) == {0, 1, 2, 3, 4}
    rgb = np.stack([a, a[:, ::-1], a], axis=-1)
    choice = check_png(api.encode_png(rgb), rgb)
    assert len(set(choice.tolist())) >= 4


def test_palette_mode_of_colormap_entries():
    x = field_1f(256, 1.2, 3)
    e = np.minimum(((x + 1.0) * 128.0).astype(np.int32), 255).astype(np.uint8)
    lut = api.colormap_lut("RdYlGn")
    b = api.encode_png(e, lut)
    check_png(b, e, palette=lut)
    small = PALETTE[:17]
    e17 = (e % 17).astype(np.uint8)
    check_png(api.encode_png(e17, small), e17, palette=small)


@pytest.mark.parametrize("beta", [1.5, 1.0])
def test_colormap_pictures_of_1f_fields(beta):
    a = colormap_picture(512, beta, seed=int(beta * 10))
    check_png(api.encode_png(a), a)
    rgb = np.ascontiguousarray(a[:, :, :3])
    check_png(api.encode_png(rgb), rgb)


def test_4096_square_rgba():
    a = colormap_picture(4096, 1.0, seed=5)
    b = api.encode_png(a)
    check_png(b, a)
    assert len(b) <= bound(4096, 4096, 4)


def test_deterministic():
    for a in (colormap_picture(1024, 1.2, seed=9), pic(200, 333, 3, "random", 4), every_filter_image()):
        first = api.encode_png(a)
        for _ in range(3):
            assert api.encode_png(a) == first


def test_seeded_fuzz():
    rng = np.random.default_rng(2024)
    for case in range(100):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        c = int(rng.choice([1, 3, 4]))
        kind = rng.choice(["random", "constant", "ramp", "runs"])
        if kind == "runs":
            levels = rng.integers(0, 256, 4, dtype=np.uint8)
            a = levels[rng.integers(0, 4, (h, w) if c == 1 else (h, w, c)) * (rng.random() < 0.5)]
            a = np.sort(a, axis=1).astype(np.uint8)
        else:
            a = pic(h, w, c, str(kind), seed=case)
        if c == 1 and case % 3 == 0:
            n = int(rng.integers(1, 257))
            pal = rng.integers(0, 256, (n, 4), dtype=np.uint8)
            a = (a % n).astype(np.uint8)
            check_png(api.encode_png(a, pal), a, palette=pal)
        else:
            check_png(api.encode_png(a), a)


@pytest.mark.parametrize("beta", [1.5, 1.0])
def test_size_against_pillow_level1(beta):
    """2048 x 2048 colormap pictures (smooth and rough 1/f fields): at most 1.15 x Pillow's compress_level=1 file."""
    a = colormap_picture(2048, beta)
    b = api.encode_png(a)
    check_png(b, a, unfilter_limit=0)
    ref = io.BytesIO()
    Image.fromarray(a, "RGBA").save(ref, "PNG", compress_level=1)
    assert len(b) <= 1.15 * ref.tell(), (len(b), ref.tell())


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------
def _decode(b):
    return np.asarray(Image.open(io.BytesIO(b)))


def test_process_image_want_png_matches_the_rgba_route():
    img = np.random.default_rng(8).integers(0, 256, (301, 517, 3), dtype=np.uint8)
    host = api.process_image(img, want_arrays=False, want_rgba=True, want_hist=True)
    dev = api.process_image(img, want_arrays=False, want_png=True, want_hist=True)
    pal = api.process_image(img, want_arrays=False, want_png="palette")
    assert np.array_equal(dev["corrected"], host["corrected"])
    for t in ("NDVI", "GNDVI", "NDWI"):
        rgba = host["indices"][t]["rgba"]
        check_png(dev["indices"][t]["png"], rgba, unfilter_limit=0)
        assert dev["indices"][t]["stats"] == host["indices"][t]["stats"]
        assert np.array_equal(dev["indices"][t]["hist"], host["indices"][t]["hist"])
        lut = api.colormap_lut(api._colormap_for(t))
        entries = api.process_image(img, indices=[t], want_arrays=False, want_entries=True)["indices"][t]["entry"]
        check_png(pal["indices"][t]["png"], entries, palette=lut, unfilter_limit=0)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(pal["indices"][t]["png"])).convert("RGBA")), rgba)
        assert host["indices"][t]["png"] is None


def test_process_image_want_png_with_arrays_and_medians():
    img = np.random.default_rng(9).integers(0, 256, (64, 80, 3), dtype=np.uint8)
    dev = api.process_image(img, indices=["NDWI"], want_png=True)
    ref = api.process_image(img, indices=["NDWI"])
    assert np.array_equal(dev["indices"]["NDWI"]["index"], ref["indices"]["NDWI"]["index"])
    assert dev["indices"]["NDWI"]["stats"] == ref["indices"]["NDWI"]["stats"]
    check_png(dev["indices"]["NDWI"]["png"], lars.colorize_index(ref["indices"]["NDWI"]["index"], "NDWI"))


@pytest.mark.parametrize("lut_format", ["png", "png8"])
def test_batch_process_device_encoder_same_pixels(tmp_path, lut_format):
    src = tmp_path / "in"
    src.mkdir()
    rng = np.random.default_rng(1)
    for i in range(3):
        tiffio.write_tiff(src / f"s{i}.tif", rng.integers(0, 256, (120 + i, 170, 3), dtype=np.uint8))
    kw = dict(process_wb=True, process_ndvi=True, process_gndvi=True, process_ndwi=True, verbose=False, lut_format=lut_format,
              workers=2)
    a = driver.batch_process(src, tmp_path / "pil", **kw)
    b = driver.batch_process(src, tmp_path / "dev", png_encoder="device", **kw)
    assert a == b
    files = sorted(p.relative_to(tmp_path / "pil") for p in (tmp_path / "pil").rglob("*") if p.is_file())
    assert files == sorted(p.relative_to(tmp_path / "dev") for p in (tmp_path / "dev").rglob("*") if p.is_file())
    assert any(str(f).endswith(".png") for f in files)
    for f in files:
        pa, pb = Image.open(tmp_path / "pil" / f), Image.open(tmp_path / "dev" / f)
        assert pa.mode == pb.mode, f
        assert np.array_equal(np.asarray(pa), np.asarray(pb)), f
        if pa.mode == "P":
            assert np.array_equal(np.asarray(pa.convert("RGBA")), np.asarray(pb.convert("RGBA"))), f
        if f.suffix == ".png":
            check_png((tmp_path / "dev" / f).read_bytes(), np.asarray(pb), palette=_palette_of(pb) if pb.mode == "P" else None,
                      unfilter_limit=0)


def _palette_of(im):
    """RGBA palette of a P image as written (PLTE + tRNS)."""
    rgb = np.frombuffer(im.palette.tobytes(), np.uint8).reshape(-1, 3)
    alpha = np.frombuffer(im.info["transparency"], np.uint8)
    return np.concatenate([rgb[:alpha.size], alpha[:, None]], axis=1)


@pytest.mark.parametrize("cached", [False, True])
def test_export_zip_device_encoder_same_pixels(cached):
    img = np.random.default_rng(4).integers(0, 256, (130, 190, 3), dtype=np.uint8)
    corrected = api.fix_white_balance(img) if cached else None
    za = zipfile.ZipFile(io.BytesIO(driver.export_zip(img, ["NDVI", "NDWI"], corrected)))
    zb = zipfile.ZipFile(io.BytesIO(driver.export_zip(img, ["NDVI", "NDWI"], corrected, png_encoder="device")))
    assert za.namelist() == zb.namelist() == ["white_balanced.png", "NDVI_visualization.png", "NDWI_visualization.png"]
    for name in za.namelist():
        a, b = _decode(za.read(name)), _decode(zb.read(name))
        assert Image.open(io.BytesIO(za.read(name))).mode == Image.open(io.BytesIO(zb.read(name))).mode
        assert np.array_equal(a, b), name
        check_png(zb.read(name), b, unfilter_limit=0)


def test_device_entry_point():
    """lars_d_encode_png_u8 on device buffers, with the library stream; the length is a device int64."""
    import ctypes as C
    a = colormap_picture(300, 1.3)
    h, w, c = a.shape
    cap = bound(h, w, c)
    d_in, d_out = _ffi.DeviceBuffer(a.nbytes), _ffi.DeviceBuffer(cap)
    d_scr, d_len = _ffi.DeviceBuffer(_ffi.load().lars_png_scratch_bytes(h, w, c)), _ffi.DeviceBuffer(8)
    try:
        d_in.upload(a)
        _ffi.call("lars_d_encode_png_u8", C.c_void_p(d_in.ptr), h, w, c, None, 0, C.c_void_p(d_out.ptr), cap, C.c_void_p(d_len.ptr),
                  C.c_void_p(d_scr.ptr), None)
        _ffi.call("lars_synchronize", None)
        n = int(d_len.download(np.int64, (1,))[0])
        b = d_out.download(np.uint8, (n,)).tobytes()
        check_png(b, a)
        assert b == api.encode_png(a)
        with pytest.raises(_ffi.LarsError):
            _ffi.call("lars_d_encode_png_u8", C.c_void_p(d_in.ptr), h, w, c, None, 0, C.c_void_p(d_out.ptr), cap - 1,
                      C.c_void_p(d_len.ptr), C.c_void_p(d_scr.ptr), None)
    finally:
        for d in (d_in, d_out, d_scr, d_len):
            d.free()


def test_filter_choice_matches_heuristic_on_colormaps():
    a = colormap_picture(256, 1.0, seed=1)
    f, want = filter_rows(a.reshape(256, -1), 4)
    got = check_png(api.encode_png(a), a)
    assert np.array_equal(got, want)
