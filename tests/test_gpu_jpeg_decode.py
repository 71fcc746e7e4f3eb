"""decode_jpeg / thumbnail_jpeg / jpeg_decoder="device" on the GPU: every array equals Pillow's, byte for byte."""
import io
import sys
import threading
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import lars_image_processing_amd as lars
from lars_image_processing_amd import _ffi, api, driver, tiffio

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_model  # noqa: E402
from jpeg_gpu_common import device_entry_point_with_guards, get_bits, same, subseq_bits  # noqa: E402,F401
from test_jpeg_decode_cpu import TABLE, find, jpeg, picture, want  # noqa: E402

pytestmark = pytest.mark.gpu


def one_over_f(h, w, channels, seed):
    """1/f content as tools/pngbench.py makes it: what a photograph's spectrum looks like."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    amp = 1.0 / np.maximum(np.hypot(fy, fx), 1.0 / max(h, w))
    planes = []
    for _ in range(channels):
        x = np.fft.irfft2(np.fft.rfft2(rng.standard_normal((h, w))) * amp, (h, w))
        planes.append(((x - x.min()) / (x.max() - x.min()) * 255).astype(np.uint8))
    return planes[0] if channels == 1 else np.dstack(planes)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_table_equals_pillow(name):
    same(TABLE[name])


@pytest.mark.parametrize("restart", [None, "rows", "one"])
@pytest.mark.parametrize("kind", ["1/f", "noise q100", "flat"])
@pytest.mark.parametrize("shape", [(1536, 2048), (4096, 4096)])
def test_large_files(shape, kind, restart):
    h, w = shape
    if kind == "1/f":
        img, save = one_over_f(h, w, 3, seed=h), {}
    elif kind == "noise q100":
        img, save = picture("noise", h, w, "RGB", seed=3), {"quality": 100}
    else:
        img, save = picture("flat", h, w, "RGB"), {}          # every block is a DC code and EOB
    if restart == "rows":
        save["restart_marker_rows"] = 1
    elif restart == "one":
        save["restart_marker_blocks"] = 1
    same(jpeg(img, **save))


def test_large_gray_and_444():
    same(jpeg(one_over_f(1536, 2048, 1, seed=9)))
    same(jpeg(one_over_f(1000, 1500, 3, seed=10), subsampling=0, quality=95))
    same(jpeg(one_over_f(1001, 1499, 3, seed=11), subsampling=1, optimize=True))


SUBSEQ_FILES = [n for n in sorted(TABLE) if "33x47" in n or "150x301" in n or "17x33" in n]


@pytest.mark.parametrize("bits", [32, 33, 37, 61, 100, 257, 1000, None])
def test_results_do_not_depend_on_the_subsequence_length(subseq_bits, bits):
    """The synchronisation logic, not luck: at the minimum (32 bits: every lane starts inside a block), at odd lengths
    and at the default every file decodes to the same array."""
    if bits is not None:
        subseq_bits(bits)
        assert get_bits() == bits
    for name in SUBSEQ_FILES:
        same(TABLE[name])
    flat = picture("flat", 200, 300, "RGB")
    for save in ({}, {"restart_marker_blocks": 5}, {"subsampling": 0}):
        same(jpeg(flat, **save))
    same(jpeg(picture("flat", 64, 2000, "L")))


def test_a_stream_that_never_synchronises_by_itself(subseq_bits):
    """A flat picture at an odd subsequence length: lanes that start inside a block find valid codes for ever, so the
    true states have to travel border by border -- through the rounds and then the serial finish."""
    subseq_bits(33)
    same(jpeg(picture("flat", 1536, 2048, "RGB")))
    same(jpeg(picture("flat", 1536, 2048, "L")))


def test_device_entry_point_on_a_callers_stream_with_guards():
    b = jpeg(one_over_f(301, 517, 3, seed=4), restart_marker_blocks=7)
    device_entry_point_with_guards(b, want(b))


@pytest.mark.parametrize("mode", ["L", "RGB"])
@pytest.mark.parametrize("shape,size", [((1536, 2048), (800, 800)), ((1536, 2048), (2000, 1100)), ((700, 500), (400, 400)),
                                        ((300, 2500), (400, 400)), ((1000, 1000), (400, 400))])
@pytest.mark.parametrize("gap", [None, 1.0, 2.0, 3.0])
def test_thumbnail_jpeg_matches_pillow(mode, shape, size, gap):
    b = jpeg(one_over_f(shape[0], shape[1], 1 if mode == "L" else 3, seed=shape[0]))
    if api.jpeg_draft_scale((shape[1], shape[0]), size, gap) != 1:
        with pytest.raises(NotImplementedError, match="scale"):
            lars.thumbnail_jpeg(b, size, gap)
        return
    im = Image.open(io.BytesIO(b))
    im.thumbnail(size, Image.Resampling.LANCZOS, gap)
    assert im.decoderconfig in ((), (1, 0))                 # Pillow decoded at full scale too
    got = lars.thumbnail_jpeg(b, size, gap)
    assert got.shape == np.asarray(im).shape and got.tobytes() == np.asarray(im).tobytes()


def test_thumbnail_jpeg_small_file_and_scaled_files():
    b = jpeg(picture("smooth", 100, 120, "RGB"))
    assert np.array_equal(lars.thumbnail_jpeg(b), want(b))  # already fits
    for shape in ((2048, 2048), (4096, 4096)):
        with pytest.raises(NotImplementedError, match="scale"):
            lars.thumbnail_jpeg(jpeg(picture("flat", shape[0], shape[1], "L")))


def test_read_image_with_the_device_decoder(tmp_path):
    f = tmp_path / "a.jpg"
    f.write_bytes(jpeg(one_over_f(240, 320, 3, seed=2)))
    assert tiffio.read_image(f, jpeg_decoder="device").tobytes() == np.array(Image.open(f)).tobytes()


def test_batch_process_with_the_device_decoder(tmp_path, monkeypatch):
    decoded, lock = [], threading.Lock()
    real_decode = api.decode_jpeg

    def counting_decode(data):
        out = real_decode(data)
        with lock:
            decoded.append(out.shape)
        return out

    monkeypatch.setattr(api, "decode_jpeg", counting_decode)
    src = tmp_path / "in"
    src.mkdir()
    Image.fromarray(one_over_f(96, 128, 3, seed=1)).save(src / "a.jpg", quality=90)
    Image.fromarray(one_over_f(80, 64, 3, seed=2)).save(src / "b.jpeg", subsampling=0)
    Image.fromarray(one_over_f(64, 64, 3, seed=3)).save(src / "c.tif")
    Image.fromarray(one_over_f(64, 96, 3, seed=4)).save(src / "d.png")
    Image.fromarray(one_over_f(72, 88, 3, seed=5)).save(src / "e_progressive.jpg", progressive=True)
    Image.fromarray(one_over_f(48, 40, 3, seed=6)).save(src / "f_png_named.jpg", "PNG")   # not a JPEG: Pillow's
    res = {}
    for dec in ("pillow", "device"):
        out = tmp_path / dec
        res[dec] = driver.batch_process(src, out, process_wb=True, process_ndvi=True, verbose=False, jpeg_decoder=dec)
        assert sorted(decoded) == ([] if dec == "pillow" else [(80, 64, 3), (96, 128, 3)]), (dec, decoded)
    assert set(res["pillow"]) == set(res["device"])
    for k, v in res["pillow"].items():
        assert not isinstance(v, Exception), (k, v)
        assert v == res["device"][k], k
    files = sorted(p.relative_to(tmp_path / "pillow") for p in (tmp_path / "pillow").rglob("*") if p.is_file())
    assert files and files == sorted(p.relative_to(tmp_path / "device") for p in (tmp_path / "device").rglob("*") if p.is_file())
    for f in files:
        assert (tmp_path / "pillow" / f).read_bytes() == (tmp_path / "device" / f).read_bytes(), f


def damaged_entropy_files():
    """A handful of fixed files whose entropy data is damaged, each confirmed as damaged by the sequential model."""
    good = jpeg(one_over_f(64, 96, 3, seed=12), quality=90)
    eoff = find(good, 0xDA)[0] + 2 + find(good, 0xDA)[1]
    elen = len(good) - 2 - eoff
    out = {"truncated after the first third": good[:eoff + elen // 3]}
    # one byte in the middle replaced: the first position from the middle on whose change the sequential decoder refuses
    for pos in range(eoff + elen // 2, eoff + elen // 2 + 200):
        if 0xFF in (good[pos - 1], good[pos], good[pos + 1]) or good[pos] ^ 0x55 == 0xFF:
            continue
        bad = good[:pos] + bytes([good[pos] ^ 0x55]) + good[pos + 1:]
        try:
            jpeg_model.decode(bad)
        except ValueError:
            out["one byte replaced"] = bad
            break
    with_rst = jpeg(one_over_f(64, 96, 3, seed=13), quality=90, restart_marker_blocks=4)
    third = with_rst.index(b"\xff\xd2")
    out["a restart marker removed"] = with_rst[:third] + with_rst[third + 2:]
    out["a restart marker out of sequence"] = with_rst[:third] + b"\xff\xd5" + with_rst[third + 2:]
    return good, out


def test_damaged_entropy_data_raises_value_error():
    good, files = damaged_entropy_files()
    assert sorted(files) == ["a restart marker out of sequence", "a restart marker removed", "one byte replaced",
                             "truncated after the first third"]
    for name, b in files.items():
        assert lars.jpeg_info(b)["supported"], name         # the host sees nothing wrong with the structure
        with pytest.raises(ValueError):                     # the sequential decoder on the CPU first: damaged as the name says
            jpeg_model.decode(b)
    for name, b in files.items():                           # each file once
        with pytest.raises(ValueError, match="restart marker" if "restart" in name else "entropy data"):
            lars.decode_jpeg(b)
        same(good)                                          # and the next good file decodes correctly afterwards


def test_threads_decode_at_once():
    files = [jpeg(one_over_f(200 + 13 * k, 300 - 7 * k, 3 if k % 2 else 1, seed=20 + k), subsampling=k % 3 if k % 2 else -1,
                  restart_marker_blocks=k % 4) for k in range(8)]
    out = [None] * 8

    def run(k):
        for _ in range(3):
            out[k] = lars.decode_jpeg(files[k])

    ts = [threading.Thread(target=run, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(8):
        assert out[k].tobytes() == want(files[k]).tobytes()
