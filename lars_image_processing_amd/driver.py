"""Directory driver: decode -> white balance -> indices -> files.

Mirrors ``backend-process.py:49-97`` (``process_image`` / ``batch_process``): same
directory layout (``white_balanced/<name>_wb.tif``, ``<INDEX>/<name>_<index>.png``), same
extension filter, same per-file ``try``/``print`` error policy -- but each image crosses PCIe
once (``lars_h_process_image``: white balance, all requested indices and their colormaps in one
upload) and decoding / encoding overlap the GPU work on a thread pool (PIL releases the GIL;
the library gives every thread its own stream and workspace).

The index pictures are the per-pixel RGBA images of the reference's colormaps at full resolution (RdYlGn / RdYlBu,
``vmin=-1, vmax=1``), produced by the fused kernel.  The reference's matplotlib figure (imshow + colorbar,
``backend-process.py:40-47``) is figure rendering and not part of this package.
"""
from __future__ import annotations

import contextlib
import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import api, codecs, nodata as nodata_rules
from ._ffi import INDEX_NAMES

EXTENSIONS = {".tif", ".tiff", ".png", ".jpg", ".jpeg"}      # backend-process.py:89
# zlib level of the per-pixel colormap PNGs: encoding, not the GPU, bounds the directory driver (a 2048x2048 RGBA map takes
# 1.2 s at Pillow's default level 6 and 0.6 s at level 1, for a smaller file on colormap images); same pixels either way
LUT_PNG_LEVEL = 1
PNG_ENCODERS = ("pillow", "device")
PNG_DECODERS = ("pillow", "device", "device+extended")
JPEG_DECODERS = ("pillow", "device")
TIFF_DECODERS = ("pillow", "device", "device+deflate")
TIFF_ENCODERS = ("pillow", "device", "device+deflate")
MATCHING = "+matching"                                       # the encoder values that turn the Deflate coder's string matching on:
PNG_ENCODERS_MATCHING = ("device" + MATCHING,)               # "device" and "device+deflate" inside codecs.deflate_matching()
TIFF_ENCODERS_MATCHING = ("device+deflate" + MATCHING,)


def _check_png_encoder(png_encoder):
    if png_encoder not in PNG_ENCODERS + PNG_ENCODERS_MATCHING:
        raise ValueError(f"png_encoder must be 'pillow' or 'device' ('device+matching' for Deflate with string matching), got {png_encoder!r}")


def _check_png_decoder(png_decoder):
    if png_decoder not in PNG_DECODERS:
        raise ValueError(f"png_decoder must be 'pillow', 'device' or 'device+extended', got {png_decoder!r}")


def _check_jpeg_decoder(jpeg_decoder):
    if jpeg_decoder not in JPEG_DECODERS:
        raise ValueError(f"jpeg_decoder must be 'pillow' or 'device', got {jpeg_decoder!r}")


def _check_tiff_decoder(tiff_decoder):
    if tiff_decoder not in TIFF_DECODERS:
        raise ValueError(f"tiff_decoder must be 'pillow', 'device' or 'device+deflate', got {tiff_decoder!r}")


def _check_tiff_encoder(tiff_encoder):
    if tiff_encoder not in TIFF_ENCODERS + TIFF_ENCODERS_MATCHING:
        raise ValueError(f"tiff_encoder must be 'pillow' or 'device' ('device+deflate' for Deflate strips, 'device+deflate+matching' for those with string matching), got {tiff_encoder!r}")


def _mask_options(nodata, alpha_mask, lut_format):
    """``nodata`` / ``alpha_mask`` as the keywords ``nodata.process_image_masked`` takes ({} = every pixel is picture)."""
    kw = {}
    if nodata is not None:
        kw["nodata"] = nodata
    if alpha_mask:
        kw["valid"] = "alpha"
    if kw and lut_format == "png8":
        raise ValueError(f"lut_format='png8' with nodata / alpha_mask: {nodata_rules.NO_PALETTE_WITH_MASK.split(':')[0]}; use 'png' or 'tiff'")
    return kw


def _mask_argument(mask_kw):
    """``_process_image``'s last argument, handed over only where a mask is set: without one the call is the one it always was."""
    return (mask_kw,) if mask_kw else ()


def _zones_argument(zones, zones_transform=None, regions=None, regions_geojson=False, zone_margin=None, regions_simplify=None):
    """``_process_image``'s ``zones`` (and ``zones_transform``, ``regions``, ``regions_geojson``, ``zone_margin``, ``regions_simplify``)
    keywords, handed over only where they are named: without them the call is the one it always was."""
    kw = {} if zones is None else {"zones": zones}
    if zones_transform is not None:
        kw["zones_transform"] = zones_transform
    if regions is not None:
        kw["regions"] = regions
    if regions_geojson:
        if regions is None:
            raise ValueError("regions_geojson writes the outlines of the regions: it goes with regions")
        kw["regions_geojson"] = True
    if zone_margin is not None:
        if zones is None and regions is None:
            raise ValueError("zone_margin shrinks the zones of the picture: it goes with zones or regions")
        if regions_geojson:
            raise ValueError("zone_margin and regions_geojson do not go together: outlines are traced from regions as found")
        kw["zone_margin"] = zone_margin
    if regions_simplify is not None:
        if not regions_geojson:
            raise ValueError("regions_simplify is the tolerance of the outlines in the GeoJSON: it goes with regions_geojson")
        kw["regions_simplify"] = regions_simplify
    return kw


POLYGON_SUFFIXES = (".geojson", ".json")


def _read_zones(zones, zones_transform, shape, image_name):
    """``zones=PATH`` -> what ``process_image_zones`` takes: the polygons of a ``.geojson`` / ``.json`` file (rasterised on the device,
    ``zones_transform``: the six numbers of the geotransform their coordinates are in), or the label raster of any other file."""
    from .tiffio import read_image
    if Path(zones).suffix.lower() in POLYGON_SUFFIXES:
        from .zones import Polygons, polygons_from_geojson
        return Polygons(polygons_from_geojson(zones), transform=zones_transform, who=Path(zones).name)
    if zones_transform is not None:
        raise ValueError(f"{Path(zones).name}: zones_transform goes with a .geojson / .json file of polygons, not with a label raster")
    labels = read_image(zones)
    if labels.shape != shape:
        raise ValueError(f"{Path(zones).name}: the label raster has shape {labels.shape}, {image_name} is {shape}")
    return labels


def _transform_numbers(text):
    """``--zones-transform a,b,c,d,e,f`` -> six floats."""
    import argparse
    try:
        numbers = tuple(float(v) for v in text.split(","))
    except ValueError:
        numbers = ()
    if len(numbers) != 6:
        raise argparse.ArgumentTypeError(f"six comma-separated numbers x0,dx,rx,y0,ry,dy are needed, got {text!r}")
    return numbers


def _regions_spec(text):
    """``--regions INDEX:above:T[:min_pixels]`` (or ``below``) -> (index, "above" / "below", T, min_pixels)."""
    import argparse
    parts = text.split(":")
    try:
        if len(parts) not in (3, 4) or parts[0] not in INDEX_NAMES or parts[1] not in ("above", "below"):
            raise ValueError
        spec = (parts[0], parts[1], float(parts[2]), int(parts[3]) if len(parts) == 4 else 1)
        if spec[3] < 1 or spec[2] != spec[2]:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError(f"INDEX:above:T[:min_pixels] or INDEX:below:T[:min_pixels] with INDEX one of {', '.join(INDEX_NAMES)} "
                                         f"is needed, got {text!r}") from None
    return spec


ZONE_CSV_COLUMNS = ("Zone", "Index", "Pixels", "Mean", "Median", "Min", "Max", "Coverage (%)")
REGION_CSV_COLUMNS = ("Area", "Row0", "Col0", "Row1", "Col1", "Centroid Row", "Centroid Col")


def _write_zones_csv(path, result, indices):
    """``<stem>_zones.csv``: one row per zone and index from ``zones.zonal_rows``, floats written with ``repr`` (they read back exactly).
    Zones that are regions of the picture (``regions=``) add their area, box and centroid to every row."""
    import csv
    from .zones import zonal_rows
    table = result["zones"].get("regions")
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(ZONE_CSV_COLUMNS + (REGION_CSV_COLUMNS if table is not None else ()))
        for t in indices:
            for i, row in enumerate(zonal_rows(result, t)):
                figures = [v for k, v in row.items() if k not in ("Zone", "Pixels")]      # analyze_index's five, in its order
                region = [] if table is None else [int(table["area"][i])] + [int(v) for v in table["bbox"][i]] + [repr(float(v)) for v in table["centroid"][i]]
                out.writerow([row["Zone"], t, row["Pixels"]] + [repr(v) for v in figures] + region)


def _write_regions_geojson(path, result, indices, transform):
    """``<stem>_regions.geojson``: one ``Polygon`` feature per region (``zones.polygons_to_geojson``), in pixel coordinates or, with
    ``transform``, in the world coordinates of that geotransform.  A feature's properties are its rows of the CSV: the region's id, area,
    box and centroid, and per index the figures under ``zones.zonal_rows``'s keys (a NaN figure is written as null)."""
    import json
    from .zones import polygons_to_geojson, zonal_rows
    zones = result["zones"]
    table = zones["regions"]
    props = [{"Zone": int(z), "Pixels": int(n), "Area": int(a), **{c: int(v) for c, v in zip(REGION_CSV_COLUMNS[1:5], box)},
              "Centroid Row": float(mid[0]), "Centroid Col": float(mid[1])}
             for z, n, a, box, mid in zip(zones["zone"], zones["pixels"], table["area"], table["bbox"], table["centroid"])]
    for t in indices:
        for i, row in enumerate(zonal_rows(result, t)):
            props[i].update({k: (v if v == v else None) for k, v in row.items() if k not in ("Zone", "Pixels")})
    doc = {"type": "FeatureCollection", "features": []} if zones["outlines"] is None else polygons_to_geojson(zones["outlines"], transform, props)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f)


def _matching(png_encoder, tiff_encoder):
    """(the block that holds the knob ``deflate_matching`` at 1 where an encoder asks for it, the encoders without that suffix).
    The knob is one per process: ``batch_process`` enters the block once around its thread pool, not per file."""
    on = png_encoder.endswith(MATCHING) or tiff_encoder.endswith(MATCHING)
    block = codecs.deflate_matching() if on else contextlib.nullcontext()
    return block, png_encoder.removesuffix(MATCHING), tiff_encoder.removesuffix(MATCHING)


def process_image(image_path, output_dir, process_wb=False, indices=None, full_depth=False, lut_format="png",
                  png_encoder="pillow", png_decoder="pillow", jpeg_decoder="pillow", tiff_decoder="pillow", tiff_encoder="pillow",
                  index_tiff=False, nodata=None, alpha_mask=False, zones=None, zones_transform=None, regions=None, regions_geojson=False,
                  zone_margin=None, regions_simplify=None):
    """One file: same outputs as backend-process.py:49-73.  Returns the statistics dicts.
    ``full_depth=True`` reads three-sample 16-bit TIFFs at their full depth (``tiffio.read_image``; Pillow, hence the
    reference, keeps their high bytes only).  ``lut_format="tiff"`` writes the colormap images as
    uncompressed RGBA TIFFs ``<name>_<index>.tif`` instead of PNGs: PNG compression of a 4096 x 4096 map takes seconds,
    the GPU work milliseconds.  ``lut_format="png8"`` writes palette PNGs (one byte per pixel = the colormap entry, the
    colormap as the palette): ``Image.open(p).convert("RGBA")`` gives the pixels of the RGBA file, from a quarter of the
    bytes to compress.  ``png_encoder="device"`` encodes the PNG / png8 pictures on the GPU (``api.encode_png``: same pixels,
    only the files cross PCIe) instead of with Pillow.  ``png_decoder="device"`` decodes the input on the GPU when it is a
    PNG file ``api.png_info`` calls supported (``tiffio.read_image``; same pixels as Pillow), ``png_decoder="device+extended"`` also the
    1-, 2-, 4- and 16-bit and interlaced files (``api.decode_png(data, extended=True)``), ``jpeg_decoder="device"`` when
    it is a JPEG file ``api.jpeg_info`` calls supported, ``tiff_decoder="device"`` when it is a TIFF file ``api.tiff_info`` calls
    supported and the array is the one read today (``tiffio.read_image``); ``tiff_decoder="device+deflate"`` sends Deflate
    TIFF files there as well (``api.decode_tiff(..., deflate=True)``).  ``tiff_encoder="device"`` builds the TIFF files on
    the GPU (``api.encode_tiff``: LZW strips, the same samples): ``<name>_wb.tif`` instead of Pillow's uncompressed file, and the
    ``lut_format="tiff"`` pictures instead of ``tiffio.write_tiff``'s uncompressed ones.  ``index_tiff=True`` also writes the
    index plane itself, ``<INDEX>/<name>_<index>_f32.tif``: a single-band float32 LZW TIFF with Predictor 3, encoded on the
    GPU (``api.encode_tiff_f32``), the exact values the picture only colours; every other output is the same file.
    ``tiff_encoder="device+deflate"`` is ``"device"`` with Deflate strips (Compression 8, ``compression="deflate"``), and the
    ``index_tiff`` file follows it: Deflate with Predictor 3.  ``png_encoder="device+matching"`` and
    ``tiff_encoder="device+deflate+matching"`` are ``"device"`` and ``"device+deflate"`` with string matching in the Deflate
    coder (``codecs.deflate_matching``, a per-process setting held for the call): smaller files, the same pixels.
    ``nodata=N`` (pixels whose R, G and NIR all equal ``N`` are no picture) and ``alpha_mask=True`` (neither are pixels whose
    channel 3 is 0) go to ``nodata.process_image_masked`` as ``nodata`` / ``valid="alpha"``: white balance and statistics of the valid
    pixels only, transparent pictures and NaN planes outside.  Not with ``lut_format="png8"``: the palette has no free entry.
    ``zones=PATH`` names a single-band integer label raster of the picture's size (0 = in no zone; ``tiffio.read_image`` reads it)
    and adds ``<name>_zones.csv`` next to the outputs: one row per zone and requested index (``zones.process_image_zones``,
    ``zones.zonal_rows``), with the picture's white balance and under the same ``nodata`` / ``alpha_mask``.  Every other file is
    unchanged; the statistics come from a call of their own.  A ``zones`` path that ends in ``.geojson`` / ``.json`` holds the plots'
    outlines instead (``zones.polygons_from_geojson``; zone ``k`` is the ``k``-th geometry of the file): they are rasterised on the
    device (``zones.rasterize_zones``'s rule), in pixel coordinates or, with ``zones_transform=(x0, dx, rx, y0, ry, dy)``, in the
    world coordinates of that GDAL geotransform.  The CSV has the same columns either way.
    ``regions=(index, "above" | "below", t, min_pixels)`` takes the zones from the picture instead (``zones.Regions``): the connected
    patches of ``index`` above / below ``t`` with ``min_pixels`` pixels or more, labelled on the device; the same CSV with each region's
    area, box and centroid added.  ``index`` must be among the requested indices; not together with ``zones``.
    ``regions_geojson=True`` (with ``regions``) also writes ``<name>_regions.geojson``: the outline of every region, traced on the
    device (``zones.region_outlines``'s rings), one feature per region with its CSV figures as properties, in pixel coordinates or
    through ``zones_transform`` in world coordinates.
    ``zone_margin=PX`` (with ``zones`` or ``regions``, not with ``regions_geojson``) shrinks every zone inward by that many pixels on
    the device before its figures are taken (``zones.shrink_zones``'s rule); the CSV has the same columns, the regions' area, box and
    centroid stay those of the regions as found.
    ``regions_simplify=PX`` (with ``regions_geojson``) simplifies the outlines on the device before they are written
    (``zones.region_outlines``'s ``simplify``: Douglas-Peucker with a tolerance of PX pixels, 0 to 254); the CSV does not change."""
    if lut_format not in ("png", "png8", "tiff"):
        raise ValueError(f"lut_format must be 'png', 'png8' or 'tiff', got {lut_format!r}")
    _check_png_encoder(png_encoder)
    _check_png_decoder(png_decoder)
    _check_jpeg_decoder(jpeg_decoder)
    _check_tiff_decoder(tiff_decoder)
    _check_tiff_encoder(tiff_encoder)
    mask_kw = _mask_options(nodata, alpha_mask, lut_format)
    block, png_encoder, tiff_encoder = _matching(png_encoder, tiff_encoder)
    with block:
        return _process_image(image_path, output_dir, process_wb, indices, full_depth, lut_format, png_encoder, png_decoder, jpeg_decoder,
                              tiff_decoder, tiff_encoder, index_tiff, *_mask_argument(mask_kw),
                              **_zones_argument(zones, zones_transform, regions, regions_geojson, zone_margin, regions_simplify))


def _process_image(image_path, output_dir, process_wb, indices, full_depth, lut_format, png_encoder, png_decoder, jpeg_decoder, tiff_decoder,
                   tiff_encoder, index_tiff, mask_kw=None, zones=None, zones_transform=None, regions=None, regions_geojson=False, zone_margin=None,
                   regions_simplify=None):
    """``process_image`` behind its checks, for ``"pillow"``, ``"device"`` and ``"device+deflate"``."""
    from PIL import Image
    from .tiffio import read_image
    image_path, output_dir = Path(image_path), Path(output_dir)
    name = image_path.stem
    arr = read_image(image_path, full_depth, png_decoder, jpeg_decoder, tiff_decoder)
    if arr.ndim != 3 or arr.shape[2] < 3:
        raise ValueError(f"{image_path.name}: expected an image with at least 3 channels, got shape {arr.shape}")
    indices = list(indices or [])
    mask_kw = mask_kw or {}
    if regions is not None and zones is not None:
        raise ValueError("regions and zones both name the zones of the picture: give one of them")
    if regions is not None:
        from .zones import Regions
        index, how, t, min_pixels = regions
        if index not in indices:
            raise ValueError(f"regions are taken from {index}, which is not among the requested indices {indices}")
        zones = Regions(index=index, min_pixels=min_pixels, **{how: t}, **({"want_outlines": True} if regions_geojson else {}),
                        **({"simplify": regions_simplify} if regions_simplify is not None else {}))
    if zones is not None and indices:
        from .zones import process_image_zones
        labels = zones if regions is not None else _read_zones(zones, zones_transform, arr.shape[:2], image_path.name)
        output_dir.mkdir(parents=True, exist_ok=True)
        if zone_margin is not None:
            from .zones import Shrunk
            labels = Shrunk(labels, zone_margin)
        zoned = process_image_zones(arr, labels, **mask_kw, indices=indices, white_balance=True, want_arrays=False)
        _write_zones_csv(output_dir / f"{name}_zones.csv", zoned, indices)
        if regions_geojson:
            _write_regions_geojson(output_dir / f"{name}_regions.geojson", zoned, indices, zones_transform)

    def run(**kw):
        """``api.process_image`` of the file, or its masked form where a mask is set."""
        if not mask_kw:
            return api.process_image(arr, **kw)
        return nodata_rules.process_image_masked(arr, **mask_kw, **kw)

    palette = lut_format == "png8"
    device_png = png_encoder == "device" and lut_format != "tiff"
    planes = None                                   # the call whose entries hold the float32 TIFF files
    compression = "deflate" if tiff_encoder == "device+deflate" else "lzw"
    plane_tiff = "deflate+predictor" if compression == "deflate" else "predictor"
    if device_png:                                  # the pictures stay on the device, their PNG files come back
        res = run(indices=indices, white_balance=True, want_arrays=False, want_png="palette" if palette else True) if indices else None
        if index_tiff and indices:                  # one kind of file per call
            planes = run(indices=indices, white_balance=True, want_arrays=False, want_tiff=plane_tiff)
    elif index_tiff and indices:
        res = planes = run(indices=indices, white_balance=True, want_arrays=False, want_rgba=not palette, want_entries=palette,
                           want_tiff=plane_tiff)
    else:
        # palette files: the colormap entry of every pixel comes from the device, one byte per pixel (lars_h_process_image)
        res = run(indices=indices, white_balance=True, want_arrays=False, want_rgba=not palette, want_entries=palette) if indices else None
    if res:
        corrected = res["corrected"]
    elif mask_kw:
        corrected = run(indices=[], white_balance=True)["corrected"]
    else:
        corrected = api.fix_white_balance(arr)
    if process_wb:
        (output_dir / "white_balanced").mkdir(parents=True, exist_ok=True)
        wb = corrected[:, :, :3] if corrected.shape[2] > 4 else corrected
        if tiff_encoder != "pillow":
            (output_dir / "white_balanced" / f"{name}_wb.tif").write_bytes(api.encode_tiff(wb, compression=compression))
        else:
            Image.fromarray(wb).save(output_dir / "white_balanced" / f"{name}_wb.tif")
    stats = {}
    for t in indices:
        (output_dir / t).mkdir(parents=True, exist_ok=True)
        out = output_dir / t / f"{name}_{t.lower()}.png"
        entry = res["indices"][t]
        if device_png:
            out.write_bytes(entry["png"])
        elif lut_format == "tiff":
            if tiff_encoder != "pillow":
                out.with_suffix(".tif").write_bytes(api.encode_tiff(entry["rgba"], compression=compression))
            else:
                from .tiffio import write_tiff
                write_tiff(out.with_suffix(".tif"), entry["rgba"])
        elif palette:
            im = Image.fromarray(entry["entry"], "P")
            im.putpalette(api.colormap_lut(api._colormap_for(t)).tobytes(), rawmode="RGBA")
            im.save(out, compress_level=LUT_PNG_LEVEL)
        else:
            Image.fromarray(entry["rgba"], "RGBA").save(out, compress_level=LUT_PNG_LEVEL)
        if planes is not None:
            (output_dir / t / f"{name}_{t.lower()}_f32.tif").write_bytes(planes["indices"][t]["tiff"])
        stats[t] = entry["stats"]
    return stats


def files_of_rank(files, rank=0, world=1):
    """The files one rank of a multi-GPU run owns: a contiguous block of the sorted list (``batch.shard_range``, the split the
    tile batches use).  Files are independent (backend-process.py:92-95 loops over them one by one), so there is no exchange."""
    from .batch import shard_range
    rank, world = int(rank), int(world)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world}")
    files = list(files)
    start, stop = shard_range(len(files), rank, world)
    return files[start:stop]


def batch_process(input_dir, output_dir, process_wb=False, process_ndvi=False, process_gndvi=False,
                  process_ndwi=True, workers=4, verbose=True, full_depth=False, lut_format="png", rank=0, world=1,
                  device=None, png_encoder="pillow", png_decoder="pillow", jpeg_decoder="pillow", tiff_decoder="pillow",
                  tiff_encoder="pillow", index_tiff=False, nodata=None, alpha_mask=False, zones=None, zones_transform=None, regions=None,
                  regions_geojson=False, zone_margin=None, regions_simplify=None):
    """backend-process.py:75-97 with its module constants as arguments.  Returns ``{file name: stats | error}``.
    ``rank`` / ``world``: one process per GPU, each takes its block of the sorted file list (``files_of_rank``); the output
    directories are shared, the file names distinct.  ``device``: the GPU ordinal every worker thread binds (the library's
    context is per thread and defaults to device 0); None leaves the threads' binding alone.  ``png_encoder``,
    ``png_decoder``, ``jpeg_decoder``, ``tiff_decoder``, ``tiff_encoder``, ``index_tiff``, ``nodata``, ``alpha_mask``, ``zones`` (one label
    raster, or one file of polygons with its ``zones_transform``, for every file of the directory), ``regions``, ``regions_geojson``,
    ``zone_margin``, ``regions_simplify``: see ``process_image``."""
    mask_kw = _mask_options(nodata, alpha_mask, lut_format)
    zones_kw = _zones_argument(zones, zones_transform, regions, regions_geojson, zone_margin, regions_simplify)
    _check_tiff_encoder(tiff_encoder)
    _check_png_encoder(png_encoder)
    _check_png_decoder(png_decoder)
    _check_jpeg_decoder(jpeg_decoder)
    _check_tiff_decoder(tiff_decoder)
    block, png_encoder, tiff_encoder = _matching(png_encoder, tiff_encoder)
    input_path, output_path = Path(input_dir), Path(output_dir)
    indices = [t for t, on in (("NDVI", process_ndvi), ("GNDVI", process_gndvi), ("NDWI", process_ndwi)) if on]
    files = files_of_rank(sorted(f for f in input_path.glob("*") if f.suffix.lower() in EXTENSIONS), rank, world)
    total = len(files)
    results = {}

    def one(job):
        idx, f = job
        try:
            if verbose:
                print(f"Processing {idx}/{total}: {f.name}")
            return f.name, _process_image(f, output_path, process_wb, indices or None, full_depth, lut_format, png_encoder,
                                          png_decoder, jpeg_decoder, tiff_decoder, tiff_encoder, index_tiff, *_mask_argument(mask_kw), **zones_kw)
        except Exception as e:                              # same policy as upstream :96-97
            if verbose:
                print(f"Error processing {f.name}: {str(e)}")
            return f.name, e

    def bind():
        if device is not None:
            from . import _ffi
            _ffi.call("lars_set_device", int(device))

    with block:
        if workers <= 1:
            bind()
            for job in enumerate(files, 1):
                k, v = one(job)
                results[k] = v
        else:
            with ThreadPoolExecutor(max_workers=min(workers, os.cpu_count() or 1), initializer=bind) as pool:
                for k, v in pool.map(one, enumerate(files, 1)):
                    results[k] = v
    return results


def export_zip(image_array, selected_indices, corrected_array=None, png_encoder="pillow"):
    """ZIP of the processed images of one upload (``download_processed_images``,
    process-images.py:567-617): ``white_balanced.png`` + ``<INDEX>_visualization.png`` per index, the latter as
    full-resolution per-pixel colormap images (one GPU pass for white balance, every index and every colormap).
    ``corrected_array`` (the cached white-balanced image the UI keeps, process-images.py:1132) skips the
    white-balance step.  ``png_encoder="device"`` encodes every PNG of the archive on the GPU (``api.encode_png``; same
    pixels): the colormap pictures never leave the device; ``"device+matching"`` does so with string matching in the
    Deflate coder (``process_image``).
    """
    _check_png_encoder(png_encoder)
    block, png_encoder, _ = _matching(png_encoder, "pillow")
    with block:
        return _export_zip(image_array, selected_indices, corrected_array, png_encoder)


def _export_zip(image_array, selected_indices, corrected_array, png_encoder):
    import io
    import zipfile
    from PIL import Image
    indices = list(selected_indices)
    device = png_encoder == "device"
    want = {"want_png": True} if device else {"want_rgba": True}
    if corrected_array is not None:
        res = api.process_image(np.asarray(corrected_array), indices=indices, white_balance=False, want_arrays=False, **want)
        corrected = np.asarray(corrected_array)
    else:
        res = api.process_image(np.asarray(image_array), indices=indices, white_balance=True, want_arrays=False, **want)
        corrected = res["corrected"]
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as zf:
        if device:
            zf.writestr("white_balanced.png", api.encode_png(corrected))
        else:
            png = io.BytesIO()
            Image.fromarray(corrected).save(png, format="PNG")
            zf.writestr("white_balanced.png", png.getvalue())
        for t in indices:
            if device:
                zf.writestr(f"{t}_visualization.png", res["indices"][t]["png"])
                continue
            png = io.BytesIO()
            Image.fromarray(res["indices"][t]["rgba"], "RGBA").save(png, format="PNG", compress_level=LUT_PNG_LEVEL)
            zf.writestr(f"{t}_visualization.png", png.getvalue())
    return buf.getvalue()


def main(argv=None):
    """``python -m lars_image_processing_amd.driver IN OUT [--wb] [--ndvi] [--gndvi] [--no-ndwi] ...``: backend-process.py's
    ``__main__`` with its constants as flags.  Under a launcher (``python -m torch.distributed.run --nproc-per-node N -m
    lars_image_processing_amd.driver ...``) every rank binds GPU ``LOCAL_RANK`` and processes its block of the files."""
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="lars_image_processing_amd.driver")
    ap.add_argument("input_dir")
    ap.add_argument("output_dir")
    ap.add_argument("--wb", action="store_true", help="also write white_balanced/<name>_wb.tif (PROCESS_WB)")
    ap.add_argument("--ndvi", action="store_true")
    ap.add_argument("--gndvi", action="store_true")
    ap.add_argument("--no-ndwi", dest="ndwi", action="store_false", help="backend-process.py:12-15 has only NDWI on")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--full-depth", action="store_true")
    ap.add_argument("--lut-format", default="png", choices=["png", "png8", "tiff"])
    ap.add_argument("--png-encoder", default="pillow", choices=list(PNG_ENCODERS + PNG_ENCODERS_MATCHING),
                    help="'device' encodes the index PNGs on the GPU (same pixels, only the files cross PCIe), "
                         "'device+matching' with string matching in the Deflate coder (smaller files)")
    ap.add_argument("--png-decoder", default="pillow", choices=list(PNG_DECODERS),
                    help="'device' decodes 8-bit non-interlaced PNG inputs on the GPU (same pixels; other files stay with Pillow), "
                         "'device+extended' also 1-, 2-, 4- and 16-bit and interlaced ones")
    ap.add_argument("--jpeg-decoder", default="pillow", choices=list(JPEG_DECODERS),
                    help="'device' decodes supported JPEG inputs on the GPU (same pixels; other files stay with Pillow)")
    ap.add_argument("--tiff-decoder", default="pillow", choices=list(TIFF_DECODERS),
                    help="'device' decodes supported TIFF inputs on the GPU (same samples; other files take today's path); "
                         "'device+deflate' decodes Deflate TIFF files there too")
    ap.add_argument("--tiff-encoder", default="pillow", choices=list(TIFF_ENCODERS + TIFF_ENCODERS_MATCHING),
                    help="'device' builds <name>_wb.tif and the --lut-format tiff pictures on the GPU (LZW strips, same samples); "
                         "'device+deflate' the same with Deflate strips, also for --index-tiff; 'device+deflate+matching' those with string matching")
    ap.add_argument("--index-tiff", action="store_true",
                    help="also write <INDEX>/<name>_<index>_f32.tif: the float32 index plane as an LZW TIFF with Predictor 3, built on the GPU")
    ap.add_argument("--nodata", type=int, default=None, metavar="N",
                    help="pixels whose R, G and NIR samples all equal N are no picture: left out of the white balance and the statistics, "
                         "transparent in the index pictures, NaN in the --index-tiff planes (not with --lut-format png8)")
    ap.add_argument("--alpha-mask", action="store_true",
                    help="pixels whose channel 3 (alpha) is 0 are no picture; combines with --nodata")
    ap.add_argument("--zones", default=None, metavar="PATH",
                    help="a single-band integer label raster of the pictures' size (0 = in no zone): also write <name>_zones.csv, one row "
                         "per zone and index, with the picture's white balance; combines with --nodata / --alpha-mask.  A .geojson / "
                         ".json file holds the plots' outlines instead: they are rasterised on the GPU, zone k is the k-th geometry")
    ap.add_argument("--zones-transform", default=None, type=_transform_numbers, metavar="x0,dx,rx,y0,ry,dy",
                    help="the GDAL geotransform (pixel -> world) the polygons of --zones are in; without it they are in pixel units")
    ap.add_argument("--regions", default=None, type=_regions_spec, metavar="INDEX:above:T[:min_pixels]",
                    help="take the zones from the picture: the connected patches of INDEX above (or 'below') T with min_pixels pixels or more, "
                         "labelled on the GPU; writes <name>_zones.csv with each region's area, box and centroid added.  Not with --zones")
    ap.add_argument("--regions-geojson", action="store_true",
                    help="with --regions: also write <name>_regions.geojson, the outline of every region traced on the GPU, one feature per "
                         "region with its CSV figures as properties; --zones-transform puts it in world coordinates")
    ap.add_argument("--regions-simplify", default=None, type=float, metavar="PX",
                    help="with --regions-geojson: simplify the outlines on the GPU before they are written, Douglas-Peucker with a tolerance "
                         "of PX pixels (0 to 254, in sixteenths); every traced vertex stays within PX of its ring")
    ap.add_argument("--zone-margin", default=None, type=float, metavar="PX",
                    help="with --zones or --regions: shrink every zone inward by PX pixels (0 to 254) on the GPU before its figures are "
                         "taken, so that the mixed pixels along a plot's edge stay out; the CSV columns are unchanged.  Not with "
                         "--regions-geojson")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    if args.regions_geojson and args.regions is None:
        ap.error("--regions-geojson writes the outlines of the regions: it goes with --regions")
    if args.regions_simplify is not None and not args.regions_geojson:
        ap.error("--regions-simplify is the tolerance of the outlines in the GeoJSON: it goes with --regions-geojson")
    if args.regions_simplify is not None and not 0 <= args.regions_simplify <= 254:
        ap.error(f"--regions-simplify must be 0 to 254 pixels, got {args.regions_simplify}")
    if args.zone_margin is not None and args.zones is None and args.regions is None:
        ap.error("--zone-margin shrinks the zones of the picture: it goes with --zones or --regions")
    if args.zone_margin is not None and args.regions_geojson:
        ap.error("--zone-margin and --regions-geojson do not go together: outlines are traced from regions as found")
    if args.zone_margin is not None and not 0 <= args.zone_margin <= 254:
        ap.error(f"--zone-margin must be 0 to 254 pixels, got {args.zone_margin}")
    from .dist import env_rank_world
    rank, local_rank, world = env_rank_world()
    res = batch_process(args.input_dir, args.output_dir, args.wb, args.ndvi, args.gndvi, args.ndwi, args.workers,
                        not args.quiet, args.full_depth, args.lut_format, rank, world,
                        device=local_rank if world > 1 else None, png_encoder=args.png_encoder,
                        png_decoder=args.png_decoder, jpeg_decoder=args.jpeg_decoder, tiff_decoder=args.tiff_decoder,
                        tiff_encoder=args.tiff_encoder, index_tiff=args.index_tiff, nodata=args.nodata, alpha_mask=args.alpha_mask,
                        **_zones_argument(args.zones, args.zones_transform, args.regions, args.regions_geojson, args.zone_margin,
                                          args.regions_simplify))
    failed = {k: str(v) for k, v in res.items() if isinstance(v, Exception)}
    print(json.dumps({"rank": rank, "world": world, "files": len(res), "failed": failed}))
    return 1 if failed else 0


if __name__ == "__main__":
    raise SystemExit(main())
