"""MI355X-native multispectral index path (white balance -> NDVI/GNDVI/NDWI -> statistics).

Drop-in for the per-pixel path of lars-uav/lars-image-processing: the functions
below keep the reference's signatures and run on hand-written HIP kernels
(gfx950) behind a C ABI (include/lars_hip.h).  No PyTorch, no NumPy fallback.
"""
from .api import (  # noqa: F401
    align_images,
    analyze_index,
    analyze_index_statistics,
    analyze_ndvi_statistics,
    calculate_index,
    calculate_index_statistics_by_timeframe,
    calculate_ndvi,
    calculate_ndvi_array,
    change_detection,
    classification_mask,
    colorize_difference,
    colorize_index,
    colormap_lut,
    correct_white_balance,
    decode_jpeg,
    encode_jpeg,
    decode_png,
    decode_tiff,
    encode_png,
    encode_tiff,
    encode_tiff_f32,
    download_processed_images,
    fix_white_balance,
    fix_white_balance_rgnir,
    generate_ndvi_report,
    index_histogram,
    jpeg_draft_scale,
    jpeg_info,
    preprocess_large_image,
    png_info,
    process_image,
    thumbnail,
    thumbnail_jpeg,
    thumbnail_plan,
    thumbnail_png,
    thumbnail_tiff,
    tiff_bound,
    tiff_f32_bound,
    tiff_info,
    time_series_points,
    timeseries_row,
)
from .codecs import deflate_matching  # noqa: F401
from .nodata import process_image_masked, valid_mask  # noqa: F401
from .zones import (Polygons, Regions, Shrunk, label_regions, polygons_from_geojson, polygons_to_geojson, process_image_zones,  # noqa: F401
                    rasterize_zones, region_outlines, shrink_zones, simplify_outlines, to_pixel, to_world, zonal_rows, zonal_statistics)
from .batch import TileBatch, local_fold, merge_records, shard_range, summarize, timeseries_rows  # noqa: F401
from .tiffio import read_image, read_tiff, write_float_tiff, write_tiff  # noqa: F401

__version__ = "0.1.0"
