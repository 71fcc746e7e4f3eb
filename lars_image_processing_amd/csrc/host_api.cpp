// Host entry points (lars_h_*): host pointers in, host pointers out.  These are
// what the Python mirror of the reference's functions binds (one call per
// reference function).  Each call stages through the calling
// thread's grow-only device workspace and stream, so concurrent Streamlit
// sessions (threads) do not share mutable state.
#include <string.h>
#include <vector>

#include "common.h"

using namespace lars;

namespace {

// ---- zonal statistics (zonal.hip): the device buffers of the four stages and their run, for both host entry points ----
struct ZoneBufs {
    char *labels;                  // [npix] labels, zone_bytes wide
    uint64_t *counts;              // [nzones + 1], then the count of bad labels
    uint64_t *ends, *cursors;      // [nzones + 1] each
    float *out[3];                 // the values of each index, zone by zone
    lars_stats *stats;             // [3][nzones]
    float *med;                    // [3][nzones][2]
    char *sel;                     // select scratch of the large zones
};

ZoneBufs zone_plan(Carver &c, size_t npix, int zone_bytes, int64_t nzones, uint32_t mask)
{
    ZoneBufs B;
    const size_t nz = (size_t)nzones;
    B.labels = c.take<char>(npix * (size_t)zone_bytes);
    B.counts = c.take<uint64_t>(nz + 2);
    B.ends = c.take<uint64_t>(nz + 1);
    B.cursors = c.take<uint64_t>(nz + 1);
    for (int k = 0; k < 3; ++k) B.out[k] = ((mask >> k) & 1u) ? c.take<float>(npix) : nullptr;
    B.stats = c.take<lars_stats>(3 * nz);
    B.med = c.take<float>(6 * nz);
    B.sel = c.take<char>(lars_select_scratch_bytes());
    return B;
}

// labels up, the four stages, the records down (host_stats[3][nzones], host_med[3][nzones][2]; rows outside mask untouched).
// The counts cross to the host once: bad labels end the call there, and zones above the knob zone_split_pixels take the array
// kernels, which spread one zone over many workgroups.  The copies down are on the stream when this returns: the caller waits.
int run_zones(const char *who, const ZoneBufs &B, const void *zones, int zone_bytes, const uint8_t *valid_dev, int64_t npix, int64_t nzones,
              const float *const planes[3], uint32_t mask, const float thr[3], int want_hist, lars_stats *host_stats, float *host_med,
              int64_t *bad_labels, hipStream_t s)
{
    const size_t nz = (size_t)nzones;
    LARS_HIP_TRY(hipMemcpyAsync(B.labels, zones, (size_t)npix * zone_bytes, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_zone_count(B.labels, zone_bytes, valid_dev, npix, nzones, B.counts, B.counts + nz + 1, s));
    std::vector<uint64_t> counts(nz + 2);
    LARS_HIP_TRY(hipMemcpyAsync(counts.data(), B.counts, (nz + 2) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (bad_labels) *bad_labels = (int64_t)counts[nz + 1];
    if (counts[nz + 1])
        return fail(LARS_ERR_INVALID, "%s: %llu labels outside 0 .. %lld", who, (unsigned long long)counts[nz + 1], (long long)nzones);
    LARS_TRY(lars_d_zone_offsets(B.counts, nzones, B.ends, B.cursors, s));
    LARS_TRY(lars_d_zone_scatter(planes, mask, B.labels, zone_bytes, valid_dev, npix, nzones, B.ends, B.cursors, B.out, s));
    const int64_t split = tuning().zone_split_pixels;
    for (int k = 0; k < 3; ++k) {
        if (!((mask >> k) & 1u)) continue;
        lars_stats *st = B.stats + k * nz;
        float *med = B.med + 2 * k * nz;
        LARS_TRY(lars_d_zone_stats(B.out[k], B.ends, B.counts, nzones, thr[k], want_hist, split, st, med, s));
        uint64_t lo = 0;
        for (size_t z = 1; z <= nz; lo += counts[z], ++z) {
            if (counts[z] <= (uint64_t)split) continue;
            LARS_TRY(lars_d_array_stats_f32(B.out[k] + lo, (int64_t)counts[z], thr[k], want_hist, st + (z - 1), s));
            LARS_TRY(lars_d_median_pair_f32(B.out[k] + lo, (int64_t)counts[z], med + 2 * (z - 1), B.sel, s));
        }
        LARS_HIP_TRY(hipMemcpyAsync(host_stats + k * nz, st, nz * sizeof(lars_stats), hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipMemcpyAsync(host_med + 2 * k * nz, med, 2 * nz * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    return LARS_OK;
}

int zone_arguments(const char *who, const void *zones, int zone_bytes, int64_t nzones, const void *stats, const void *medians)
{
    if (!zones || !stats || !medians) return fail(LARS_ERR_INVALID, "%s: zones, their records and their medians are required", who);
    if (zone_bytes != 1 && zone_bytes != 2 && zone_bytes != 4) return fail(LARS_ERR_INVALID, "%s: labels are 1, 2 or 4 bytes wide, got %d", who, zone_bytes);
    if (nzones < 1 || nzones > LARS_ZONES_MAX) return fail(LARS_ERR_INVALID, "%s: 1 to %d zones, got %lld", who, LARS_ZONES_MAX, (long long)nzones);
    return LARS_OK;
}

struct ImageJob {
    const void *img;
    int64_t h, w;
    int channels, dtype;
    int apply_wb, wb_variant;
    uint32_t mask;
    int want_stats, want_hist, want_median;
    uint8_t *out_wb;
    float *out_index[3];
    lars_stats *stats;
    float *medians;               // [3][2]
    uint8_t *out_rgba[3];
    const uint8_t *cmap[3];
    double *pcts;                 // [3][2]
    int png_mode;                 // 0 none, 1 RGBA colormap pictures, 2 palette pictures of the colormap entries (PNG on the device)
    uint8_t *out_png[3];
    size_t png_cap;
    int64_t *png_len;             // [3]
    int tiff;                     // 0 none, 1 float32 TIFF files of the index planes (encoded on the device)
    int tiff_compression;         // 5 LZW, 8 Deflate
    int tiff_predictor;
    int64_t tiff_rps;
    uint8_t *out_tiff[3];
    size_t tiff_cap;
    int64_t *tiff_len;            // [3]
    // nodata-aware job (masked.hip): pixels outside the mask take no part in the percentiles and the statistics
    int masked;
    const uint8_t *valid;         // [h][w], nonzero = picture, or null
    int use_alpha, has_nodata, nodata;
    int64_t *valid_pixels;
    // ... with one record per zone and index as well (zonal.hip): the planes stay on the device for the zone stages
    const void *zones;            // [h][w] labels 0 .. nzones, zone_bytes wide, or null
    int zone_bytes;
    int64_t nzones;
    lars_stats *zone_stats;       // [3][nzones]
    float *zone_medians;          // [3][nzones][2]
    int64_t *bad_labels;
};

struct TiffAnswer { int64_t len; int32_t status[2]; };

struct Layout {
    uint8_t *img; uint32_t *hist; uint8_t *table; double *pcts; uint8_t *wb;
    float *idx[3]; lars_stats *stats; float *med; char *sel; uint8_t *rgba[3]; uint8_t *cmap[3];
    uint8_t *entry[3];             // colormap entry planes (out_rgba[k] without a cmap_lut[k]): one byte per pixel
    float *pairs; char *selq;      // statistics + medians without planes (lars_d_stats_medians)
    uint8_t *png[3], *pal[3];      // PNG files of the index pictures, palettes of the P pictures
    int64_t *png_len; char *png_scratch;
    size_t png_bound;
    uint8_t *tif[3];               // float32 TIFF files of the index planes
    TiffAnswer *tif_ans; char *tif_scratch;
    size_t tif_bound;
    uint8_t *vmask;                // masked jobs: one byte per pixel, 1 = picture
    uint64_t *vcount;              // {|V|, cursor of the compaction}
    uint32_t *vhist;               // channel histograms of the valid pixels
    float *vals[3];                // the valid values of each index, compacted
    ZoneBufs zone;                 // jobs with zones
};

// Medians of uint8 RGNir images come from the two-level select on recomputed values (select_q.hip): two passes over the
// 3-byte pixels instead of four or more over each 4-byte plane, whether or not the planes are written as well.
bool select_route(const ImageJob &j)
{
    if (j.masked || !j.want_median || !j.medians || !j.mask || j.dtype != LARS_U8 || j.channels != 3) return false;
    return (long long)j.h * j.w * 6 < (1ll << 30);
}
// ... and when no plane is wanted (one index or all three), the statistics kernel counts the select's first pass itself:
// the planes never exist on the device either
bool recompute_route(const ImageJob &j)
{
    if (!select_route(j) || !j.want_stats || j.png_mode || j.tiff) return false;
    if (j.mask != 1u && j.mask != 2u && j.mask != 4u && j.mask != 7u) return false;
    for (int k = 0; k < 3; ++k)
        if (j.out_index[k] || j.out_rgba[k]) return false;
    return true;
}

Layout plan(const ImageJob &j, Carver &c)
{
    Layout L;
    const size_t npix = (size_t)j.h * j.w;
    const size_t esz = j.dtype == LARS_U8 ? 1 : 2;
    const size_t nval = j.dtype == LARS_U8 ? 256 : 65536;
    L.img = c.take<uint8_t>(npix * j.channels * esz);
    L.hist = nullptr;
    L.table = j.apply_wb ? c.take<uint8_t>(lars_wb_table_bytes(j.dtype)) : nullptr;
    L.pcts = j.apply_wb ? c.take<double>(6) : nullptr;
    L.wb = (j.apply_wb && j.out_wb) ? c.take<uint8_t>(npix * j.channels) : nullptr;
    const bool select = select_route(j);
    const int png_channels = j.png_mode == 1 ? 4 : 1;
    L.png_bound = j.png_mode ? lars_png_bound(j.h, j.w, png_channels) : 0;
    for (int k = 0; k < 3; ++k) {
        const bool on = (j.mask >> k) & 1u;
        // the entry plane is derived from the float32 plane on the device
        const bool entries = on && ((j.out_rgba[k] && !j.cmap[k]) || j.png_mode == 2);
        const bool rgba = on && j.cmap[k] && (j.out_rgba[k] || j.png_mode == 1);
        L.idx[k] = (on && (j.out_index[k] || entries || j.tiff || j.zones || (j.want_median && !select && !j.masked))) ? c.take<float>(npix) : nullptr;
        L.rgba[k] = rgba ? c.take<uint8_t>(npix * 4) : nullptr;
        L.cmap[k] = rgba ? c.take<uint8_t>(1024) : nullptr;
        L.entry[k] = entries ? c.take<uint8_t>(npix + 4) : nullptr;
        L.pal[k] = (on && j.png_mode == 2) ? c.take<uint8_t>(1024) : nullptr;
        L.png[k] = (on && j.png_mode) ? c.take<uint8_t>(L.png_bound) : nullptr;
    }
    const bool tif_deflate = j.tiff_compression == 8;
    L.tif_bound = !j.tiff ? 0 : tif_deflate ? lars_tiff_float32_deflate_bound(j.h, j.w, 1, j.tiff_rps) : lars_tiff_f32_bound(j.h, j.w, 1, j.tiff_rps);
    for (int k = 0; k < 3; ++k) L.tif[k] = (j.tiff && ((j.mask >> k) & 1u)) ? c.take<uint8_t>(L.tif_bound) : nullptr;
    L.tif_ans = j.tiff ? c.take<TiffAnswer>(3) : nullptr;
    L.tif_scratch = !j.tiff ? nullptr : c.take<char>(tif_deflate ? lars_tiff_float32_deflate_encode_scratch_bytes(j.h, j.w, 1, j.tiff_rps)
                                                                 : lars_tiff_f32_encode_scratch_bytes(j.h, j.w, 1, j.tiff_rps));
    L.png_len = j.png_mode ? c.take<int64_t>(3) : nullptr;
    L.png_scratch = j.png_mode ? c.take<char>(lars_png_scratch_bytes(j.h, j.w, png_channels)) : nullptr;
    L.stats = c.take<lars_stats>(3);
    L.med = c.take<float>(6);
    L.sel = c.take<char>(3 * ((lars_select_scratch_bytes() + 255) & ~(size_t)255));
    L.pairs = select ? c.take<float>(4) : nullptr;
    L.selq = select ? c.take<char>(lars_quotient_median_scratch_bytes(1)) : nullptr;
    L.vmask = j.masked ? c.take<uint8_t>(npix + 4) : nullptr;
    L.vcount = j.masked ? c.take<uint64_t>(2) : nullptr;
    L.vhist = (j.masked && j.apply_wb) ? c.take<uint32_t>(3 * nval) : nullptr;
    for (int k = 0; k < 3; ++k)
        L.vals[k] = (j.masked && ((j.mask >> k) & 1u) && (j.want_stats || j.want_median)) ? c.take<float>(npix) : nullptr;
    if (j.zones) L.zone = zone_plan(c, npix, j.zone_bytes, j.nzones, j.mask);
    return L;
}

// A masked job's white-balance pre-pass and fused step (everything after them is run_image's): the mask and |V|, the
// histograms of the valid pixels and their tables, the planes, and the record and the median of each index from its
// compacted values.  |V| crosses to the host once: the table, statistics and select launches are sized by it.
int run_masked(const ImageJob &j, const Layout &L, hipStream_t s)
{
    const int64_t npix = j.h * j.w;
    if (j.valid) LARS_HIP_TRY(hipMemcpyAsync(L.vmask, j.valid, (size_t)npix, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_valid_mask(L.img, npix, j.channels, j.dtype, j.valid ? L.vmask : nullptr, j.use_alpha, j.has_nodata, j.nodata, L.vmask,
                               L.vcount, s));
    uint64_t nvalid = 0;
    LARS_HIP_TRY(hipMemcpyAsync(&nvalid, L.vcount, sizeof nvalid, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (j.valid_pixels) *j.valid_pixels = (int64_t)nvalid;
    if (!nvalid) return fail(LARS_ERR_INVALID, "lars_h_process_image_masked: no valid pixel");
    if (j.apply_wb) {
        LARS_TRY(lars_d_masked_channel_hist(L.img, npix, j.channels, j.dtype, L.vmask, L.vhist, s));
        LARS_TRY(lars_d_wb_table(L.vhist, 1, (int64_t)nvalid, j.dtype, L.table, L.pcts, j.wb_variant, s));
    }
    if (!j.mask && !L.wb) return LARS_OK;
    lars_fused_args a;
    memset(&a, 0, sizeof a);
    a.tiles = L.img; a.ntiles = 1; a.npix = npix; a.channels = j.channels; a.dtype = j.dtype;
    a.wb_table = j.apply_wb ? L.table : nullptr;
    a.index_mask = j.mask;
    for (int k = 0; k < 3; ++k) {
        a.out_index[k] = L.idx[k];
        a.out_rgba[k] = L.rgba[k];
        a.cmap_lut[k] = L.cmap[k];
        if (L.cmap[k]) LARS_HIP_TRY(hipMemcpyAsync(L.cmap[k], j.cmap[k], 1024, hipMemcpyHostToDevice, s));
    }
    a.out_wb = L.wb;
    a.stream = s;
    LARS_TRY(lars_d_masked_fused(&a, L.vmask, L.vals, L.vcount + 1));
    const size_t selsz = (lars_select_scratch_bytes() + 255) & ~(size_t)255;
    for (int k = 0; k < 3; ++k) {
        if (!L.vals[k]) continue;
        // process-images.py:498-504: coverage above 0.2, water (NDWI) above 0
        if (j.want_stats) LARS_TRY(lars_d_array_stats_f32(L.vals[k], (int64_t)nvalid, k == LARS_NDWI ? 0.0f : 0.2f, j.want_hist, L.stats + k, s));
        if (j.want_median && j.medians) LARS_TRY(lars_d_median_pair_f32(L.vals[k], (int64_t)nvalid, L.med + 2 * k, L.sel + k * selsz, s));
    }
    return LARS_OK;
}

int run_image(const ImageJob &j)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!j.img || j.h <= 0 || j.w <= 0 || j.channels < 3)
        return fail(LARS_ERR_INVALID, "image must be a non-empty [h][w][>=3] array");
    if (j.dtype != LARS_U8 && j.dtype != LARS_U16) return fail(LARS_ERR_INVALID, "dtype must be LARS_U8 or LARS_U16");
    if (j.mask & ~LARS_MASK_ALL) return fail(LARS_ERR_INVALID, "unknown index bits in mask");
    const size_t npix = (size_t)j.h * j.w;
    const size_t esz = j.dtype == LARS_U8 ? 1 : 2;
    Layout L;
    LARS_TRY(ws_plan(c, [&](Carver &cv) { L = plan(j, cv); }));
    hipStream_t s = c->stream;

    LARS_HIP_TRY(hipMemcpyAsync(L.img, j.img, npix * j.channels * esz, hipMemcpyHostToDevice, s));
    const bool stats = j.want_stats && j.mask;
    if (j.masked) {
        LARS_TRY(run_masked(j, L, s));
        if (j.zones) {
            // process-images.py:498-504, as run_masked's records
            const float thr[3] = {0.2f, 0.2f, 0.0f};
            LARS_TRY(run_zones("lars_h_process_image_zones", L.zone, j.zones, j.zone_bytes, L.vmask, (int64_t)npix, j.nzones, L.idx, j.mask, thr,
                               j.want_hist, j.zone_stats, j.zone_medians, j.bad_labels, s));
        }
    } else if (j.apply_wb) {
        LARS_TRY(lars_d_wb_prepare(L.img, 1, (int64_t)npix, j.channels, j.dtype, L.table, L.pcts, j.wb_variant, s));
    }
    if (!j.masked && (j.mask || L.wb)) {
        lars_fused_args a;
        memset(&a, 0, sizeof a);
        a.tiles = L.img; a.ntiles = 1; a.npix = (int64_t)npix; a.channels = j.channels; a.dtype = j.dtype;
        a.wb_table = j.apply_wb ? L.table : nullptr;
        a.index_mask = j.mask;
        a.flags = stats ? (LARS_F_STATS | (j.want_hist ? LARS_F_HIST : 0u)) : 0u;
        for (int k = 0; k < 3; ++k) {
            a.out_index[k] = L.idx[k];
            a.out_rgba[k] = L.rgba[k];
            a.cmap_lut[k] = L.cmap[k];
            if (L.cmap[k]) LARS_HIP_TRY(hipMemcpyAsync(L.cmap[k], j.cmap[k], 1024, hipMemcpyHostToDevice, s));
        }
        a.out_wb = L.wb;
        a.stats = stats ? L.stats : nullptr;
        a.stream = s;
        if (recompute_route(j)) {
            if (L.wb) {                                     // the white-balanced image on its own, then statistics + medians
                lars_fused_args w = a;
                w.index_mask = 0; w.flags = 0; w.stats = nullptr;
                LARS_TRY(lars_d_fused(&w));
                a.out_wb = nullptr;
            }
            LARS_TRY(lars_d_stats_medians(&a, L.pairs, L.selq));
        } else {
            LARS_TRY(lars_d_fused(&a));
            if (L.pairs)
                LARS_TRY(lars_d_quotient_median_pairs(L.img, 1, (int64_t)npix, 3, LARS_U8, a.wb_table,
                                                      ((j.mask & 1u) ? 1u : 0u) | ((j.mask & 6u) ? 2u : 0u), L.pairs, L.selq, s));
        }
    }
    const size_t selsz = (lars_select_scratch_bytes() + 255) & ~(size_t)255;
    for (int k = 0; k < 3; ++k) {
        if (!((j.mask >> k) & 1u) || L.pairs || j.masked) continue;
        if (j.want_median && j.medians)
            LARS_TRY(lars_d_median_pair_f32(L.idx[k], (int64_t)npix, L.med + 2 * k, L.sel + k * selsz, s));
    }
    // results back
    if (L.wb) LARS_HIP_TRY(hipMemcpyAsync(j.out_wb, L.wb, npix * j.channels, hipMemcpyDeviceToHost, s));
    for (int k = 0; k < 3; ++k) {
        if (!((j.mask >> k) & 1u)) continue;
        if (j.out_index[k]) LARS_HIP_TRY(hipMemcpyAsync(j.out_index[k], L.idx[k], npix * 4, hipMemcpyDeviceToHost, s));
        if (L.rgba[k] && j.out_rgba[k]) LARS_HIP_TRY(hipMemcpyAsync(j.out_rgba[k], L.rgba[k], npix * 4, hipMemcpyDeviceToHost, s));
        if (L.entry[k]) {                                   // one byte per pixel crosses PCIe instead of four (or a float32 plane)
            LARS_TRY(lars_d_colormap_entry_f32(L.idx[k], (int64_t)npix, L.entry[k], s));
            if (j.out_rgba[k]) LARS_HIP_TRY(hipMemcpyAsync(j.out_rgba[k], L.entry[k], npix, hipMemcpyDeviceToHost, s));
        }
        if (L.png[k]) {                                     // the picture stays on the device; only its PNG file crosses PCIe
            if (L.pal[k]) LARS_HIP_TRY(hipMemcpyAsync(L.pal[k], j.cmap[k], 1024, hipMemcpyHostToDevice, s));
            LARS_TRY(lars_d_encode_png_u8(j.png_mode == 1 ? L.rgba[k] : L.entry[k], j.h, j.w, j.png_mode == 1 ? 4 : 1, L.pal[k],
                                          L.pal[k] ? 256 : 0, L.png[k], L.png_bound, L.png_len + k, L.png_scratch, s));
        }
    }
    TiffAnswer htif[3] = {{0, {0, 0}}, {0, {0, 0}}, {0, {0, 0}}};
    if (L.tif_ans) {                                        // the plane stays on the device; only its TIFF file crosses PCIe
        for (int k = 0; k < 3; ++k)
            if (L.tif[k])
                LARS_TRY((j.tiff_compression == 8 ? lars_d_encode_tiff_deflate_float32 : lars_d_encode_tiff_f32)(
                    L.idx[k], j.h, j.w, 1, j.tiff_rps, j.tiff_predictor, L.tif[k], L.tif_bound, &L.tif_ans[k].len, L.tif_ans[k].status, L.tif_scratch, s));
        LARS_HIP_TRY(hipMemcpyAsync(htif, L.tif_ans, sizeof htif, hipMemcpyDeviceToHost, s));
    }
    int64_t hlen[3] = {0, 0, 0};
    if (L.png_len) LARS_HIP_TRY(hipMemcpyAsync(hlen, L.png_len, sizeof hlen, hipMemcpyDeviceToHost, s));
    lars_stats hstats[3];
    float hmed[6];
    double hp[6];
    if (stats) LARS_HIP_TRY(hipMemcpyAsync(hstats, L.stats, sizeof hstats, hipMemcpyDeviceToHost, s));
    float hpairs[4] = {0, 0, 0, 0};
    if (L.pairs) LARS_HIP_TRY(hipMemcpyAsync(hpairs, L.pairs, sizeof hpairs, hipMemcpyDeviceToHost, s));
    else if (j.want_median && j.medians && j.mask) LARS_HIP_TRY(hipMemcpyAsync(hmed, L.med, sizeof hmed, hipMemcpyDeviceToHost, s));
    if (j.apply_wb && j.pcts) LARS_HIP_TRY(hipMemcpyAsync(hp, L.pcts, sizeof hp, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (L.pairs) {
        // {NDVI middles, GNDVI middles}; NDWI = -GNDVI: its two middles are the negated GNDVI middles in reverse order
        hmed[0] = hpairs[0]; hmed[1] = hpairs[1]; hmed[2] = hpairs[2]; hmed[3] = hpairs[3];
        hmed[4] = 0.0f - hpairs[3]; hmed[5] = 0.0f - hpairs[2];
        for (int k = 0; k < 3; ++k)
            if (((j.mask >> k) & 1u) && (hmed[2 * k] != hmed[2 * k] || hmed[2 * k + 1] != hmed[2 * k + 1]))
                return fail(LARS_ERR_HIP, "exact median select did not settle");
    }
    for (int k = 0; k < 3; ++k) {
        if (!((j.mask >> k) & 1u)) continue;
        if (stats && j.stats) j.stats[k] = hstats[k];
        if (j.want_median && j.medians) { j.medians[2 * k] = hmed[2 * k]; j.medians[2 * k + 1] = hmed[2 * k + 1]; }
    }
    if (j.apply_wb && j.pcts) memcpy(j.pcts, hp, sizeof hp);
    if (j.png_mode) {
        for (int k = 0; k < 3; ++k) {
            if (!L.png[k]) continue;
            if (hlen[k] <= 0 || (size_t)hlen[k] > j.png_cap)
                return fail(LARS_ERR_HIP, "lars_h_process_image_png: file %d has %lld bytes (capacity %zu)", k, (long long)hlen[k], j.png_cap);
            LARS_HIP_TRY(hipMemcpyAsync(j.out_png[k], L.png[k], (size_t)hlen[k], hipMemcpyDeviceToHost, s));
        }
        LARS_HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 3; ++k) j.png_len[k] = L.png[k] ? hlen[k] : 0;
    }
    if (j.tiff) {
        for (int k = 0; k < 3; ++k) {
            if (!L.tif[k]) continue;
            if (htif[k].status[0] != LARS_TIFE_OK || htif[k].len <= 0 || (size_t)htif[k].len > j.tiff_cap || (size_t)htif[k].len > L.tif_bound)
                return fail(LARS_ERR_HIP, "lars_h_process_image_tiff_f32: file %d has %lld bytes (capacity %zu, encoder status %d)", k,
                            (long long)htif[k].len, j.tiff_cap, htif[k].status[0]);
            LARS_HIP_TRY(hipMemcpyAsync(j.out_tiff[k], L.tif[k], (size_t)htif[k].len, hipMemcpyDeviceToHost, s));
        }
        LARS_HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 3; ++k) j.tiff_len[k] = L.tif[k] ? htif[k].len : 0;
    }
    return LARS_OK;
}

}  // namespace

template <typename T>
static int analyze_impl(const T *x, int64_t n, T thr, int want_hist, lars_stats *out, T *median_pair, double *sumsqdev)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || n <= 0 || !out) return fail(LARS_ERR_INVALID, "lars_h_analyze: bad arguments");
    T *dx, *dmed;
    lars_stats *dst;
    double *dss;
    char *dsel;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        dx = d.take<T>(n);
        dst = d.take<lars_stats>(1);
        dmed = d.take<T>(2);
        dss = d.take<double>(1);
        dsel = d.take<char>(lars_select_scratch_bytes());
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * sizeof(T), hipMemcpyHostToDevice, s));
    if (sizeof(T) == 4) {
        LARS_TRY(lars_d_array_stats_f32(reinterpret_cast<const float *>(dx), n, (float)thr, want_hist, dst, s));
        if (median_pair)
            LARS_TRY(lars_d_median_pair_f32(reinterpret_cast<const float *>(dx), n, reinterpret_cast<float *>(dmed), dsel, s));
    } else {
        LARS_TRY(lars_d_array_stats_f64(reinterpret_cast<const double *>(dx), n, (double)thr, want_hist, dst,
                                        sumsqdev ? dss : nullptr, s));
        if (median_pair)
            LARS_TRY(lars_d_median_pair_f64(reinterpret_cast<const double *>(dx), n, reinterpret_cast<double *>(dmed), dsel, s));
    }
    LARS_HIP_TRY(hipMemcpyAsync(out, dst, sizeof(lars_stats), hipMemcpyDeviceToHost, s));
    if (median_pair) LARS_HIP_TRY(hipMemcpyAsync(median_pair, dmed, 2 * sizeof(T), hipMemcpyDeviceToHost, s));
    if (sumsqdev) LARS_HIP_TRY(hipMemcpyAsync(sumsqdev, dss, sizeof(double), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

extern "C" {

int lars_h_fix_white_balance(const void *img, int64_t h, int64_t w, int channels, int dtype, int variant, uint8_t *out,
                             double *percentiles)
{
    if (!out) return fail(LARS_ERR_INVALID, "lars_h_fix_white_balance: out == NULL");
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = 1; j.wb_variant = variant; j.mask = 0; j.out_wb = out; j.pcts = percentiles;
    return run_image(j);
}

int lars_h_calculate_index(const void *img, int64_t h, int64_t w, int channels, int dtype, uint32_t index_mask,
                           float *const out[3], lars_stats *stats, int want_hist)
{
    if (!index_mask) return fail(LARS_ERR_INVALID, "lars_h_calculate_index: empty index mask");
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.mask = index_mask;
    for (int k = 0; k < 3; ++k) j.out_index[k] = out ? out[k] : nullptr;
    j.stats = stats; j.want_stats = stats != nullptr; j.want_hist = want_hist;
    return run_image(j);
}

int lars_h_process_image(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb,
                         uint32_t index_mask, int want_hist, uint8_t *out_wb, float *const out_index[3],
                         lars_stats *stats, float *medians, uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3])
{
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = apply_wb; j.mask = index_mask; j.out_wb = out_wb;
    for (int k = 0; k < 3; ++k) {
        j.out_index[k] = out_index ? out_index[k] : nullptr;
        j.out_rgba[k] = out_rgba ? out_rgba[k] : nullptr;
        j.cmap[k] = cmap_lut ? cmap_lut[k] : nullptr;
    }
    j.stats = stats; j.want_stats = stats != nullptr; j.want_hist = want_hist;
    j.medians = medians; j.want_median = medians != nullptr;
    if (!index_mask && !(apply_wb && out_wb)) return fail(LARS_ERR_INVALID, "lars_h_process_image: nothing requested");
    return run_image(j);
}

int lars_h_process_image_png(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                             int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                             const uint8_t *const cmap_lut[3], int png_mode, uint8_t *const out_png[3], size_t png_cap,
                             int64_t png_len[3])
{
    if (png_mode != 1 && png_mode != 2) return fail(LARS_ERR_INVALID, "lars_h_process_image_png: png_mode must be 1 (RGBA) or 2 (P)");
    if (!index_mask || (index_mask & ~LARS_MASK_ALL) || !cmap_lut || !out_png || !png_len)
        return fail(LARS_ERR_INVALID, "lars_h_process_image_png: indices, colormaps and PNG outputs are required");
    if (h <= 0 || w <= 0 || h > (1 << 24) || w > (1 << 24))
        return fail(LARS_ERR_INVALID, "lars_h_process_image_png: %lld x %lld image", (long long)h, (long long)w);
    const size_t bound = lars_png_bound(h, w, png_mode == 1 ? 4 : 1);
    for (int k = 0; k < 3; ++k)
        if (((index_mask >> k) & 1u) && (!cmap_lut[k] || !out_png[k]))
            return fail(LARS_ERR_INVALID, "lars_h_process_image_png: index %d needs cmap_lut and out_png", k);
    if (png_cap < bound) return fail(LARS_ERR_INVALID, "lars_h_process_image_png: png_cap %zu < lars_png_bound %zu", png_cap, bound);
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = apply_wb; j.mask = index_mask; j.out_wb = out_wb;
    for (int k = 0; k < 3; ++k) {
        j.out_index[k] = out_index ? out_index[k] : nullptr;
        j.cmap[k] = cmap_lut[k];
        j.out_png[k] = out_png[k];
    }
    j.stats = stats; j.want_stats = stats != nullptr; j.want_hist = want_hist;
    j.medians = medians; j.want_median = medians != nullptr;
    j.png_mode = png_mode; j.png_cap = png_cap; j.png_len = png_len;
    return run_image(j);
}

static int process_image_tiff(const char *who, int compression, const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb,
                              uint32_t index_mask, int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                              uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], int predictor, int64_t rows_per_strip,
                              uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3])
{
    if (!index_mask || (index_mask & ~LARS_MASK_ALL) || !out_tiff || !tiff_len)
        return fail(LARS_ERR_INVALID, "%s: indices and TIFF outputs are required", who);
    const size_t bound = compression == 8 ? lars_tiff_float32_deflate_bound(h, w, 1, rows_per_strip) : lars_tiff_f32_bound(h, w, 1, rows_per_strip);
    if (!bound)
        return fail(LARS_ERR_INVALID, "%s: %lld x %lld image in strips of %lld rows (1 to 2^24 on each side, strips of at most 2^30 bytes)", who,
                    (long long)h, (long long)w, (long long)rows_per_strip);
    for (int k = 0; k < 3; ++k)
        if (((index_mask >> k) & 1u) && !out_tiff[k]) return fail(LARS_ERR_INVALID, "%s: index %d needs out_tiff", who, k);
    if (tiff_cap < bound)
        return fail(LARS_ERR_INVALID, "%s: tiff_cap %zu < %s %zu", who, tiff_cap, compression == 8 ? "lars_tiff_float32_deflate_bound" : "lars_tiff_f32_bound",
                    bound);
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = apply_wb; j.mask = index_mask; j.out_wb = out_wb;
    for (int k = 0; k < 3; ++k) {
        j.out_index[k] = out_index ? out_index[k] : nullptr;
        j.out_rgba[k] = out_rgba ? out_rgba[k] : nullptr;
        j.cmap[k] = cmap_lut ? cmap_lut[k] : nullptr;
        j.out_tiff[k] = out_tiff[k];
    }
    j.stats = stats; j.want_stats = stats != nullptr; j.want_hist = want_hist;
    j.medians = medians; j.want_median = medians != nullptr;
    j.tiff = 1; j.tiff_compression = compression; j.tiff_predictor = predictor; j.tiff_rps = rows_per_strip; j.tiff_cap = tiff_cap;
    j.tiff_len = tiff_len;
    return run_image(j);
}

int lars_h_process_image_tiff_f32(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                  int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                  uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], int predictor, int64_t rows_per_strip,
                                  uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3])
{
    return process_image_tiff("lars_h_process_image_tiff_f32", 5, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index,
                              stats, medians, out_rgba, cmap_lut, predictor, rows_per_strip, out_tiff, tiff_cap, tiff_len);
}

int lars_h_process_image_tiff_float32(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                              int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                              uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], int compression, int predictor,
                                              int64_t rows_per_strip, uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3])
{
    static const char *who = "lars_h_process_image_tiff_float32";
    if (compression != 5 && compression != 8) return fail(LARS_ERR_INVALID, "%s: compression must be 5 (LZW) or 8 (Deflate), got %d", who, compression);
    return process_image_tiff(who, compression, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians,
                              out_rgba, cmap_lut, predictor, rows_per_strip, out_tiff, tiff_cap, tiff_len);
}

int lars_h_process_image_masked(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                int has_nodata, int nodata, int64_t *valid_pixels, int file_kind, int predictor, int64_t rows_per_strip,
                                uint8_t *const out_file[3], size_t file_cap, int64_t file_len[3])
{
    static const char *who = "lars_h_process_image_masked";
    if (valid_pixels) *valid_pixels = -1;
    if (!img || h <= 0 || w <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "%s: image must be a non-empty [h][w][>=3] array", who);
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "%s: dtype must be LARS_U8 or LARS_U16", who);
    if (index_mask & ~LARS_MASK_ALL) return fail(LARS_ERR_INVALID, "%s: unknown index bits in mask", who);
    if (!index_mask && !(apply_wb && out_wb)) return fail(LARS_ERR_INVALID, "%s: nothing requested", who);
    if (use_alpha && channels < 4) return fail(LARS_ERR_INVALID, "%s: the alpha rule needs 4 or more channels, got %d", who, channels);
    if (has_nodata && (nodata < 0 || nodata > (dtype == LARS_U8 ? 255 : 65535)))
        return fail(LARS_ERR_INVALID, "%s: nodata %d is outside the sample type's range", who, nodata);
    if (file_kind != 0 && file_kind != 1 && file_kind != 5 && file_kind != 8)
        return fail(LARS_ERR_INVALID, "%s: file_kind must be 0 (none), 1 (RGBA PNG), 5 (LZW TIFF) or 8 (Deflate TIFF), got %d", who, file_kind);
    for (int k = 0; k < 3; ++k)
        if (((index_mask >> k) & 1u) && out_rgba && out_rgba[k] && !(cmap_lut && cmap_lut[k]))
            return fail(LARS_ERR_INVALID, "%s: out_rgba[%d] needs cmap_lut[%d] (the 256 colormap entries leave no free one for \"no data\": "
                                          "entry planes are not built with a mask)", who, k, k);
    ImageJob j;
    memset(&j, 0, sizeof j);
    if (file_kind) {
        if (!index_mask || !out_file || !file_len) return fail(LARS_ERR_INVALID, "%s: indices and file outputs are required", who);
        const size_t bound = file_kind == 1 ? ((h > (1 << 24) || w > (1 << 24)) ? 0 : lars_png_bound(h, w, 4))
                           : file_kind == 8 ? lars_tiff_float32_deflate_bound(h, w, 1, rows_per_strip) : lars_tiff_f32_bound(h, w, 1, rows_per_strip);
        if (!bound) return fail(LARS_ERR_INVALID, "%s: a %lld x %lld picture is not encoded as this kind of file", who, (long long)h, (long long)w);
        if (file_cap < bound) return fail(LARS_ERR_INVALID, "%s: file_cap %zu < the bound %zu of this kind of file", who, file_cap, bound);
        for (int k = 0; k < 3; ++k) {
            if (!((index_mask >> k) & 1u)) continue;
            if (!out_file[k]) return fail(LARS_ERR_INVALID, "%s: index %d needs out_file", who, k);
            if (file_kind == 1 && !(cmap_lut && cmap_lut[k])) return fail(LARS_ERR_INVALID, "%s: index %d needs cmap_lut for its PNG", who, k);
        }
    }
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = apply_wb; j.mask = index_mask; j.out_wb = out_wb;
    for (int k = 0; k < 3; ++k) {
        j.out_index[k] = out_index ? out_index[k] : nullptr;
        j.out_rgba[k] = (out_rgba && file_kind != 1) ? out_rgba[k] : nullptr;
        j.cmap[k] = cmap_lut ? cmap_lut[k] : nullptr;
        if (file_kind == 1) j.out_png[k] = out_file[k];
        else if (file_kind) j.out_tiff[k] = out_file[k];
    }
    j.stats = stats; j.want_stats = stats != nullptr; j.want_hist = want_hist;
    j.medians = medians; j.want_median = medians != nullptr;
    if (file_kind == 1) { j.png_mode = 1; j.png_cap = file_cap; j.png_len = file_len; }
    else if (file_kind) {
        j.tiff = 1; j.tiff_compression = file_kind; j.tiff_predictor = predictor; j.tiff_rps = rows_per_strip; j.tiff_cap = file_cap;
        j.tiff_len = file_len;
    }
    j.masked = 1; j.valid = valid; j.use_alpha = use_alpha; j.has_nodata = has_nodata; j.nodata = nodata; j.valid_pixels = valid_pixels;
    return run_image(j);
}

int lars_h_process_image_zones(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                               int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                               uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                               int has_nodata, int nodata, int64_t *valid_pixels, const void *zones, int zone_bytes, int64_t nzones,
                               lars_stats *zone_stats, float *zone_medians, int64_t *bad_labels)
{
    static const char *who = "lars_h_process_image_zones";
    if (valid_pixels) *valid_pixels = -1;
    if (bad_labels) *bad_labels = -1;
    if (!img || h <= 0 || w <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "%s: image must be a non-empty [h][w][>=3] array", who);
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "%s: dtype must be LARS_U8 or LARS_U16", who);
    if (!index_mask || (index_mask & ~LARS_MASK_ALL)) return fail(LARS_ERR_INVALID, "%s: index_mask must name one to three indices", who);
    if (use_alpha && channels < 4) return fail(LARS_ERR_INVALID, "%s: the alpha rule needs 4 or more channels, got %d", who, channels);
    if (has_nodata && (nodata < 0 || nodata > (dtype == LARS_U8 ? 255 : 65535)))
        return fail(LARS_ERR_INVALID, "%s: nodata %d is outside the sample type's range", who, nodata);
    LARS_TRY(zone_arguments(who, zones, zone_bytes, nzones, zone_stats, zone_medians));
    for (int k = 0; k < 3; ++k)
        if (((index_mask >> k) & 1u) && out_rgba && out_rgba[k] && !(cmap_lut && cmap_lut[k]))
            return fail(LARS_ERR_INVALID, "%s: out_rgba[%d] needs cmap_lut[%d] (entry planes are not built with a mask)", who, k, k);
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = apply_wb; j.mask = index_mask; j.out_wb = out_wb;
    for (int k = 0; k < 3; ++k) {
        j.out_index[k] = out_index ? out_index[k] : nullptr;
        j.out_rgba[k] = out_rgba ? out_rgba[k] : nullptr;
        j.cmap[k] = cmap_lut ? cmap_lut[k] : nullptr;
    }
    j.stats = stats; j.want_stats = stats != nullptr; j.want_hist = want_hist;
    j.medians = medians; j.want_median = medians != nullptr;
    // the masked route even when no mask is given: the results are the same by definition
    j.masked = 1; j.valid = valid; j.use_alpha = use_alpha; j.has_nodata = has_nodata; j.nodata = nodata; j.valid_pixels = valid_pixels;
    j.zones = zones; j.zone_bytes = zone_bytes; j.nzones = nzones; j.zone_stats = zone_stats; j.zone_medians = zone_medians;
    j.bad_labels = bad_labels;
    return run_image(j);
}

int lars_h_zonal_stats_f32(const float *x, const void *zones, int zone_bytes, const uint8_t *valid, int64_t h, int64_t w, int64_t nzones,
                           float threshold, int want_hist, lars_stats *stats, float *medians, int64_t *bad_labels)
{
    static const char *who = "lars_h_zonal_stats_f32";
    if (bad_labels) *bad_labels = -1;
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || h <= 0 || w <= 0) return fail(LARS_ERR_INVALID, "%s: x must be a non-empty [h][w] float32 array", who);
    LARS_TRY(zone_arguments(who, zones, zone_bytes, nzones, stats, medians));
    const size_t npix = (size_t)h * w;
    float *dx;
    uint8_t *dvalid;
    ZoneBufs B;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        dx = d.take<float>(npix);
        dvalid = valid ? d.take<uint8_t>(npix) : nullptr;
        B = zone_plan(d, npix, zone_bytes, nzones, 1u);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, npix * sizeof(float), hipMemcpyHostToDevice, s));
    if (valid) LARS_HIP_TRY(hipMemcpyAsync(dvalid, valid, npix, hipMemcpyHostToDevice, s));
    const float *planes[3] = {dx, nullptr, nullptr};
    const float thr[3] = {threshold, threshold, threshold};
    LARS_TRY(run_zones(who, B, zones, zone_bytes, dvalid, (int64_t)npix, nzones, planes, 1u, thr, want_hist, stats, medians, bad_labels, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_valid_mask(const void *img, int64_t h, int64_t w, int channels, int dtype, int use_alpha, int has_nodata, int nodata,
                      uint8_t *out_mask, int64_t *valid_pixels)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out_mask || h <= 0 || w <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "lars_h_valid_mask: bad arguments");
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "lars_h_valid_mask: dtype must be LARS_U8 or LARS_U16");
    const size_t npix = (size_t)h * w, esz = dtype == LARS_U8 ? 1 : 2;
    uint8_t *dimg, *dmask;
    uint64_t *dcount;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dimg = d.take<uint8_t>(npix * channels * esz), dmask = d.take<uint8_t>(npix + 4), dcount = d.take<uint64_t>(1); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dimg, img, npix * channels * esz, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_valid_mask(dimg, (int64_t)npix, channels, dtype, nullptr, use_alpha, has_nodata, nodata, dmask, dcount, s));
    uint64_t n = 0;
    LARS_HIP_TRY(hipMemcpyAsync(out_mask, dmask, npix, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipMemcpyAsync(&n, dcount, sizeof n, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (valid_pixels) *valid_pixels = (int64_t)n;
    return LARS_OK;
}

int lars_h_calculate_index_planes(const float *red, const float *green, const float *nir, int64_t n, int index_id,
                                  float *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!red || !green || !nir || !out || n <= 0) return fail(LARS_ERR_INVALID, "lars_h_calculate_index_planes: bad arguments");
    float *dr, *dg, *dn, *dout;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dr = d.take<float>(n), dg = d.take<float>(n), dn = d.take<float>(n), dout = d.take<float>(n); }));
    hipStream_t s = c->stream;
    // only the two bands the index reads cross PCIe
    const float *ha = index_id == LARS_NDWI ? green : nir;
    const float *hb = index_id == LARS_NDVI ? red : (index_id == LARS_GNDVI ? green : nir);
    float *da = index_id == LARS_NDWI ? dg : dn;
    float *db = index_id == LARS_NDVI ? dr : (index_id == LARS_GNDVI ? dg : dn);
    LARS_HIP_TRY(hipMemcpyAsync(da, ha, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(db, hb, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_index_planes_f32(dr, dg, dn, n, index_id, dout, s));
    LARS_HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_ndvi_f64(const void *img, int64_t h, int64_t w, int channels, int dtype, double *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out || h <= 0 || w <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "lars_h_ndvi_f64: bad arguments");
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "lars_h_ndvi_f64: dtype");
    const size_t npix = (size_t)h * w, esz = dtype == LARS_U8 ? 1 : 2;
    uint8_t *dimg;
    double *dout;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dimg = d.take<uint8_t>(npix * channels * esz), dout = d.take<double>(npix); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dimg, img, npix * channels * esz, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_ndvi_f64(dimg, (int64_t)npix, channels, dtype, dout, s));
    LARS_HIP_TRY(hipMemcpyAsync(out, dout, npix * 8, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_analyze_f32(const float *x, int64_t n, float threshold, int want_hist, lars_stats *out, float median_pair[2])
{
    return analyze_impl<float>(x, n, threshold, want_hist, out, median_pair, nullptr);
}
int lars_h_analyze_f64(const double *x, int64_t n, double threshold, int want_hist, lars_stats *out, double median_pair[2],
                       double *sumsqdev)
{
    return analyze_impl<double>(x, n, threshold, want_hist, out, median_pair, sumsqdev);
}

int lars_h_threshold_mask_f32(const float *x, int64_t n, float threshold, uint8_t *out_mask)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || !out_mask || n <= 0) return fail(LARS_ERR_INVALID, "lars_h_threshold_mask_f32: bad arguments");
    float *dx;
    uint8_t *dm;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dx = d.take<float>(n), dm = d.take<uint8_t>((size_t)n + 4); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_threshold_mask_f32(dx, n, threshold, dm, s));
    LARS_HIP_TRY(hipMemcpyAsync(out_mask, dm, (size_t)n, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

// lars_h_colormap_f32 (range == nullptr) and lars_h_colormap_norm_f32 (range = {vmin, vmax})
static int colormap_impl(const char *who, const float *x, int64_t n, const float *range, const uint8_t *lut_rgba, uint8_t *out_rgba)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || !lut_rgba || !out_rgba || n <= 0) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    float *dx;
    uint8_t *dl, *dout;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dx = d.take<float>(n), dl = d.take<uint8_t>(1024), dout = d.take<uint8_t>((size_t)n * 4); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(dl, lut_rgba, 1024, hipMemcpyHostToDevice, s));
    LARS_TRY(range ? lars_d_colormap_norm_f32(dx, n, range[0], range[1], dl, dout, s) : lars_d_colormap_f32(dx, n, dl, dout, s));
    LARS_HIP_TRY(hipMemcpyAsync(out_rgba, dout, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_colormap_f32(const float *x, int64_t n, const uint8_t *lut_rgba, uint8_t *out_rgba)
{
    return colormap_impl("lars_h_colormap_f32", x, n, nullptr, lut_rgba, out_rgba);
}

int lars_h_colormap_norm_f32(const float *x, int64_t n, float vmin, float vmax, const uint8_t *lut_rgba, uint8_t *out_rgba)
{
    const float range[2] = {vmin, vmax};
    return colormap_impl("lars_h_colormap_norm_f32", x, n, range, lut_rgba, out_rgba);
}

// device-side registration of `moving` (device, uint8 [h][w][channels]) to `fixed`: estimate + apply
static int align_on_device(ThreadCtx *c, const uint8_t *d_fixed, const uint8_t *d_moving, int64_t h, int64_t w, int channels,
                           double *d_fa, double *d_fb, void *d_scratch, int64_t *d_shift, uint8_t *d_aligned, hipStream_t s)
{
    const int64_t npix = h * w;
    LARS_TRY(lars_d_gray_c128(d_fixed, npix, channels, d_fa, s));
    LARS_TRY(lars_d_gray_c128(d_moving, npix, channels, d_fb, s));
    LARS_TRY(lars_d_phase_correlation(d_fa, d_fb, h, w, d_shift, d_scratch, s));
    LARS_TRY(lars_d_shift_reflect_u8(d_moving, h, w, channels, d_shift, d_aligned, s));
    return LARS_OK;
}

int lars_h_align_images(const uint8_t *fixed, const uint8_t *moving, int64_t h, int64_t w, int channels, uint8_t *out_aligned,
                        double shift[2])
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!fixed || !moving || !out_aligned || h <= 0 || w <= 0 || (channels != 1 && channels != 3))
        return fail(LARS_ERR_INVALID, "lars_h_align_images: two uint8 [h][w][3] (or [h][w]) images of the same shape are required");
    const size_t npix = (size_t)h * w, nbytes = npix * channels;
    uint8_t *df, *dm, *da;
    double *fa, *fb;
    char *sc;
    int64_t *dshift;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        df = d.take<uint8_t>(nbytes), dm = d.take<uint8_t>(nbytes), da = d.take<uint8_t>(nbytes);
        fa = d.take<double>(npix * 2), fb = d.take<double>(npix * 2);
        sc = d.take<char>(lars_phase_scratch_bytes());
        dshift = d.take<int64_t>(2);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(df, fixed, nbytes, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(dm, moving, nbytes, hipMemcpyHostToDevice, s));
    LARS_TRY(align_on_device(c, df, dm, h, w, channels, fa, fb, sc, dshift, da, s));
    int64_t hs[2] = {0, 0};
    LARS_HIP_TRY(hipMemcpyAsync(out_aligned, da, nbytes, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipMemcpyAsync(hs, dshift, sizeof hs, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (shift) { shift[0] = (double)hs[0]; shift[1] = (double)hs[1]; }
    return LARS_OK;
}

int lars_h_change_detection(const uint8_t *early, const uint8_t *late, int64_t h, int64_t w, int channels, int wb_early,
                            int wb_late, int align, int index_id, float *out_early, float *out_late, float *out_diff,
                            uint8_t *out_rgba_diff, const uint8_t *lut_rgba, float vmin, float vmax,
                            uint8_t *out_aligned_late, double shift[2])
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!early || !late || h <= 0 || w <= 0 || channels < 3)
        return fail(LARS_ERR_INVALID, "lars_h_change_detection: two uint8 [h][w][>=3] images of the same shape are required");
    if (index_id < 0 || index_id > 2) return fail(LARS_ERR_INVALID, "lars_h_change_detection: index_id");
    if (align && channels != 3) return fail(LARS_ERR_INVALID, "lars_h_change_detection: registration needs 3-channel images (rgb2gray)");
    if (out_rgba_diff && !lut_rgba) return fail(LARS_ERR_INVALID, "lars_h_change_detection: out_rgba_diff needs lut_rgba");
    const size_t npix = (size_t)h * w, nbytes = npix * channels;
    const size_t tbytes = lars_wb_table_bytes(LARS_U8);
    Carver cv(nullptr);
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0 sizes the workspace, pass 1 carves it
        if (pass == 1) { LARS_TRY(ws_reserve(c, cv.off + 256)); cv = Carver(c->ws); }
        Carver &d = cv;
        uint8_t *d_e = d.take<uint8_t>(nbytes), *d_l = d.take<uint8_t>(nbytes);
        uint8_t *d_ewb = d.take<uint8_t>(nbytes), *d_lwb = d.take<uint8_t>(nbytes), *d_al = d.take<uint8_t>(nbytes);
        uint8_t *d_tab = d.take<uint8_t>(tbytes);
        double *d_pct = d.take<double>(6);
        double *fa = d.take<double>(align ? npix * 2 : 1), *fb = d.take<double>(align ? npix * 2 : 1);
        char *sc = d.take<char>(lars_phase_scratch_bytes());
        int64_t *d_shift = d.take<int64_t>(2);
        float *d_ie = d.take<float>(npix), *d_il = d.take<float>(npix), *d_df = d.take<float>(npix);
        uint8_t *d_rgba = d.take<uint8_t>(out_rgba_diff ? npix * 4 : 1), *d_lut = d.take<uint8_t>(1024);
        if (pass == 0) continue;

        hipStream_t s = c->stream;
        LARS_HIP_TRY(hipMemcpyAsync(d_e, early, nbytes, hipMemcpyHostToDevice, s));
        LARS_HIP_TRY(hipMemcpyAsync(d_l, late, nbytes, hipMemcpyHostToDevice, s));
        LARS_HIP_TRY(hipMemsetAsync(d_shift, 0, 2 * sizeof(int64_t), s));
        // white balance where the caller holds no cached corrected array (process-images.py:894-902)
        const uint8_t *src[2] = {d_e, d_l};
        uint8_t *wb_out[2] = {d_ewb, d_lwb};
        const int want_wb[2] = {wb_early, wb_late};
        for (int k = 0; k < 2; ++k) {
            if (!want_wb[k]) continue;
            LARS_TRY(lars_d_wb_prepare(src[k], 1, (int64_t)npix, channels, LARS_U8, d_tab, d_pct, 0, s));
            lars_fused_args a;
            memset(&a, 0, sizeof a);
            a.tiles = src[k]; a.ntiles = 1; a.npix = (int64_t)npix; a.channels = channels; a.dtype = LARS_U8;
            a.wb_table = d_tab; a.out_wb = wb_out[k]; a.stream = s;
            LARS_TRY(lars_d_fused(&a));
            src[k] = wb_out[k];
        }
        // registration of the late image onto the early one (:905-908)
        const uint8_t *late_final = src[1];
        if (align) {
            LARS_TRY(align_on_device(c, src[0], src[1], h, w, channels, fa, fb, sc, d_shift, d_al, s));
            late_final = d_al;
        }
        // indices (:911-919), difference (:923) and its colour map (:956)
        const uint8_t *imgs[2] = {src[0], late_final};
        float *idx[2] = {d_ie, d_il};
        for (int k = 0; k < 2; ++k) {
            lars_fused_args a;
            memset(&a, 0, sizeof a);
            a.tiles = imgs[k]; a.ntiles = 1; a.npix = (int64_t)npix; a.channels = channels; a.dtype = LARS_U8;
            a.index_mask = 1u << index_id; a.out_index[index_id] = idx[k]; a.stream = s;
            LARS_TRY(lars_d_fused(&a));
        }
        LARS_TRY(lars_d_diff_f32(d_ie, d_il, (int64_t)npix, d_df, s));
        if (out_rgba_diff) {
            LARS_HIP_TRY(hipMemcpyAsync(d_lut, lut_rgba, 1024, hipMemcpyHostToDevice, s));
            LARS_TRY(lars_d_colormap_norm_f32(d_df, (int64_t)npix, vmin, vmax, d_lut, d_rgba, s));
            LARS_HIP_TRY(hipMemcpyAsync(out_rgba_diff, d_rgba, npix * 4, hipMemcpyDeviceToHost, s));
        }
        int64_t hs[2] = {0, 0};
        if (out_early) LARS_HIP_TRY(hipMemcpyAsync(out_early, d_ie, npix * 4, hipMemcpyDeviceToHost, s));
        if (out_late) LARS_HIP_TRY(hipMemcpyAsync(out_late, d_il, npix * 4, hipMemcpyDeviceToHost, s));
        if (out_diff) LARS_HIP_TRY(hipMemcpyAsync(out_diff, d_df, npix * 4, hipMemcpyDeviceToHost, s));
        if (out_aligned_late) LARS_HIP_TRY(hipMemcpyAsync(out_aligned_late, late_final, nbytes, hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipMemcpyAsync(hs, d_shift, sizeof hs, hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipStreamSynchronize(s));
        if (shift) { shift[0] = (double)hs[0]; shift[1] = (double)hs[1]; }
    }
    return LARS_OK;
}

}  // extern "C"
