// The picture path of the host entry points: fix_white_balance, calculate_index, process_image and its PNG, TIFF, masked, zones,
// polygons and regions variants, and valid_mask.  Every picture entry point fills an ImageJob (picture_job plus what is its own) and
// hands it to run_image, which decides the route once (route_of) and then runs a short sequence of stages: plan, upload, planes and
// statistics (one runner per route), pictures, TIFF, collect, fetch files.  Zones are seen only through host_zones.h: a job names
// where its labels come from (ZoneSource), and the masked runner ends with run_zones (host_zones.cpp).
#include <string.h>

#include "host_zones.h"

using namespace lars;

namespace {

// ---- the job: what an entry point asks for ----
struct ImageJob {
    const char *who;              // the entry point, for messages
    const void *img;
    int64_t h, w;
    int channels, dtype;
    int apply_wb, wb_variant;
    uint32_t mask;
    int want_hist;
    uint8_t *out_wb;
    float *out_index[3];
    lars_stats *stats;            // [3], or null: no records
    float *medians;               // [3][2], or null: no medians
    uint8_t *out_rgba[3];
    const uint8_t *cmap[3];
    double *pcts;                 // [3][2]
    // at most one kind of file per job, encoded on the device: only the files cross PCIe
    int png_mode;                 // 0 none, 1 RGBA colormap pictures, 2 palette pictures of the colormap entries
    int tiff;                     // 0 none, float32 files of the index planes: 5 LZW, 8 Deflate
    int tiff_predictor;
    int64_t tiff_rps;
    uint8_t *out_file[3];
    size_t file_cap;
    int64_t *file_len;            // [3]
    // nodata-aware job (masked.hip): pixels outside the mask take no part in the percentiles and the statistics
    int masked;
    const uint8_t *valid;         // [h][w], nonzero = picture, or null
    int use_alpha, has_nodata, nodata;
    int64_t *valid_pixels;
    // ... with one record per zone and index as well (zonal.hip): the planes stay on the device for the zone stages
    const ZoneSource *zone_src;   // where the labels come from (a raster, polygons or regions), or null: no zones
    ZoneOutputs zone_out;         // the caller's per-zone arrays, zone_src->rows() rows to each index
};

// The head every picture entry point shares, in the order of their prototypes; each entry point adds only what is its own.
ImageJob picture_job(const char *who, const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                     int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                     uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3])
{
    ImageJob j;
    memset(&j, 0, sizeof j);
    j.who = who;
    j.img = img; j.h = h; j.w = w; j.channels = channels; j.dtype = dtype;
    j.apply_wb = apply_wb; j.mask = index_mask; j.out_wb = out_wb;
    for (int k = 0; k < 3; ++k) {
        j.out_index[k] = out_index ? out_index[k] : nullptr;
        j.out_rgba[k] = out_rgba ? out_rgba[k] : nullptr;
        j.cmap[k] = cmap_lut ? cmap_lut[k] : nullptr;
    }
    j.stats = stats; j.want_hist = want_hist; j.medians = medians;
    return j;
}

void under_mask(ImageJob &j, const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels)
{
    j.masked = 1; j.valid = valid; j.use_alpha = use_alpha; j.has_nodata = has_nodata; j.nodata = nodata; j.valid_pixels = valid_pixels;
}

size_t tiff_bound(int compression, int64_t h, int64_t w, int64_t rows_per_strip)
{
    return compression == 8 ? lars_tiff_float32_deflate_bound(h, w, 1, rows_per_strip) : lars_tiff_f32_bound(h, w, 1, rows_per_strip);
}

// The files of a job, checked before anything touches the device.  kind: 1 / 2 PNG (RGBA / P), 5 / 8 TIFF (LZW / Deflate)
int want_files(ImageJob &j, int kind, int predictor, int64_t rows_per_strip, uint8_t *const out[3], size_t cap, int64_t len[3])
{
    if (!j.mask || (j.mask & ~LARS_MASK_ALL) || !out || !len || j.png_mode || j.tiff)      // collect() and fetch_files() rely on the one kind
        return fail(LARS_ERR_INVALID, "%s: indices and file outputs are required, and a job has one kind of file", j.who);
    const size_t bound = kind >= 5 ? tiff_bound(kind, j.h, j.w, rows_per_strip)
                       : (j.h <= 0 || j.w <= 0 || j.h > (1 << 24) || j.w > (1 << 24)) ? 0 : lars_png_bound(j.h, j.w, kind == 1 ? 4 : 1);
    if (!bound)
        return fail(LARS_ERR_INVALID, "%s: a %lld x %lld picture is not encoded as this kind of file (1 to 2^24 on each side; TIFF in strips of "
                                      "%lld rows, of at most 2^30 bytes)", j.who, (long long)j.h, (long long)j.w, (long long)rows_per_strip);
    const char *bound_of = kind <= 2 ? "lars_png_bound" : kind == 8 ? "lars_tiff_float32_deflate_bound" : "lars_tiff_f32_bound";
    if (cap < bound) return fail(LARS_ERR_INVALID, "%s: capacity %zu of the file buffers (png_cap, tiff_cap, file_cap) < %s %zu", j.who, cap, bound_of, bound);
    for (int k = 0; k < 3; ++k) {
        if (!((j.mask >> k) & 1u)) continue;
        if (!out[k]) return fail(LARS_ERR_INVALID, "%s: index %d needs out_file", j.who, k);
        if (kind <= 2 && !j.cmap[k]) return fail(LARS_ERR_INVALID, "%s: index %d needs cmap_lut for its PNG", j.who, k);
        j.out_file[k] = out[k];
    }
    j.png_mode = kind <= 2 ? kind : 0; j.tiff = kind >= 5 ? kind : 0; j.tiff_predictor = predictor; j.tiff_rps = rows_per_strip;
    j.file_cap = cap; j.file_len = len;
    return LARS_OK;
}

int check_image(const char *who, const void *img, int64_t h, int64_t w, int channels, int dtype)
{
    if (!img || h <= 0 || w <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "%s: image must be a non-empty [h][w][>=3] array", who);
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "%s: dtype must be LARS_U8 or LARS_U16", who);
    return LARS_OK;
}

// what the entry points that take a mask check before they touch the device
int check_picture(const char *who, const void *img, int64_t h, int64_t w, int channels, int dtype, uint32_t index_mask, int use_alpha,
                  int has_nodata, int nodata, uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3])
{
    LARS_TRY(check_image(who, img, h, w, channels, dtype));
    if (use_alpha && channels < 4) return fail(LARS_ERR_INVALID, "%s: the alpha rule needs 4 or more channels, got %d", who, channels);
    if (has_nodata && (nodata < 0 || nodata > (dtype == LARS_U8 ? 255 : 65535)))
        return fail(LARS_ERR_INVALID, "%s: nodata %d is outside the sample type's range", who, nodata);
    for (int k = 0; k < 3; ++k)
        if (((index_mask >> k) & 1u) && out_rgba && out_rgba[k] && !(cmap_lut && cmap_lut[k]))
            return fail(LARS_ERR_INVALID, "%s: out_rgba[%d] needs cmap_lut[%d] (the 256 colormap entries leave no free one for \"no data\": "
                                          "entry planes are not built with a mask)", who, k, k);
    return LARS_OK;
}

// The head the picture-plus-zones entry points share: the out-parameters reset, every check that is not the source's own, and the
// job with its mask and its zone outputs.  Each entry point adds only the checks of its source (src must outlive the job).
int zones_job(ImageJob *j, const char *who, const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
              int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians, uint8_t *const out_rgba[3],
              const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
              const ZoneSource &src, const ZoneOutputs &out)
{
    if (valid_pixels) *valid_pixels = -1;
    reset_zone_outputs(src, out.bad_labels);
    LARS_TRY(check_picture(who, img, h, w, channels, dtype, index_mask, use_alpha, has_nodata, nodata, out_rgba, cmap_lut));
    if (!index_mask || (index_mask & ~LARS_MASK_ALL)) return fail(LARS_ERR_INVALID, "%s: index_mask must name one to three indices", who);
    LARS_TRY(check_zone_records(who, src, out.stats, out.medians));
    *j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut);
    // the masked route even when no mask is given: the results are the same by definition
    under_mask(*j, valid, use_alpha, has_nodata, nodata, valid_pixels);
    j->zone_src = &src;
    j->zone_out = out;
    return LARS_OK;
}

// ---- the route: which path produces the planes and the statistics, and which float32 planes must exist on the device ----
struct Route {
    enum Planes {
        FUSED,          // one fused launch; medians, where wanted, by a select over each float32 plane
        FUSED_SELECT,   // ... medians of uint8 RGNir images by the two-level select on recomputed values (select_q.hip): two passes
                        // over the 3-byte pixels instead of four or more over each 4-byte plane
        STATS_MEDIANS,  // ... and when no plane is wanted (one index or all three), the statistics kernel counts the select's first
                        // pass itself: the planes never exist on the device either
        MASKED          // nodata-aware (masked.hip): records and medians from the compacted valid values
    } planes;
    bool select;        // FUSED_SELECT or STATS_MEDIANS: the medians arrive as pairs
    bool stats;         // records are computed and copied back
    bool medians;       // medians are computed and copied back
    bool entry[3];      // a colormap entry plane (out_rgba[k] without a cmap_lut[k], or a palette PNG)
    bool rgba[3];       // an RGBA colormap picture (for the caller or for its PNG)
    bool plane[3];      // a float32 plane on the device
};

Route route_of(const ImageJob &j)
{
    Route r;
    r.stats = j.stats && j.mask;
    r.medians = j.medians && j.mask;
    r.select = r.medians && !j.masked && j.dtype == LARS_U8 && j.channels == 3 && (long long)j.h * j.w * 6 < (1ll << 30);
    bool lean = r.select && j.stats && !j.png_mode && !j.tiff && (j.mask == 1u || j.mask == 2u || j.mask == 4u || j.mask == 7u);
    for (int k = 0; k < 3; ++k)
        if (j.out_index[k] || j.out_rgba[k]) lean = false;
    r.planes = j.masked ? Route::MASKED : lean ? Route::STATS_MEDIANS : r.select ? Route::FUSED_SELECT : Route::FUSED;
    for (int k = 0; k < 3; ++k) {
        const bool on = (j.mask >> k) & 1u;
        r.entry[k] = on && ((j.out_rgba[k] && !j.cmap[k]) || j.png_mode == 2);
        r.rgba[k] = on && j.cmap[k] && (j.out_rgba[k] || j.png_mode == 1);
        const bool for_caller = j.out_index[k] != nullptr;                       // it is copied back
        const bool for_entries = r.entry[k];                                     // the entry plane is derived from it on the device
        const bool for_tiff = j.tiff != 0;                                       // its file is encoded from it
        const bool for_zones = j.zone_src != nullptr;                            // the zone stages scatter it
        const bool for_median = r.medians && r.planes == Route::FUSED;           // the select over the plane reads it
        r.plane[k] = on && (for_caller || for_entries || for_tiff || for_zones || for_median);
    }
    return r;
}

// ---- the device buffers of a job ----
struct FileAnswer { int64_t len; int32_t status[2]; };     // what the TIFF encoder leaves on the device; PNG: the length alone

struct Layout {
    uint8_t *img; uint8_t *table; double *pcts; uint8_t *wb;
    float *idx[3]; lars_stats *stats; float *med; char *sel; uint8_t *rgba[3]; uint8_t *cmap[3];
    uint8_t *entry[3];             // colormap entry planes: one byte per pixel
    float *pairs; char *selq;      // the select on recomputed values
    uint8_t *png[3], *pal[3];      // PNG files of the index pictures, palettes of the P pictures
    int64_t *png_len; char *png_scratch;
    size_t png_bound;
    uint8_t *tif[3];               // float32 TIFF files of the index planes
    FileAnswer *tif_ans; char *tif_scratch;
    size_t tif_bound;
    uint8_t *vmask;                // masked jobs: one byte per pixel, 1 = picture
    uint64_t *vcount;              // {|V|, cursor of the compaction}
    uint32_t *vhist;               // channel histograms of the valid pixels
    float *vals[3];                // the valid values of each index, compacted
    ZoneBufs zone;                 // jobs with zones
};

size_t select_slot() { return (lars_select_scratch_bytes() + 255) & ~(size_t)255; }      // L.sel holds one per index

Layout plan(const ImageJob &j, const Route &r, Carver &c)
{
    Layout L;
    const size_t npix = (size_t)j.h * j.w;
    const size_t esz = j.dtype == LARS_U8 ? 1 : 2;
    const size_t nval = j.dtype == LARS_U8 ? 256 : 65536;
    L.img = c.take<uint8_t>(npix * j.channels * esz);
    L.table = j.apply_wb ? c.take<uint8_t>(lars_wb_table_bytes(j.dtype)) : nullptr;
    L.pcts = j.apply_wb ? c.take<double>(6) : nullptr;
    L.wb = (j.apply_wb && j.out_wb) ? c.take<uint8_t>(npix * j.channels) : nullptr;
    const int png_channels = j.png_mode == 1 ? 4 : 1;
    L.png_bound = j.png_mode ? lars_png_bound(j.h, j.w, png_channels) : 0;
    for (int k = 0; k < 3; ++k) {
        const bool on = (j.mask >> k) & 1u;
        L.idx[k] = r.plane[k] ? c.take<float>(npix) : nullptr;
        L.rgba[k] = r.rgba[k] ? c.take<uint8_t>(npix * 4) : nullptr;
        L.cmap[k] = r.rgba[k] ? c.take<uint8_t>(1024) : nullptr;
        L.entry[k] = r.entry[k] ? c.take<uint8_t>(npix + 4) : nullptr;
        L.pal[k] = (on && j.png_mode == 2) ? c.take<uint8_t>(1024) : nullptr;
        L.png[k] = (on && j.png_mode) ? c.take<uint8_t>(L.png_bound) : nullptr;
    }
    L.tif_bound = j.tiff ? tiff_bound(j.tiff, j.h, j.w, j.tiff_rps) : 0;
    for (int k = 0; k < 3; ++k) L.tif[k] = (j.tiff && ((j.mask >> k) & 1u)) ? c.take<uint8_t>(L.tif_bound) : nullptr;
    L.tif_ans = j.tiff ? c.take<FileAnswer>(3) : nullptr;
    L.tif_scratch = !j.tiff ? nullptr : c.take<char>(j.tiff == 8 ? lars_tiff_float32_deflate_encode_scratch_bytes(j.h, j.w, 1, j.tiff_rps)
                                                                 : lars_tiff_f32_encode_scratch_bytes(j.h, j.w, 1, j.tiff_rps));
    L.png_len = j.png_mode ? c.take<int64_t>(3) : nullptr;
    L.png_scratch = j.png_mode ? c.take<char>(lars_png_scratch_bytes(j.h, j.w, png_channels)) : nullptr;
    L.stats = c.take<lars_stats>(3);
    L.med = c.take<float>(6);
    L.sel = c.take<char>(3 * select_slot());
    L.pairs = r.select ? c.take<float>(4) : nullptr;
    L.selq = r.select ? c.take<char>(lars_quotient_median_scratch_bytes(1)) : nullptr;
    L.vmask = j.masked ? c.take<uint8_t>(npix + 4) : nullptr;
    L.vcount = j.masked ? c.take<uint64_t>(2) : nullptr;
    L.vhist = (j.masked && j.apply_wb) ? c.take<uint32_t>(3 * nval) : nullptr;
    for (int k = 0; k < 3; ++k)
        L.vals[k] = (j.masked && ((j.mask >> k) & 1u) && (j.stats || j.medians)) ? c.take<float>(npix) : nullptr;
    if (j.zone_src) L.zone = plan_zones(c, *j.zone_src, j.mask);
    return L;
}

// ---- stage 3: planes and statistics, one runner per route ----
// the fused step's arguments, the colormap tables uploaded; `stats`: the kernel keeps the records itself
int fused_args(const ImageJob &j, const Layout &L, bool stats, hipStream_t s, lars_fused_args *a)
{
    memset(a, 0, sizeof *a);
    a->tiles = L.img; a->ntiles = 1; a->npix = j.h * j.w; a->channels = j.channels; a->dtype = j.dtype;
    a->wb_table = j.apply_wb ? L.table : nullptr;
    a->index_mask = j.mask;
    a->flags = stats ? (LARS_F_STATS | (j.want_hist ? LARS_F_HIST : 0u)) : 0u;
    for (int k = 0; k < 3; ++k) {
        a->out_index[k] = L.idx[k];
        a->out_rgba[k] = L.rgba[k];
        a->cmap_lut[k] = L.cmap[k];
        if (L.cmap[k]) LARS_HIP_TRY(hipMemcpyAsync(L.cmap[k], j.cmap[k], 1024, hipMemcpyHostToDevice, s));
    }
    a->out_wb = L.wb;
    a->stats = stats ? L.stats : nullptr;
    a->stream = s;
    return LARS_OK;
}

// FUSED and FUSED_SELECT
int run_fused(const ImageJob &j, const Route &r, const Layout &L, hipStream_t s)
{
    const int64_t npix = j.h * j.w;
    if (j.apply_wb) LARS_TRY(lars_d_wb_prepare(L.img, 1, npix, j.channels, j.dtype, L.table, L.pcts, j.wb_variant, s));
    if (!j.mask && !L.wb) return LARS_OK;
    lars_fused_args a;
    LARS_TRY(fused_args(j, L, r.stats, s, &a));
    LARS_TRY(lars_d_fused(&a));
    if (r.select)
        return lars_d_quotient_median_pairs(L.img, 1, npix, 3, LARS_U8, a.wb_table, ((j.mask & 1u) ? 1u : 0u) | ((j.mask & 6u) ? 2u : 0u),
                                            L.pairs, L.selq, s);
    for (int k = 0; k < 3; ++k)
        if (r.medians && ((j.mask >> k) & 1u)) LARS_TRY(lars_d_median_pair_f32(L.idx[k], npix, L.med + 2 * k, L.sel + k * select_slot(), s));
    return LARS_OK;
}

// STATS_MEDIANS: the white-balanced image on its own where it is wanted, then statistics + medians
int run_stats_medians(const ImageJob &j, const Layout &L, hipStream_t s)
{
    if (j.apply_wb) LARS_TRY(lars_d_wb_prepare(L.img, 1, j.h * j.w, j.channels, j.dtype, L.table, L.pcts, j.wb_variant, s));
    lars_fused_args a;
    LARS_TRY(fused_args(j, L, true, s, &a));
    if (L.wb) {
        lars_fused_args w = a;
        w.index_mask = 0; w.flags = 0; w.stats = nullptr;
        LARS_TRY(lars_d_fused(&w));
        a.out_wb = nullptr;
    }
    return lars_d_stats_medians(&a, L.pairs, L.selq);
}

// MASKED: the mask and |V|, the histograms of the valid pixels and their tables, the planes, and the record and the median of each
// index from its compacted values.  |V| crosses to the host once: the table, statistics and select launches are sized by it.
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
    if (!nvalid) return fail(LARS_ERR_INVALID, "%s: no valid pixel", j.who);
    if (j.apply_wb) {
        LARS_TRY(lars_d_masked_channel_hist(L.img, npix, j.channels, j.dtype, L.vmask, L.vhist, s));
        LARS_TRY(lars_d_wb_table(L.vhist, 1, (int64_t)nvalid, j.dtype, L.table, L.pcts, j.wb_variant, s));
    }
    if (!j.mask && !L.wb) return LARS_OK;
    lars_fused_args a;
    LARS_TRY(fused_args(j, L, false, s, &a));
    LARS_TRY(lars_d_masked_fused(&a, L.vmask, L.vals, L.vcount + 1));
    for (int k = 0; k < 3; ++k) {
        if (!L.vals[k]) continue;
        // process-images.py:498-504: coverage above 0.2, water (NDWI) above 0
        if (j.stats) LARS_TRY(lars_d_array_stats_f32(L.vals[k], (int64_t)nvalid, k == LARS_NDWI ? 0.0f : 0.2f, j.want_hist, L.stats + k, s));
        if (j.medians) LARS_TRY(lars_d_median_pair_f32(L.vals[k], (int64_t)nvalid, L.med + 2 * k, L.sel + k * select_slot(), s));
    }
    if (!j.zone_src) return LARS_OK;
    const ZonePlanes in = {{L.idx[0], L.idx[1], L.idx[2]}, j.mask, L.vmask, {0.2f, 0.2f, 0.0f}, j.want_hist};     // the thresholds of the records above
    return run_zones(j.who, *j.zone_src, L.zone, in, j.zone_out, s);
}

// ---- stage 4: the planes and pictures back, entry planes and PNG files built from what stays on the device ----
int send_pictures(const ImageJob &j, const Layout &L, hipStream_t s)
{
    const size_t npix = (size_t)j.h * j.w;
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
    return LARS_OK;
}

// ---- stage 5: the planes stay on the device; only their TIFF files cross PCIe.  The answers are on the stream when this returns ----
int encode_tiffs(const ImageJob &j, const Layout &L, hipStream_t s, FileAnswer answers[3])
{
    if (!j.tiff) return LARS_OK;
    for (int k = 0; k < 3; ++k)
        if (L.tif[k])
            LARS_TRY((j.tiff == 8 ? lars_d_encode_tiff_deflate_float32 : lars_d_encode_tiff_f32)(
                L.idx[k], j.h, j.w, 1, j.tiff_rps, j.tiff_predictor, L.tif[k], L.tif_bound, &L.tif_ans[k].len, L.tif_ans[k].status, L.tif_scratch, s));
    LARS_HIP_TRY(hipMemcpyAsync(answers, L.tif_ans, 3 * sizeof(FileAnswer), hipMemcpyDeviceToHost, s));
    return LARS_OK;
}

// ---- stage 6: the small results, and the one synchronise every job has ----
int collect(const ImageJob &j, const Route &r, const Layout &L, hipStream_t s, FileAnswer png[3])
{
    int64_t png_len[3] = {0, 0, 0};
    lars_stats hstats[3];
    float hmed[6], hpairs[4] = {0, 0, 0, 0};
    double hp[6];
    if (L.png_len) LARS_HIP_TRY(hipMemcpyAsync(png_len, L.png_len, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (r.stats) LARS_HIP_TRY(hipMemcpyAsync(hstats, L.stats, sizeof hstats, hipMemcpyDeviceToHost, s));
    if (r.select) LARS_HIP_TRY(hipMemcpyAsync(hpairs, L.pairs, sizeof hpairs, hipMemcpyDeviceToHost, s));
    else if (r.medians) LARS_HIP_TRY(hipMemcpyAsync(hmed, L.med, sizeof hmed, hipMemcpyDeviceToHost, s));
    if (j.apply_wb && j.pcts) LARS_HIP_TRY(hipMemcpyAsync(hp, L.pcts, sizeof hp, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (r.select) {
        // {NDVI middles, GNDVI middles}; NDWI = -GNDVI: its two middles are the negated GNDVI middles in reverse order
        hmed[0] = hpairs[0]; hmed[1] = hpairs[1]; hmed[2] = hpairs[2]; hmed[3] = hpairs[3];
        hmed[4] = 0.0f - hpairs[3]; hmed[5] = 0.0f - hpairs[2];
        for (int k = 0; k < 3; ++k)
            if (((j.mask >> k) & 1u) && (hmed[2 * k] != hmed[2 * k] || hmed[2 * k + 1] != hmed[2 * k + 1]))
                return fail(LARS_ERR_HIP, "exact median select did not settle");
    }
    for (int k = 0; k < 3; ++k) {
        if (!((j.mask >> k) & 1u)) continue;
        if (r.stats) j.stats[k] = hstats[k];
        if (r.medians) { j.medians[2 * k] = hmed[2 * k]; j.medians[2 * k + 1] = hmed[2 * k + 1]; }
    }
    if (j.apply_wb && j.pcts) memcpy(j.pcts, hp, sizeof hp);
    for (int k = 0; k < 3 && L.png_len; ++k) png[k].len = png_len[k];
    return LARS_OK;
}

// ---- stage 7: the files of one kind, now that their lengths are known: checked, copied, waited for (PNG: the status stays 0) ----
int fetch_files(const ImageJob &j, uint8_t *const dev[3], size_t bound, const FileAnswer got[3], hipStream_t s)
{
    for (int k = 0; k < 3; ++k) {
        if (!dev[k]) continue;
        if (got[k].status[0] != LARS_TIFE_OK || got[k].len <= 0 || (size_t)got[k].len > j.file_cap || (size_t)got[k].len > bound)
            return fail(LARS_ERR_HIP, "%s: file %d has %lld bytes (capacity %zu; status of the TIFF encoder %d)", j.who, k, (long long)got[k].len, j.file_cap,
                        got[k].status[0]);
        LARS_HIP_TRY(hipMemcpyAsync(j.out_file[k], dev[k], (size_t)got[k].len, hipMemcpyDeviceToHost, s));
    }
    LARS_HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) j.file_len[k] = dev[k] ? got[k].len : 0;
    return LARS_OK;
}

int run_image(const ImageJob &j)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_TRY(check_image(j.who, j.img, j.h, j.w, j.channels, j.dtype));
    if (j.mask & ~LARS_MASK_ALL) return fail(LARS_ERR_INVALID, "%s: unknown index bits in mask", j.who);
    const Route r = route_of(j);
    Layout L;
    LARS_TRY(ws_plan(c, [&](Carver &cv) { L = plan(j, r, cv); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(L.img, j.img, (size_t)j.h * j.w * j.channels * (j.dtype == LARS_U8 ? 1 : 2), hipMemcpyHostToDevice, s));
    LARS_TRY(r.planes == Route::MASKED ? run_masked(j, L, s) : r.planes == Route::STATS_MEDIANS ? run_stats_medians(j, L, s) : run_fused(j, r, L, s));
    LARS_TRY(send_pictures(j, L, s));
    FileAnswer files[3] = {{0, {0, 0}}, {0, {0, 0}}, {0, {0, 0}}};         // of the job's one kind of file
    LARS_TRY(encode_tiffs(j, L, s, files));
    LARS_TRY(collect(j, r, L, s, files));
    if (j.png_mode || j.tiff) LARS_TRY(fetch_files(j, j.tiff ? L.tif : L.png, j.tiff ? L.tif_bound : L.png_bound, files, s));
    return LARS_OK;
}

}  // namespace

extern "C" {

int lars_h_fix_white_balance(const void *img, int64_t h, int64_t w, int channels, int dtype, int variant, uint8_t *out,
                             double *percentiles)
{
    if (!out) return fail(LARS_ERR_INVALID, "lars_h_fix_white_balance: out == NULL");
    ImageJob j = picture_job("lars_h_fix_white_balance", img, h, w, channels, dtype, 1, 0, 0, out, nullptr, nullptr, nullptr, nullptr, nullptr);
    j.wb_variant = variant; j.pcts = percentiles;
    return run_image(j);
}

int lars_h_calculate_index(const void *img, int64_t h, int64_t w, int channels, int dtype, uint32_t index_mask,
                           float *const out[3], lars_stats *stats, int want_hist)
{
    if (!index_mask) return fail(LARS_ERR_INVALID, "lars_h_calculate_index: empty index mask");
    return run_image(picture_job("lars_h_calculate_index", img, h, w, channels, dtype, 0, index_mask, want_hist, nullptr, out, stats, nullptr, nullptr,
                                 nullptr));
}

int lars_h_process_image(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb,
                         uint32_t index_mask, int want_hist, uint8_t *out_wb, float *const out_index[3],
                         lars_stats *stats, float *medians, uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3])
{
    static const char *who = "lars_h_process_image";
    if (!index_mask && !(apply_wb && out_wb)) return fail(LARS_ERR_INVALID, "%s: nothing requested", who);
    return run_image(picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut));
}

int lars_h_process_image_png(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                             int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                             const uint8_t *const cmap_lut[3], int png_mode, uint8_t *const out_png[3], size_t png_cap,
                             int64_t png_len[3])
{
    static const char *who = "lars_h_process_image_png";
    if (png_mode != 1 && png_mode != 2) return fail(LARS_ERR_INVALID, "%s: png_mode must be 1 (RGBA) or 2 (P)", who);
    ImageJob j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, nullptr, cmap_lut);
    LARS_TRY(want_files(j, png_mode, 0, 0, out_png, png_cap, png_len));
    return run_image(j);
}

int lars_h_process_image_tiff_float32(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                      int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                      uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], int compression, int predictor,
                                      int64_t rows_per_strip, uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3])
{
    static const char *who = "lars_h_process_image_tiff_float32";
    if (compression != 5 && compression != 8) return fail(LARS_ERR_INVALID, "%s: compression must be 5 (LZW) or 8 (Deflate), got %d", who, compression);
    ImageJob j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut);
    LARS_TRY(want_files(j, compression, predictor, rows_per_strip, out_tiff, tiff_cap, tiff_len));
    return run_image(j);
}

int lars_h_process_image_tiff_f32(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                  int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                  uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], int predictor, int64_t rows_per_strip,
                                  uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3])
{
    ImageJob j = picture_job("lars_h_process_image_tiff_f32", img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats,
                             medians, out_rgba, cmap_lut);
    LARS_TRY(want_files(j, 5, predictor, rows_per_strip, out_tiff, tiff_cap, tiff_len));
    return run_image(j);
}

int lars_h_process_image_masked(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                int has_nodata, int nodata, int64_t *valid_pixels, int file_kind, int predictor, int64_t rows_per_strip,
                                uint8_t *const out_file[3], size_t file_cap, int64_t file_len[3])
{
    static const char *who = "lars_h_process_image_masked";
    if (valid_pixels) *valid_pixels = -1;
    LARS_TRY(check_picture(who, img, h, w, channels, dtype, index_mask, use_alpha, has_nodata, nodata, out_rgba, cmap_lut));
    if (index_mask & ~LARS_MASK_ALL) return fail(LARS_ERR_INVALID, "%s: unknown index bits in mask", who);
    if (!index_mask && !(apply_wb && out_wb)) return fail(LARS_ERR_INVALID, "%s: nothing requested", who);
    if (file_kind != 0 && file_kind != 1 && file_kind != 5 && file_kind != 8)
        return fail(LARS_ERR_INVALID, "%s: file_kind must be 0 (none), 1 (RGBA PNG), 5 (LZW TIFF) or 8 (Deflate TIFF), got %d", who, file_kind);
    // with a PNG the RGBA pictures stay on the device
    ImageJob j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians,
                             file_kind == 1 ? nullptr : out_rgba, cmap_lut);
    if (file_kind) LARS_TRY(want_files(j, file_kind, predictor, rows_per_strip, out_file, file_cap, file_len));
    under_mask(j, valid, use_alpha, has_nodata, nodata, valid_pixels);
    return run_image(j);
}

int lars_h_process_image_zones(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                               int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                               uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                               int has_nodata, int nodata, int64_t *valid_pixels, const void *zones, int zone_bytes, int64_t nzones,
                               lars_stats *zone_stats, float *zone_medians, int64_t *bad_labels)
{
    return lars_h_process_image_zones_margin(img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut,
                                             valid, use_alpha, has_nodata, nodata, valid_pixels, zones, zone_bytes, nzones, zone_stats, zone_medians, bad_labels,
                                             -1);
}

int lars_h_process_image_zones_margin(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                      int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                      uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                      int has_nodata, int nodata, int64_t *valid_pixels, const void *zones, int zone_bytes, int64_t nzones,
                                      lars_stats *zone_stats, float *zone_medians, int64_t *bad_labels, int64_t margin2)
{
    const char *who = margin2 == -1 ? "lars_h_process_image_zones" : "lars_h_process_image_zones_margin";
    const ZoneSource src = ZoneSource::raster(h, w, zones, zone_bytes, nzones).shrunk_by(margin2);
    ImageJob j;
    LARS_TRY(zones_job(&j, who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut, valid,
                       use_alpha, has_nodata, nodata, valid_pixels, src, {zone_stats, zone_medians, bad_labels}));
    LARS_TRY(check_zone_source(who, src, LARS_ZONES_MAX));
    return run_image(j);
}

int lars_h_process_image_zones_polygons(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                        int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                        uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                        int has_nodata, int nodata, int64_t *valid_pixels, const double *verts, int64_t nverts,
                                        const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts, int64_t npolys,
                                        lars_stats *zone_stats, float *zone_medians, void *labels_out, int label_bytes)
{
    return lars_h_process_image_zones_polygons_margin(img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba,
                                                      cmap_lut, valid, use_alpha, has_nodata, nodata, valid_pixels, verts, nverts, ring_starts, nrings, poly_starts,
                                                      npolys, zone_stats, zone_medians, labels_out, label_bytes, -1);
}

int lars_h_process_image_zones_polygons_margin(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                               int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                               uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                               int has_nodata, int nodata, int64_t *valid_pixels, const double *verts, int64_t nverts,
                                               const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts, int64_t npolys,
                                               lars_stats *zone_stats, float *zone_medians, void *labels_out, int label_bytes, int64_t margin2)
{
    const char *who = margin2 == -1 ? "lars_h_process_image_zones_polygons" : "lars_h_process_image_zones_polygons_margin";
    const ZoneSource src = ZoneSource::of(h, w, ZonePolys{verts, nverts, ring_starts, nrings, poly_starts, npolys, labels_out, label_bytes}).shrunk_by(margin2);
    ImageJob j;
    LARS_TRY(zones_job(&j, who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut, valid,
                       use_alpha, has_nodata, nodata, valid_pixels, src, {zone_stats, zone_medians, nullptr}));
    LARS_TRY(check_zone_source(who, src, LARS_ZONES_MAX));
    return run_image(j);
}

// process_image with regions as its zones: their outlines or a margin as well, never both
static int process_image_regions(const char *who, const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                 int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                 uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                 int has_nodata, int nodata, int64_t *valid_pixels, const uint8_t *mask, int source_index, int mode, float t,
                                 int connectivity, int64_t min_pixels, int64_t capacity, lars_stats *zone_stats, float *zone_medians,
                                 lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out,
                                 lars_outlines *outlines, int64_t margin2, int64_t *traced_vertices = nullptr, int64_t tq = 0)
{
    const ZoneSource src = ZoneSource::of(h, w, ZoneRegions{mask, mask ? 0 : source_index, mode, t, connectivity, min_pixels, capacity, table, n_regions,
                                                            labels_out, label_bytes, label_bytes_out, outlines, tq, traced_vertices}).shrunk_by(margin2);
    ImageJob j;
    LARS_TRY(zones_job(&j, who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut, valid,
                       use_alpha, has_nodata, nodata, valid_pixels, src, {zone_stats, zone_medians, nullptr}));
    if (!mask && (source_index < 0 || source_index > 2 || !((index_mask >> source_index) & 1u)))
        return fail(LARS_ERR_INVALID, "%s: source_index %d is not among the indices of index_mask", who, source_index);
    LARS_TRY(check_zone_source(who, src, LARS_ZONES_MAX));
    return run_image(j);
}

int lars_h_process_image_regions_outlines(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                          int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                          uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                          int has_nodata, int nodata, int64_t *valid_pixels, const uint8_t *mask, int source_index, int mode, float t,
                                          int connectivity, int64_t min_pixels, int64_t capacity, lars_stats *zone_stats, float *zone_medians,
                                          lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out,
                                          lars_outlines *outlines)
{
    return process_image_regions(outlines ? "lars_h_process_image_regions_outlines" : "lars_h_process_image_regions", img, h, w, channels, dtype, apply_wb,
                                 index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut, valid, use_alpha, has_nodata, nodata, valid_pixels,
                                 mask, source_index, mode, t, connectivity, min_pixels, capacity, zone_stats, zone_medians, table, n_regions, labels_out,
                                 label_bytes, label_bytes_out, outlines, -1);
}

int lars_h_process_image_regions_outlines_simplified(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                                     int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                                     uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                                     int has_nodata, int nodata, int64_t *valid_pixels, const uint8_t *mask, int source_index, int mode,
                                                     float t, int connectivity, int64_t min_pixels, int64_t capacity, lars_stats *zone_stats,
                                                     float *zone_medians, lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes,
                                                     int *label_bytes_out, lars_outlines *outlines, int64_t *traced_vertices, int64_t tq)
{
    if (!tq)
        return lars_h_process_image_regions_outlines(img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba,
                                                     cmap_lut, valid, use_alpha, has_nodata, nodata, valid_pixels, mask, source_index, mode, t, connectivity,
                                                     min_pixels, capacity, zone_stats, zone_medians, table, n_regions, labels_out, label_bytes, label_bytes_out,
                                                     outlines);
    static const char *who = "lars_h_process_image_regions_outlines_simplified";
    if (!outlines) return fail(LARS_ERR_INVALID, "%s: outlines == NULL", who);
    return process_image_regions(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut, valid,
                                 use_alpha, has_nodata, nodata, valid_pixels, mask, source_index, mode, t, connectivity, min_pixels, capacity, zone_stats,
                                 zone_medians, table, n_regions, labels_out, label_bytes, label_bytes_out, outlines, -1, traced_vertices, tq);
}

int lars_h_process_image_regions_margin(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                        int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                        uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                        int has_nodata, int nodata, int64_t *valid_pixels, const uint8_t *mask, int source_index, int mode, float t,
                                        int connectivity, int64_t min_pixels, int64_t capacity, lars_stats *zone_stats, float *zone_medians,
                                        lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out,
                                        int64_t margin2)
{
    return process_image_regions("lars_h_process_image_regions_margin", img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats,
                                 medians, out_rgba, cmap_lut, valid, use_alpha, has_nodata, nodata, valid_pixels, mask, source_index, mode, t, connectivity,
                                 min_pixels, capacity, zone_stats, zone_medians, table, n_regions, labels_out, label_bytes, label_bytes_out, nullptr, margin2);
}

int lars_h_process_image_regions(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                 int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                 uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                 int has_nodata, int nodata, int64_t *valid_pixels, const uint8_t *mask, int source_index, int mode, float t,
                                 int connectivity, int64_t min_pixels, int64_t capacity, lars_stats *zone_stats, float *zone_medians,
                                 lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out)
{
    return lars_h_process_image_regions_outlines(img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba,
                                                 cmap_lut, valid, use_alpha, has_nodata, nodata, valid_pixels, mask, source_index, mode, t, connectivity,
                                                 min_pixels, capacity, zone_stats, zone_medians, table, n_regions, labels_out, label_bytes, label_bytes_out,
                                                 nullptr);
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

}  // extern "C"
