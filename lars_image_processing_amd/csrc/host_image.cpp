// The single-picture path of the host entry points: fix_white_balance, calculate_index, process_image and its PNG, TIFF,
// masked and zones variants, zonal_stats and valid_mask.  Every picture entry point fills an ImageJob (picture_job plus what is
// its own) and hands it to run_image, which decides the route once (route_of) and then runs a short sequence of stages:
// plan, upload, planes and statistics (one runner per route), pictures, TIFF, collect, fetch files.
#include <math.h>
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
    // labels made from polygons (zone_raster.hip): B.labels is then the int32 raster the rasteriser writes
    double *verts;
    int32_t *rings, *polys;
    char *raster_scratch;
    char *narrow;                  // the labels at the width the caller wants them back in, where that is not 4
    // labels made from regions (regions.hip): B.labels is the int32 raster the labelling writes, raster_scratch its scratch
    uint8_t *rmask;                // [npix] the foreground
    lars_region *rtable;           // [capacity]
    int64_t *rcount;               // R
    int64_t *ocounts;              // [3] the tracer's counts, where the regions' outlines are wanted (outlines.hip)
};

// The polygons of a job, as the entry points take them (include/lars_hip.h "zones from polygons"); nzones = npolys.
struct ZonePolys {
    const double *verts; int64_t nverts;
    const int32_t *ring_starts; int64_t nrings;
    const int32_t *poly_starts; int64_t npolys;
    void *labels_out; int label_bytes;     // host [h][w] labels back, or null
};

// The regions of a job (include/lars_hip.h "zones from regions"): nzones is known only once the labels exist, the buffers are sized
// by the capacity of the caller's record arrays.
struct ZoneRegions {
    const uint8_t *mask;                   // host [h][w] foreground, or null: the plane `source` above (mode 1) or below (mode 2) t
    int source, mode;
    float t;
    int connectivity;
    int64_t min_pixels, capacity;
    lars_region *table_out;                // host [capacity]
    int64_t *n_regions;
    void *labels_out; int label_bytes; int *label_bytes_out;     // host [h][w] labels back, or null; label_bytes 0: the narrowest
    int64_t h, w;
    lars_outlines *outlines;               // the regions' rings and vertices back as well (outlines.hip), or null
};

ZoneBufs zone_plan(Carver &c, size_t npix, int zone_bytes, int64_t nzones, uint32_t mask, const ZonePolys *P = nullptr,
                   const ZoneRegions *G = nullptr)
{
    ZoneBufs B;
    memset(&B, 0, sizeof B);
    const size_t nz = (size_t)nzones;
    if (P) {
        B.verts = c.take<double>(2 * (size_t)P->nverts);
        B.rings = c.take<int32_t>((size_t)P->nrings + 1);
        B.polys = c.take<int32_t>((size_t)P->npolys + 1);
        B.raster_scratch = c.take<char>(lars_zone_rasterize_scratch_bytes(P->npolys));
        B.narrow = (P->labels_out && P->label_bytes != 4) ? c.take<char>(npix * (size_t)P->label_bytes) : nullptr;
    }
    if (G) {
        B.rmask = c.take<uint8_t>(npix);
        B.rtable = c.take<lars_region>((size_t)G->capacity);
        B.rcount = c.take<int64_t>(1);
        B.ocounts = G->outlines ? c.take<int64_t>(3) : nullptr;
        B.raster_scratch = c.take<char>(lars_region_label_scratch_bytes(G->h, G->w));
        B.narrow = (G->labels_out && G->label_bytes != 4) ? c.take<char>(npix * 2) : nullptr;
    }
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

// Everything about the polygons that needs no device: the first ring or vertex that breaks a rule is named.
int check_polygons(const char *who, const ZonePolys &P, int64_t h, int64_t w)
{
    if (!P.verts || !P.ring_starts || !P.poly_starts) return fail(LARS_ERR_INVALID, "%s: verts, ring_starts and poly_starts are required", who);
    if (P.npolys < 1 || P.npolys > LARS_ZONES_MAX) return fail(LARS_ERR_INVALID, "%s: 1 to %d polygons, got %lld", who, LARS_ZONES_MAX, (long long)P.npolys);
    if (P.nrings < P.npolys || P.nverts < 3 * P.nrings || P.nverts > LARS_ZONE_VERTS_MAX)
        return fail(LARS_ERR_INVALID, "%s: %lld polygons need as many rings or more (got %lld) of three vertices or more each (got %lld in all, at most %d)",
                    who, (long long)P.npolys, (long long)P.nrings, (long long)P.nverts, LARS_ZONE_VERTS_MAX);
    if (h <= 0 || w <= 0 || h > (1 << 24) || w > (1 << 24)) return fail(LARS_ERR_INVALID, "%s: the raster is 1 to 2^24 on each side", who);
    if (P.labels_out && P.label_bytes != 1 && P.label_bytes != 2 && P.label_bytes != 4)
        return fail(LARS_ERR_INVALID, "%s: labels come back 1, 2 or 4 bytes wide, got %d", who, P.label_bytes);
    if (P.labels_out && ((P.label_bytes == 1 && P.npolys > 255) || !aligned_to(P.labels_out, (uintptr_t)P.label_bytes)))
        return fail(LARS_ERR_INVALID, "%s: %lld labels do not fit %d-byte labels, or the labels are not aligned", who, (long long)P.npolys, P.label_bytes);
    if (P.poly_starts[0] != 0 || P.poly_starts[P.npolys] != P.nrings || P.ring_starts[0] != 0 || P.ring_starts[P.nrings] != P.nverts)
        return fail(LARS_ERR_INVALID, "%s: poly_starts must run from 0 to nrings and ring_starts from 0 to nverts", who);
    for (int64_t k = 0; k < P.npolys; ++k)
        if (P.poly_starts[k + 1] <= P.poly_starts[k] || P.poly_starts[k + 1] > P.nrings)
            return fail(LARS_ERR_INVALID, "%s: polygon %lld has no ring (poly_starts must rise)", who, (long long)k);
    for (int64_t r = 0; r < P.nrings; ++r)
        if ((int64_t)P.ring_starts[r + 1] - P.ring_starts[r] < 3 || P.ring_starts[r + 1] > P.nverts)
            return fail(LARS_ERR_INVALID, "%s: ring %lld has fewer than three vertices (ring_starts must rise by three or more)", who, (long long)r);
    for (int64_t i = 0; i < 2 * P.nverts; ++i)
        if (!(fabs(P.verts[i]) <= 1e9))
            return fail(LARS_ERR_INVALID, "%s: vertex %lld has a coordinate that is not finite or beyond 1e9 in size", who, (long long)(i / 2));
    return LARS_OK;
}

// the polygons up, their labels into B.labels (int32) and, where the caller wants them, back at his width: on the stream
int raster_zones(const ZoneBufs &B, const ZonePolys &P, int64_t h, int64_t w, hipStream_t s)
{
    LARS_HIP_TRY(hipMemcpyAsync(B.verts, P.verts, 2 * (size_t)P.nverts * sizeof(double), hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(B.rings, P.ring_starts, ((size_t)P.nrings + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(B.polys, P.poly_starts, ((size_t)P.npolys + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    int32_t *labels = reinterpret_cast<int32_t *>(B.labels);
    LARS_TRY(lars_d_zone_rasterize(B.verts, P.nverts, B.rings, P.nrings, B.polys, P.npolys, h, w, labels, B.raster_scratch, s));
    if (!P.labels_out) return LARS_OK;
    const size_t npix = (size_t)h * (size_t)w;
    if (B.narrow) LARS_TRY(lars_d_zone_labels_narrow(labels, (int64_t)npix, P.label_bytes, B.narrow, s));
    LARS_HIP_TRY(hipMemcpyAsync(P.labels_out, B.narrow ? B.narrow : B.labels, npix * (size_t)P.label_bytes, hipMemcpyDeviceToHost, s));
    return LARS_OK;
}

// What the region entry points check before they touch the device.
int check_regions(const char *who, const ZoneRegions &G, int64_t most)
{
    if (G.h < 1 || G.w < 1 || !lars_region_label_scratch_bytes(G.h, G.w))
        return fail(LARS_ERR_INVALID, "%s: the raster is 1 or more on each side and has fewer than 2^31 pixels", who);
    if (!G.mask && G.mode != 1 && G.mode != 2) return fail(LARS_ERR_INVALID, "%s: a mask, or mode 1 (above t) or 2 (below t), is required", who);
    if (G.connectivity != 4 && G.connectivity != 8) return fail(LARS_ERR_INVALID, "%s: connectivity must be 4 or 8, got %d", who, G.connectivity);
    if (G.min_pixels < 1) return fail(LARS_ERR_INVALID, "%s: min_pixels must be 1 or more, got %lld", who, (long long)G.min_pixels);
    if (G.capacity < 1 || G.capacity > most || !G.table_out || !G.n_regions)
        return fail(LARS_ERR_INVALID, "%s: a table of capacity 1 to %lld and n_regions are required, got %lld", who, (long long)most, (long long)G.capacity);
    if (G.labels_out && G.label_bytes != 0 && G.label_bytes != 1 && G.label_bytes != 2 && G.label_bytes != 4)
        return fail(LARS_ERR_INVALID, "%s: labels come back 1, 2 or 4 bytes wide (0: the narrowest), got %d", who, G.label_bytes);
    if (G.labels_out && !aligned_to(G.labels_out, 4)) return fail(LARS_ERR_INVALID, "%s: the labels are not aligned", who);
    if (G.outlines) {
        lars_outlines &O = *G.outlines;
        O.n_rings = O.n_vertices = O.n_edges = -1;
        if (!lars_region_outline_scratch_bytes(G.h, G.w, 0))
            return fail(LARS_ERR_INVALID, "%s: outlines are traced on fewer than 2^29 pixels (an edge id fits int32), got %lld x %lld", who, (long long)G.h, (long long)G.w);
        if (O.ring_capacity < 0 || O.vert_capacity < 0 || (O.ring_capacity > 0 && !O.rings) || (O.vert_capacity > 0 && !O.verts) ||
            !aligned_to(O.rings, 8) || !aligned_to(O.verts, 4))
            return fail(LARS_ERR_INVALID, "%s: the outlines need a ring table and a vertex array of capacity >= 0, 8- and 4-byte aligned", who);
    }
    return LARS_OK;
}

// The outlines of the nregions labels in B.labels (int32), once everything else of the call is on the stream.  Three waits: for the
// edge count, which sizes the tracer's own area (the labels stand in the workspace, which cannot grow under them), for the ring and
// vertex counts, which may exceed the caller's room, and for the rows and vertices.
int trace_zone_outlines(const char *who, const ZoneBufs &B, const ZoneRegions &G, int64_t nregions, hipStream_t s)
{
    lars_outlines &O = *G.outlines;
    O.n_rings = O.n_vertices = O.n_edges = 0;
    if (!nregions) return LARS_OK;
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    const int32_t *labels = reinterpret_cast<const int32_t *>(B.labels);
    int64_t counts[3] = {-1, -1, -1};
    LARS_TRY(lars_d_region_outline_count(labels, G.h, G.w, B.ocounts, s));
    LARS_HIP_TRY(hipMemcpyAsync(counts, B.ocounts, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    const int64_t edges = counts[0];
    const size_t tracer = edges > 0 ? lars_region_outline_scratch_bytes(G.h, G.w, edges) : 0;
    if (!tracer) return fail(LARS_ERR_INVALID, "%s: %lld regions with %lld edges", who, (long long)nregions, (long long)edges);
    O.n_edges = edges;
    // no more rings than the tracer's own ring arrays hold, no more vertices than edges
    const int64_t rcap = O.ring_capacity < edges / 4 + 1 ? O.ring_capacity : edges / 4 + 1, vcap = O.vert_capacity < edges ? O.vert_capacity : edges;
    char *scratch;
    lars_outline_ring *rings;
    int32_t *verts;
    auto plan = [&](Carver &d) { scratch = d.take<char>(tracer), rings = d.take<lars_outline_ring>((size_t)rcap), verts = d.take<int32_t>(2 * (size_t)vcap); };
    Carver size(nullptr);
    plan(size);
    LARS_TRY(outline_reserve(c, size.bytes() + 256));
    Carver area(c->outline);
    plan(area);
    LARS_TRY(lars_d_region_outline(labels, G.h, G.w, G.connectivity, nregions, edges, rings, rcap, verts, vcap, B.ocounts, scratch, s));
    LARS_HIP_TRY(hipMemcpyAsync(counts, B.ocounts, sizeof counts, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    O.n_rings = counts[1];
    O.n_vertices = counts[2];
    if (counts[0] != edges || counts[1] < 1 || counts[2] < 4) return fail(LARS_ERR_HIP, "%s: the tracer counted %lld edges after %lld", who, (long long)counts[0], (long long)edges);
    if (counts[1] > O.ring_capacity || counts[2] > O.vert_capacity)
        return fail(LARS_ERR_INVALID, "%s: %lld rings and %lld vertices; the room is %lld and %lld", who, (long long)counts[1], (long long)counts[2],
                    (long long)O.ring_capacity, (long long)O.vert_capacity);
    LARS_HIP_TRY(hipMemcpyAsync(O.rings, rings, (size_t)counts[1] * sizeof(lars_outline_ring), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipMemcpyAsync(O.verts, verts, 2 * (size_t)counts[2] * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

// The foreground (uploaded, or the plane against t; never outside valid_dev), its labels into B.labels (int32) and R to the host: the one
// wait of this route.  R above the capacity ends the call; otherwise the table's R rows and, where wanted, the labels follow on the stream.
int label_zone_regions(const char *who, const ZoneBufs &B, const ZoneRegions &G, const float *plane, const uint8_t *valid_dev, int64_t *nzones,
                       hipStream_t s)
{
    const size_t npix = (size_t)G.h * (size_t)G.w;
    if (G.mask) LARS_HIP_TRY(hipMemcpyAsync(B.rmask, G.mask, npix, hipMemcpyHostToDevice, s));
    if (!G.mask || valid_dev)
        LARS_TRY(lars_d_region_mask_f32(G.mask ? nullptr : plane, G.mask ? B.rmask : nullptr, valid_dev, (int64_t)npix, G.t, G.mode == 2, B.rmask, s));
    int32_t *labels = reinterpret_cast<int32_t *>(B.labels);
    LARS_TRY(lars_d_region_label(B.rmask, G.h, G.w, G.connectivity, G.min_pixels, labels, B.rtable, G.capacity, B.rcount, B.raster_scratch, s));
    int64_t r = -1;
    LARS_HIP_TRY(hipMemcpyAsync(&r, B.rcount, sizeof r, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    *G.n_regions = r;
    int bytes = G.label_bytes ? G.label_bytes : r <= 255 ? 1 : r <= 65535 ? 2 : 4;
    if (r < 0 || r > G.capacity || (G.labels_out && ((bytes == 1 && r > 255) || (bytes == 2 && r > 65535))))
        return fail(LARS_ERR_INVALID, "%s: %lld regions; the capacity is %lld%s", who, (long long)r, (long long)G.capacity,
                    r <= G.capacity ? " and the labels are too narrow for them" : "");
    *nzones = r;
    if (r) LARS_HIP_TRY(hipMemcpyAsync(G.table_out, B.rtable, (size_t)r * sizeof(lars_region), hipMemcpyDeviceToHost, s));
    if (!G.labels_out) return LARS_OK;
    if (G.label_bytes_out) *G.label_bytes_out = bytes;
    if (bytes != 4) LARS_TRY(lars_d_zone_labels_narrow(labels, (int64_t)npix, bytes, B.narrow, s));
    LARS_HIP_TRY(hipMemcpyAsync(G.labels_out, bytes != 4 ? B.narrow : B.labels, npix * (size_t)bytes, hipMemcpyDeviceToHost, s));
    return LARS_OK;
}

// labels up (or made from the polygons P or the regions G, zone_bytes 4), the four stages, the records down (host_stats[3][nzones], host_med[3][nzones][2]; rows outside mask untouched).
// The counts cross to the host once: bad labels end the call there, and zones above the knob zone_split_pixels take the array
// kernels, which spread one zone over many workgroups.  The copies down are on the stream when this returns: the caller waits.
int run_zones(const char *who, const ZoneBufs &B, const void *zones, int zone_bytes, const uint8_t *valid_dev, int64_t npix, int64_t nzones,
              const float *const planes[3], uint32_t mask, const float thr[3], int want_hist, lars_stats *host_stats, float *host_med,
              int64_t *bad_labels, hipStream_t s, const ZonePolys *P = nullptr, int64_t h = 0, int64_t w = 0, const ZoneRegions *G = nullptr)
{
    // with regions nzones becomes R here and the host rows keep the stride of the caller's capacity; no region is a result, not an error
    const size_t host_stride = (size_t)(G ? G->capacity : nzones);
    if (G) {
        LARS_TRY(label_zone_regions(who, B, *G, planes[G->source], valid_dev, &nzones, s));
        if (!nzones) return G->outlines ? trace_zone_outlines(who, B, *G, 0, s) : LARS_OK;
    }
    const size_t nz = (size_t)nzones;
    if (P) LARS_TRY(raster_zones(B, *P, h, w, s));
    else if (!G) LARS_HIP_TRY(hipMemcpyAsync(B.labels, zones, (size_t)npix * zone_bytes, hipMemcpyHostToDevice, s));
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
        LARS_HIP_TRY(hipMemcpyAsync(host_stats + k * host_stride, st, nz * sizeof(lars_stats), hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipMemcpyAsync(host_med + 2 * k * host_stride, med, 2 * nz * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if (G && G->outlines) LARS_TRY(trace_zone_outlines(who, B, *G, nzones, s));
    return LARS_OK;
}

int zone_arguments(const char *who, const void *zones, int zone_bytes, int64_t nzones, const void *stats, const void *medians)
{
    if (!zones || !stats || !medians) return fail(LARS_ERR_INVALID, "%s: zones, their records and their medians are required", who);
    if (zone_bytes != 1 && zone_bytes != 2 && zone_bytes != 4) return fail(LARS_ERR_INVALID, "%s: labels are 1, 2 or 4 bytes wide, got %d", who, zone_bytes);
    if (nzones < 1 || nzones > LARS_ZONES_MAX) return fail(LARS_ERR_INVALID, "%s: 1 to %d zones, got %lld", who, LARS_ZONES_MAX, (long long)nzones);
    return LARS_OK;
}

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
    const void *zones;            // [h][w] labels 0 .. nzones, zone_bytes wide, or null
    int zone_bytes;
    int64_t nzones;
    lars_stats *zone_stats;       // [3][nzones]
    float *zone_medians;          // [3][nzones][2]
    int64_t *bad_labels;
    const ZonePolys *polys;       // ... or the plots' outlines instead of zones: the labels are made on the device (zone_raster.hip)
    const ZoneRegions *regions;   // ... or the connected regions of a mask or of a thresholded plane (regions.hip); nzones = their capacity
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
        const bool for_zones = j.zones != nullptr || j.polys != nullptr || j.regions != nullptr;   // the zone stages scatter it
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
    if (j.zones || j.polys || j.regions) L.zone = zone_plan(c, npix, j.zone_bytes, j.nzones, j.mask, j.polys, j.regions);
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
    if (!j.zones && !j.polys && !j.regions) return LARS_OK;
    const float thr[3] = {0.2f, 0.2f, 0.0f};                // as the records above
    return run_zones(j.who, L.zone, j.zones, j.zone_bytes, L.vmask, npix, j.nzones, L.idx, j.mask, thr, j.want_hist, j.zone_stats,
                     j.zone_medians, j.bad_labels, s, j.polys, j.h, j.w, j.regions);
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
    static const char *who = "lars_h_process_image_zones";
    if (valid_pixels) *valid_pixels = -1;
    if (bad_labels) *bad_labels = -1;
    LARS_TRY(check_picture(who, img, h, w, channels, dtype, index_mask, use_alpha, has_nodata, nodata, out_rgba, cmap_lut));
    if (!index_mask || (index_mask & ~LARS_MASK_ALL)) return fail(LARS_ERR_INVALID, "%s: index_mask must name one to three indices", who);
    LARS_TRY(zone_arguments(who, zones, zone_bytes, nzones, zone_stats, zone_medians));
    ImageJob j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut);
    // the masked route even when no mask is given: the results are the same by definition
    under_mask(j, valid, use_alpha, has_nodata, nodata, valid_pixels);
    j.zones = zones; j.zone_bytes = zone_bytes; j.nzones = nzones; j.zone_stats = zone_stats; j.zone_medians = zone_medians;
    j.bad_labels = bad_labels;
    return run_image(j);
}

int lars_h_process_image_zones_polygons(const void *img, int64_t h, int64_t w, int channels, int dtype, int apply_wb, uint32_t index_mask,
                                        int want_hist, uint8_t *out_wb, float *const out_index[3], lars_stats *stats, float *medians,
                                        uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3], const uint8_t *valid, int use_alpha,
                                        int has_nodata, int nodata, int64_t *valid_pixels, const double *verts, int64_t nverts,
                                        const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts, int64_t npolys,
                                        lars_stats *zone_stats, float *zone_medians, void *labels_out, int label_bytes)
{
    static const char *who = "lars_h_process_image_zones_polygons";
    if (valid_pixels) *valid_pixels = -1;
    LARS_TRY(check_picture(who, img, h, w, channels, dtype, index_mask, use_alpha, has_nodata, nodata, out_rgba, cmap_lut));
    if (!index_mask || (index_mask & ~LARS_MASK_ALL)) return fail(LARS_ERR_INVALID, "%s: index_mask must name one to three indices", who);
    if (!zone_stats || !zone_medians) return fail(LARS_ERR_INVALID, "%s: the zones' records and medians are required", who);
    const ZonePolys P = {verts, nverts, ring_starts, nrings, poly_starts, npolys, labels_out, label_bytes};
    LARS_TRY(check_polygons(who, P, h, w));
    ImageJob j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut);
    under_mask(j, valid, use_alpha, has_nodata, nodata, valid_pixels);
    j.polys = &P; j.zone_bytes = 4; j.nzones = npolys; j.zone_stats = zone_stats; j.zone_medians = zone_medians;
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
    const char *who = outlines ? "lars_h_process_image_regions_outlines" : "lars_h_process_image_regions";
    if (valid_pixels) *valid_pixels = -1;
    if (n_regions) *n_regions = -1;
    LARS_TRY(check_picture(who, img, h, w, channels, dtype, index_mask, use_alpha, has_nodata, nodata, out_rgba, cmap_lut));
    if (!index_mask || (index_mask & ~LARS_MASK_ALL)) return fail(LARS_ERR_INVALID, "%s: index_mask must name one to three indices", who);
    if (!zone_stats || !zone_medians) return fail(LARS_ERR_INVALID, "%s: the zones' records and medians are required", who);
    if (!mask && (source_index < 0 || source_index > 2 || !((index_mask >> source_index) & 1u)))
        return fail(LARS_ERR_INVALID, "%s: source_index %d is not among the indices of index_mask", who, source_index);
    const ZoneRegions G = {mask, mask ? 0 : source_index, mode, t, connectivity, min_pixels, capacity, table, n_regions, labels_out, label_bytes,
                           label_bytes_out, h, w, outlines};
    LARS_TRY(check_regions(who, G, LARS_ZONES_MAX));
    ImageJob j = picture_job(who, img, h, w, channels, dtype, apply_wb, index_mask, want_hist, out_wb, out_index, stats, medians, out_rgba, cmap_lut);
    under_mask(j, valid, use_alpha, has_nodata, nodata, valid_pixels);
    j.regions = &G; j.zone_bytes = 4; j.nzones = capacity; j.zone_stats = zone_stats; j.zone_medians = zone_medians;
    return run_image(j);
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

}  // extern "C"

namespace {

// zonal_statistics of a host plane, with the labels uploaded (zones) or rasterised (P)
int zonal_stats(const char *who, const float *x, const void *zones, int zone_bytes, const ZonePolys *P, const uint8_t *valid, int64_t h, int64_t w,
                int64_t nzones, float threshold, int want_hist, lars_stats *stats, float *medians, int64_t *bad_labels, const ZoneRegions *G = nullptr)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || h <= 0 || w <= 0) return fail(LARS_ERR_INVALID, "%s: x must be a non-empty [h][w] float32 array", who);
    if (P || G) {
        if (!stats || !medians) return fail(LARS_ERR_INVALID, "%s: the zones' records and medians are required", who);
        LARS_TRY(P ? check_polygons(who, *P, h, w) : check_regions(who, *G, LARS_ZONES_MAX));
    } else {
        LARS_TRY(zone_arguments(who, zones, zone_bytes, nzones, stats, medians));
    }
    const size_t npix = (size_t)h * w;
    float *dx;
    uint8_t *dvalid;
    ZoneBufs B;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        dx = d.take<float>(npix);
        dvalid = valid ? d.take<uint8_t>(npix) : nullptr;
        B = zone_plan(d, npix, zone_bytes, nzones, 1u, P, G);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, npix * sizeof(float), hipMemcpyHostToDevice, s));
    if (valid) LARS_HIP_TRY(hipMemcpyAsync(dvalid, valid, npix, hipMemcpyHostToDevice, s));
    const float *planes[3] = {dx, nullptr, nullptr};
    const float thr[3] = {threshold, threshold, threshold};
    LARS_TRY(run_zones(who, B, zones, zone_bytes, dvalid, (int64_t)npix, nzones, planes, 1u, thr, want_hist, stats, medians, bad_labels, s, P, h, w, G));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

}  // namespace

extern "C" {

int lars_h_zonal_stats_f32(const float *x, const void *zones, int zone_bytes, const uint8_t *valid, int64_t h, int64_t w, int64_t nzones,
                           float threshold, int want_hist, lars_stats *stats, float *medians, int64_t *bad_labels)
{
    if (bad_labels) *bad_labels = -1;
    return zonal_stats("lars_h_zonal_stats_f32", x, zones, zone_bytes, nullptr, valid, h, w, nzones, threshold, want_hist, stats, medians, bad_labels);
}

int lars_h_zonal_stats_polygons_f32(const float *x, const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                    const int32_t *poly_starts, int64_t npolys, const uint8_t *valid, int64_t h, int64_t w, float threshold,
                                    int want_hist, lars_stats *stats, float *medians, void *labels_out, int label_bytes)
{
    const ZonePolys P = {verts, nverts, ring_starts, nrings, poly_starts, npolys, labels_out, label_bytes};
    return zonal_stats("lars_h_zonal_stats_polygons_f32", x, nullptr, 4, &P, valid, h, w, npolys, threshold, want_hist, stats, medians, nullptr);
}

int lars_h_zonal_stats_regions_outlines_f32(const float *x, const uint8_t *mask, int mode, float t, int connectivity, int64_t min_pixels,
                                            const uint8_t *valid, int64_t h, int64_t w, float threshold, int want_hist, int64_t capacity,
                                            lars_stats *stats, float *medians, lars_region *table, int64_t *n_regions, void *labels_out,
                                            int label_bytes, int *label_bytes_out, lars_outlines *outlines)
{
    if (n_regions) *n_regions = -1;
    const ZoneRegions G = {mask, 0, mode, t, connectivity, min_pixels, capacity, table, n_regions, labels_out, label_bytes, label_bytes_out, h, w, outlines};
    return zonal_stats(outlines ? "lars_h_zonal_stats_regions_outlines_f32" : "lars_h_zonal_stats_regions_f32", x, nullptr, 4, nullptr, valid, h, w, capacity,
                       threshold, want_hist, stats, medians, nullptr, &G);
}

int lars_h_zonal_stats_regions_f32(const float *x, const uint8_t *mask, int mode, float t, int connectivity, int64_t min_pixels,
                                   const uint8_t *valid, int64_t h, int64_t w, float threshold, int want_hist, int64_t capacity, lars_stats *stats,
                                   float *medians, lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out)
{
    return lars_h_zonal_stats_regions_outlines_f32(x, mask, mode, t, connectivity, min_pixels, valid, h, w, threshold, want_hist, capacity, stats, medians, table,
                                                   n_regions, labels_out, label_bytes, label_bytes_out, nullptr);
}

// label_regions, and region_outlines where outlines are wanted: the labels stay in the workspace for the tracer
static int label_regions_call(const char *who, const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                              int *label_bytes_out, lars_region *table, int64_t capacity, int64_t *n_regions, lars_outlines *outlines)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (n_regions) *n_regions = -1;
    if (!mask || !labels) return fail(LARS_ERR_INVALID, "%s: mask and labels are required", who);
    const ZoneRegions G = {mask, 0, 0, 0.0f, connectivity, min_pixels, capacity, table, n_regions, labels, label_bytes, label_bytes_out, h, w, outlines};
    LARS_TRY(check_regions(who, G, 0x7FFFFFFF));
    ZoneBufs B;
    memset(&B, 0, sizeof B);
    const size_t npix = (size_t)h * (size_t)w;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        B.labels = d.take<char>(npix * 4);
        B.rmask = d.take<uint8_t>(npix);
        B.rtable = d.take<lars_region>((size_t)capacity);
        B.rcount = d.take<int64_t>(1);
        B.ocounts = outlines ? d.take<int64_t>(3) : nullptr;
        B.raster_scratch = d.take<char>(lars_region_label_scratch_bytes(h, w));
        B.narrow = label_bytes != 4 ? d.take<char>(npix * 2) : nullptr;
    }));
    int64_t r = 0;
    LARS_TRY(label_zone_regions(who, B, G, nullptr, nullptr, &r, c->stream));
    if (outlines) LARS_TRY(trace_zone_outlines(who, B, G, r, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    return LARS_OK;
}

int lars_h_label_regions(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                         int *label_bytes_out, lars_region *table, int64_t capacity, int64_t *n_regions)
{
    return label_regions_call("lars_h_label_regions", mask, h, w, connectivity, min_pixels, label_bytes, labels, label_bytes_out, table, capacity, n_regions,
                              nullptr);
}

int lars_h_region_outlines(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                           int *label_bytes_out, lars_region *table, int64_t capacity, int64_t *n_regions, lars_outlines *outlines)
{
    static const char *who = "lars_h_region_outlines";
    if (!outlines) return fail(LARS_ERR_INVALID, "%s: outlines == NULL", who);
    return label_regions_call(who, mask, h, w, connectivity, min_pixels, label_bytes, labels, label_bytes_out, table, capacity, n_regions, outlines);
}

int lars_h_rasterize_zones(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                           int64_t npolys, int64_t h, int64_t w, int zone_bytes, void *labels)
{
    static const char *who = "lars_h_rasterize_zones";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!labels) return fail(LARS_ERR_INVALID, "%s: labels == NULL", who);
    const ZonePolys P = {verts, nverts, ring_starts, nrings, poly_starts, npolys, labels, zone_bytes};
    LARS_TRY(check_polygons(who, P, h, w));
    ZoneBufs B;
    LARS_TRY(ws_plan(c, [&](Carver &d) { B = zone_plan(d, (size_t)h * (size_t)w, 4, npolys, 0u, &P); }));
    LARS_TRY(raster_zones(B, P, h, w, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
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

}  // extern "C"
