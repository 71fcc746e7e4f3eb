// The zone path of the host entry points: zonal statistics of a plane from a label raster, from polygons or from regions,
// label_regions, region_outlines and rasterize_zones; process_image_zones and its kin (host_image.cpp) come through host_zones.h.
// Every call states where its labels come from in one ZoneSource, which is checked once (check_zone_source), sizes the device
// buffers once (plan_zone_labels, plus plan_zone_stats where statistics follow) and is turned into labels on the device by one step
// (zone_labels), which also shrinks them where the source has a margin (zone_margin.hip).  run_zones is that step, the four stages of
// zonal.hip and, where wanted, the outline trace.
#include <math.h>
#include <string.h>
#include <vector>

#include "host_zones.h"

namespace lars {

namespace {

// ---- what needs no device ----
int check_raster(const char *who, const ZoneSource &src)
{
    if (!src.labels) return fail(LARS_ERR_INVALID, "%s: zones, their records and their medians are required", who);
    if (src.label_bytes != 1 && src.label_bytes != 2 && src.label_bytes != 4)
        return fail(LARS_ERR_INVALID, "%s: labels are 1, 2 or 4 bytes wide, got %d", who, src.label_bytes);
    if (src.nzones < 1 || src.nzones > LARS_ZONES_MAX) return fail(LARS_ERR_INVALID, "%s: 1 to %d zones, got %lld", who, LARS_ZONES_MAX, (long long)src.nzones);
    return LARS_OK;
}

// the first ring or vertex that breaks a rule is named
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

int check_regions(const char *who, const ZoneRegions &G, int64_t h, int64_t w, int64_t most)
{
    if (h < 1 || w < 1 || !lars_region_label_scratch_bytes(h, w))
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
        if (G.traced_vertices) *G.traced_vertices = -1;
        if (G.simplify_tq < 0 || G.simplify_tq > LARS_SIMPLIFY_TQ_MAX)
            return fail(LARS_ERR_INVALID, "%s: tq must be 0 to %d sixteenths of a pixel, got %lld", who, LARS_SIMPLIFY_TQ_MAX, (long long)G.simplify_tq);
        if (G.simplify_tq && (h > LARS_SIMPLIFY_SIDE_MAX || w > LARS_SIMPLIFY_SIDE_MAX))
            return fail(LARS_ERR_INVALID, "%s: outlines are simplified on a raster of at most %d a side (every product of coordinates fits 64 bits), got %lld x %lld",
                        who, LARS_SIMPLIFY_SIDE_MAX, (long long)h, (long long)w);
        if (!lars_region_outline_scratch_bytes(h, w, 0))
            return fail(LARS_ERR_INVALID, "%s: outlines are traced on fewer than 2^29 pixels (an edge id fits int32), got %lld x %lld", who, (long long)h, (long long)w);
        if (O.ring_capacity < 0 || O.vert_capacity < 0 || (O.ring_capacity > 0 && !O.rings) || (O.vert_capacity > 0 && !O.verts) ||
            !aligned_to(O.rings, 8) || !aligned_to(O.verts, 4))
            return fail(LARS_ERR_INVALID, "%s: the outlines need a ring table and a vertex array of capacity >= 0, 8- and 4-byte aligned", who);
    }
    return LARS_OK;
}

// ---- the device buffers ----
// Of the source alone: every call that makes or takes labels carves these, whether statistics follow or not.
ZoneLabelBufs plan_zone_labels(Carver &c, const ZoneSource &src)
{
    ZoneLabelBufs B;
    memset(&B, 0, sizeof B);
    const size_t npix = src.npix();
    if (src.kind == ZoneSource::POLYGONS) {
        const ZonePolys &P = src.polys;
        B.verts = c.take<double>(2 * (size_t)P.nverts);
        B.rings = c.take<int32_t>((size_t)P.nrings + 1);
        B.polys = c.take<int32_t>((size_t)P.npolys + 1);
        B.raster_scratch = c.take<char>(lars_zone_rasterize_scratch_bytes(P.npolys));
        if (P.labels_out && P.label_bytes != 4) B.narrow = c.take<char>(npix * (size_t)P.label_bytes);
    }
    if (src.kind == ZoneSource::REGIONS) {
        const ZoneRegions &G = src.regions;
        B.mask = c.take<uint8_t>(npix);
        B.table = c.take<lars_region>((size_t)G.capacity);
        B.count = c.take<int64_t>(1);
        if (G.outlines) B.outline_counts = c.take<int64_t>(3);
        B.label_scratch = c.take<char>(lars_region_label_scratch_bytes(src.h, src.w));
        if (G.labels_out && G.label_bytes != 4) B.narrow = c.take<char>(npix * 2);     // the narrowest is known once R is: 2 bytes at most
    }
    if (src.kind == ZoneSource::RASTER) B.labels = B.raw = c.take<char>(npix * (size_t)src.label_bytes);
    else B.labels = B.raw = B.made = c.take<int32_t>(npix);
    if (src.margin2 >= 0) {
        B.margin_g = c.take<uint8_t>(npix);
        B.labels = c.take<char>(npix * (size_t)src.zone_bytes());     // shrinking in place would race with the neighbours' reads
        if (src.kind == ZoneSource::RASTER) B.margin_counts = c.take<uint64_t>((size_t)src.nzones + 2);
    }
    return B;
}

ZoneStatBufs plan_zone_stats(Carver &c, size_t npix, int64_t rows, uint32_t mask)
{
    ZoneStatBufs B;
    const size_t nz = (size_t)rows;
    B.counts = c.take<uint64_t>(nz + 2);
    B.ends = c.take<uint64_t>(nz + 1);
    B.cursors = c.take<uint64_t>(nz + 1);
    for (int k = 0; k < 3; ++k) B.out[k] = ((mask >> k) & 1u) ? c.take<float>(npix) : nullptr;
    B.stats = c.take<lars_stats>(3 * nz);
    B.med = c.take<float>(6 * nz);
    B.sel = c.take<char>(lars_select_scratch_bytes());
    return B;
}

// ---- the labels onto the device ----
// the polygons up and their labels made: on the stream
int raster_zones(const ZoneSource &src, const ZoneLabelBufs &B, hipStream_t s)
{
    const ZonePolys &P = src.polys;
    LARS_HIP_TRY(hipMemcpyAsync(B.verts, P.verts, 2 * (size_t)P.nverts * sizeof(double), hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(B.rings, P.ring_starts, ((size_t)P.nrings + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(B.polys, P.poly_starts, ((size_t)P.npolys + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return lars_d_zone_rasterize(B.verts, P.nverts, B.rings, P.nrings, B.polys, P.npolys, src.h, src.w, B.made, B.raster_scratch, s);
}

// The foreground (uploaded, or the plane against t; never outside valid_dev), its labels and R to the host: the one wait of this step.
// R above the capacity ends the call; otherwise the table's R rows follow on the stream.  *bytes: the width the labels go back in.
int label_zone_regions(const char *who, const ZoneSource &src, const ZoneLabelBufs &B, const float *plane, const uint8_t *valid_dev, int64_t *nzones,
                       int *bytes, hipStream_t s)
{
    const ZoneRegions &G = src.regions;
    const size_t npix = src.npix();
    if (G.mask) LARS_HIP_TRY(hipMemcpyAsync(B.mask, G.mask, npix, hipMemcpyHostToDevice, s));
    if (!G.mask || valid_dev)
        LARS_TRY(lars_d_region_mask_f32(G.mask ? nullptr : plane, G.mask ? B.mask : nullptr, valid_dev, (int64_t)npix, G.t, G.mode == 2, B.mask, s));
    LARS_TRY(lars_d_region_label(B.mask, src.h, src.w, G.connectivity, G.min_pixels, B.made, B.table, G.capacity, B.count, B.label_scratch, s));
    int64_t r = -1;
    LARS_HIP_TRY(hipMemcpyAsync(&r, B.count, sizeof r, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    *G.n_regions = r;
    *bytes = G.label_bytes ? G.label_bytes : r <= 255 ? 1 : r <= 65535 ? 2 : 4;
    if (r < 0 || r > G.capacity || (G.labels_out && ((*bytes == 1 && r > 255) || (*bytes == 2 && r > 65535))))
        return fail(LARS_ERR_INVALID, "%s: %lld regions; the capacity is %lld%s", who, (long long)r, (long long)G.capacity,
                    r <= G.capacity ? " and the labels are too narrow for them" : "");
    *nzones = r;
    if (r) LARS_HIP_TRY(hipMemcpyAsync(G.table_out, B.table, (size_t)r * sizeof(lars_region), hipMemcpyDeviceToHost, s));
    if (G.labels_out && G.label_bytes_out) *G.label_bytes_out = *bytes;
    return LARS_OK;
}

// The margin (zone_margin.hip): B.raw shrunk into B.labels.  Labels above nzones can only come with an uploaded raster; they are
// counted where they still stand and end the call as the stages would, which see none afterwards.
int shrink_zone_labels(const char *who, const ZoneSource &src, const ZoneLabelBufs &B, int64_t *bad_labels, hipStream_t s)
{
    if (src.kind == ZoneSource::RASTER) {
        const size_t nz = (size_t)src.nzones;
        uint64_t bad = 0;
        LARS_TRY(lars_d_zone_count(B.raw, src.label_bytes, nullptr, (int64_t)src.npix(), src.nzones, B.margin_counts, B.margin_counts + nz + 1, s));
        LARS_HIP_TRY(hipMemcpyAsync(&bad, B.margin_counts + nz + 1, sizeof bad, hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipStreamSynchronize(s));
        if (bad_labels) *bad_labels = (int64_t)bad;
        if (bad) return fail(LARS_ERR_INVALID, "%s: %llu labels outside 0 .. %lld", who, (unsigned long long)bad, (long long)src.nzones);
    }
    return lars_d_zone_shrink(B.raw, src.zone_bytes(), src.h, src.w, src.margin2, B.margin_g, B.labels, s);
}

// Uploaded, rasterised or labelled, and shrunk where the source has a margin: afterwards the labels stand in B.labels, src.zone_bytes()
// wide, and *nzones says how many zones they name; where the caller wants them they are on their way back at his width.  With
// regions that is R, which may be 0: no region is a result, not an error.  planes: what a threshold is compared with.
int zone_labels(const char *who, const ZoneSource &src, const ZoneLabelBufs &B, const float *const planes[3], const uint8_t *valid_dev, int64_t *nzones,
                int64_t *bad_labels, hipStream_t s)
{
    *nzones = src.rows();
    void *back = src.raster_out;
    int bytes = src.label_bytes;
    if (src.kind == ZoneSource::REGIONS) {
        LARS_TRY(label_zone_regions(who, src, B, planes ? planes[src.regions.source] : nullptr, valid_dev, nzones, &bytes, s));
        back = src.regions.labels_out;
    } else if (src.kind == ZoneSource::POLYGONS) {
        LARS_TRY(raster_zones(src, B, s));
        back = src.polys.labels_out, bytes = src.polys.label_bytes;
    } else {
        LARS_HIP_TRY(hipMemcpyAsync(B.raw, src.labels, src.npix() * (size_t)src.label_bytes, hipMemcpyHostToDevice, s));
    }
    if (src.margin2 >= 0) LARS_TRY(shrink_zone_labels(who, src, B, bad_labels, s));
    if (!back) return LARS_OK;
    const bool narrow = bytes != src.zone_bytes();
    if (narrow) LARS_TRY(lars_d_zone_labels_narrow(static_cast<const int32_t *>(B.labels), (int64_t)src.npix(), bytes, B.narrow, s));
    LARS_HIP_TRY(hipMemcpyAsync(back, narrow ? B.narrow : B.labels, src.npix() * (size_t)bytes, hipMemcpyDeviceToHost, s));
    return LARS_OK;
}

// ---- the four stages (zonal.hip) over nzones zones, the records down at the stride of the caller's rows ----
// The counts cross to the host once: bad labels end the call there, and zones above the knob zone_split_pixels take the array
// kernels, which spread one zone over many workgroups.
int zone_stages(const char *who, const ZoneSource &src, const ZoneBufs &B, const ZonePlanes &in, const ZoneOutputs &out, int64_t nzones, hipStream_t s)
{
    const ZoneStatBufs &T = B.st;
    const void *labels = B.lab.labels;
    const int zone_bytes = src.zone_bytes();
    const int64_t npix = (int64_t)src.npix();
    const size_t nz = (size_t)nzones, host_stride = (size_t)src.rows();
    LARS_TRY(lars_d_zone_count(labels, zone_bytes, in.valid, npix, nzones, T.counts, T.counts + nz + 1, s));
    std::vector<uint64_t> counts(nz + 2);
    LARS_HIP_TRY(hipMemcpyAsync(counts.data(), T.counts, (nz + 2) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (out.bad_labels) *out.bad_labels = (int64_t)counts[nz + 1];
    if (counts[nz + 1])
        return fail(LARS_ERR_INVALID, "%s: %llu labels outside 0 .. %lld", who, (unsigned long long)counts[nz + 1], (long long)nzones);
    LARS_TRY(lars_d_zone_offsets(T.counts, nzones, T.ends, T.cursors, s));
    LARS_TRY(lars_d_zone_scatter(in.plane, in.mask, labels, zone_bytes, in.valid, npix, nzones, T.ends, T.cursors, T.out, s));
    const int64_t split = tuning().zone_split_pixels;
    for (int k = 0; k < 3; ++k) {
        if (!((in.mask >> k) & 1u)) continue;
        lars_stats *st = T.stats + k * nz;
        float *med = T.med + 2 * k * nz;
        LARS_TRY(lars_d_zone_stats(T.out[k], T.ends, T.counts, nzones, in.thr[k], in.want_hist, split, st, med, s));
        uint64_t lo = 0;
        for (size_t z = 1; z <= nz; lo += counts[z], ++z) {
            if (counts[z] <= (uint64_t)split) continue;
            LARS_TRY(lars_d_array_stats_f32(T.out[k] + lo, (int64_t)counts[z], in.thr[k], in.want_hist, st + (z - 1), s));
            LARS_TRY(lars_d_median_pair_f32(T.out[k] + lo, (int64_t)counts[z], med + 2 * (z - 1), T.sel, s));
        }
        LARS_HIP_TRY(hipMemcpyAsync(out.stats + k * host_stride, st, nz * sizeof(lars_stats), hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipMemcpyAsync(out.medians + 2 * k * host_stride, med, 2 * nz * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    return LARS_OK;
}

// The outlines of the nregions labels in B.made, once everything else of the call is on the stream; no region: no ring.  Three waits:
// for the edge count, which sizes the tracer's own area (the labels stand in the workspace, which cannot grow under them), for the ring
// and vertex counts, which may exceed the caller's room, and for the rows and vertices.  With a tolerance the rings are simplified
// between the trace and the download (outline_simplify.hip, which waits once per batch of rounds): the traced vertices stay on the
// device, in room for as many as there are edges, and only the vertices written have to fit the caller's room and come down.
int trace_zone_outlines(const char *who, const ZoneSource &src, const ZoneLabelBufs &B, int64_t nregions, hipStream_t s)
{
    lars_outlines &O = *src.regions.outlines;
    const int64_t h = src.h, w = src.w, tq = src.regions.simplify_tq;
    O.n_rings = O.n_vertices = O.n_edges = 0;
    if (src.regions.traced_vertices) *src.regions.traced_vertices = 0;
    if (!nregions) return LARS_OK;
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    int64_t counts[3] = {-1, -1, -1};
    LARS_TRY(lars_d_region_outline_count(B.made, h, w, B.outline_counts, s));
    LARS_HIP_TRY(hipMemcpyAsync(counts, B.outline_counts, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    const int64_t edges = counts[0];
    const size_t tracer = edges > 0 ? lars_region_outline_scratch_bytes(h, w, edges) : 0;
    if (!tracer) return fail(LARS_ERR_INVALID, "%s: %lld regions with %lld edges", who, (long long)nregions, (long long)edges);
    O.n_edges = edges;
    // no more rings than the tracer's own ring arrays hold, no more vertices than edges; with a tolerance all of them stay on the device
    const int64_t rcap = tq || O.ring_capacity > edges / 4 + 1 ? edges / 4 + 1 : O.ring_capacity;
    const int64_t vcap = tq || O.vert_capacity > edges ? edges : O.vert_capacity, vcap_out = O.vert_capacity < edges ? O.vert_capacity : edges;
    const size_t simplifier = tq ? lars_outline_simplify_scratch_bytes(rcap, vcap) : 0;
    if (tq && !simplifier) return fail(LARS_ERR_INVALID, "%s: %lld rings and %lld vertices are more than can be simplified", who, (long long)rcap, (long long)vcap);
    char *scratch;
    lars_outline_ring *rings, *rings_out = nullptr;
    int32_t *verts, *verts_out = nullptr;
    int64_t *counts_out = nullptr;
    auto plan = [&](Carver &d) {
        scratch = d.take<char>(tracer > simplifier ? tracer : simplifier);       // the simplifier starts when the tracer is done with it
        rings = d.take<lars_outline_ring>((size_t)rcap), verts = d.take<int32_t>(2 * (size_t)vcap);
        if (tq) rings_out = d.take<lars_outline_ring>((size_t)rcap), verts_out = d.take<int32_t>(2 * (size_t)vcap_out), counts_out = d.take<int64_t>(3);
    };
    Carver size(nullptr);
    plan(size);
    LARS_TRY(outline_reserve(c, size.bytes() + 256));
    Carver area(c->outline);
    plan(area);
    LARS_TRY(lars_d_region_outline(B.made, h, w, src.regions.connectivity, nregions, edges, rings, rcap, verts, vcap, B.outline_counts, scratch, s));
    LARS_HIP_TRY(hipMemcpyAsync(counts, B.outline_counts, sizeof counts, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    O.n_rings = counts[1];
    O.n_vertices = counts[2];
    if (src.regions.traced_vertices) *src.regions.traced_vertices = counts[2];
    if (counts[0] != edges || counts[1] < 1 || counts[2] < 4) return fail(LARS_ERR_HIP, "%s: the tracer counted %lld edges after %lld", who, (long long)counts[0], (long long)edges);
    if (!tq && (counts[1] > O.ring_capacity || counts[2] > O.vert_capacity))
        return fail(LARS_ERR_INVALID, "%s: %lld rings and %lld vertices; the room is %lld and %lld", who, (long long)counts[1], (long long)counts[2],
                    (long long)O.ring_capacity, (long long)O.vert_capacity);
    if (tq) {
        if (counts[1] > rcap || counts[2] > vcap)
            return fail(LARS_ERR_HIP, "%s: the tracer wrote %lld rings and %lld vertices for %lld edges", who, (long long)counts[1], (long long)counts[2], (long long)edges);
        int64_t written[3] = {-1, -1, -1};
        LARS_TRY(lars_d_outline_simplify(rings, rcap, verts, vcap, B.outline_counts, tq, h, w, rings_out, verts_out, vcap_out, counts_out, scratch, nullptr, s));
        LARS_HIP_TRY(hipMemcpyAsync(written, counts_out, sizeof written, hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipStreamSynchronize(s));
        if (written[0] != counts[1] || written[1] < 3 || written[1] > counts[2])
            return fail(LARS_ERR_HIP, "%s: %lld rings and %lld vertices simplified after %lld and %lld traced", who, (long long)written[0], (long long)written[1],
                        (long long)counts[1], (long long)counts[2]);
        O.n_vertices = counts[2] = written[1];
        if (counts[1] > O.ring_capacity || written[1] > O.vert_capacity)
            return fail(LARS_ERR_INVALID, "%s: %lld rings and %lld vertices; the room is %lld and %lld", who, (long long)counts[1], (long long)written[1],
                        (long long)O.ring_capacity, (long long)O.vert_capacity);
        rings = rings_out, verts = verts_out;
    }
    LARS_HIP_TRY(hipMemcpyAsync(O.rings, rings, (size_t)counts[1] * sizeof(lars_outline_ring), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipMemcpyAsync(O.verts, verts, 2 * (size_t)counts[2] * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

// Rings and vertices that came down earlier, simplified (simplify_outlines): up, lars_d_outline_simplify, down.
int simplify_host_outlines(const char *who, const lars_outline_ring *rings, int64_t n_rings, const int32_t *verts, int64_t n_vertices, int64_t tq, int64_t h,
                           int64_t w, lars_outline_ring *rings_out, int32_t *verts_out, int64_t vert_capacity_out, int64_t *counts_out, int64_t *rounds_out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!counts_out) return fail(LARS_ERR_INVALID, "%s: counts_out == NULL", who);
    counts_out[0] = counts_out[1] = counts_out[2] = -1;
    if (n_rings < 0 || n_vertices < 0 || vert_capacity_out < 0 || (n_rings > 0 && (!rings || !rings_out)) || (n_vertices > 0 && !verts) ||
        (vert_capacity_out > 0 && !verts_out) || !lars_outline_simplify_scratch_bytes(n_rings, n_vertices))
        return fail(LARS_ERR_INVALID, "%s: ring tables of 0 to 2^31 - 1 rows and vertex arrays of as many vertices are required", who);
    const int64_t vcap_out = vert_capacity_out < n_vertices ? vert_capacity_out : n_vertices;
    lars_outline_ring *d_rings, *d_rings_out;
    int32_t *d_verts, *d_verts_out;
    int64_t *d_counts;
    char *scratch;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        d_rings = d.take<lars_outline_ring>((size_t)n_rings), d_rings_out = d.take<lars_outline_ring>((size_t)n_rings);
        d_verts = d.take<int32_t>(2 * (size_t)n_vertices), d_verts_out = d.take<int32_t>(2 * (size_t)vcap_out);
        d_counts = d.take<int64_t>(6);
        scratch = d.take<char>(lars_outline_simplify_scratch_bytes(n_rings, n_vertices));
    }));
    hipStream_t s = c->stream;
    const int64_t given[3] = {0, n_rings, n_vertices};
    int64_t written[3] = {-1, -1, -1};
    LARS_HIP_TRY(hipMemcpyAsync(d_counts, given, sizeof given, hipMemcpyHostToDevice, s));
    if (n_rings) LARS_HIP_TRY(hipMemcpyAsync(d_rings, rings, (size_t)n_rings * sizeof(lars_outline_ring), hipMemcpyHostToDevice, s));
    if (n_vertices) LARS_HIP_TRY(hipMemcpyAsync(d_verts, verts, 2 * (size_t)n_vertices * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_outline_simplify(d_rings, n_rings, d_verts, n_vertices, d_counts, tq, h, w, d_rings_out, d_verts_out, vcap_out, d_counts + 3, scratch, rounds_out, s));
    LARS_HIP_TRY(hipMemcpyAsync(written, d_counts + 3, sizeof written, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    memcpy(counts_out, written, sizeof written);
    if (written[0] != n_rings || written[1] < 0 || written[1] > n_vertices)
        return fail(LARS_ERR_HIP, "%s: %lld rings and %lld vertices written for %lld and %lld given", who, (long long)written[0], (long long)written[1],
                    (long long)n_rings, (long long)n_vertices);
    if (written[1] > vert_capacity_out)
        return fail(LARS_ERR_INVALID, "%s: %lld vertices; the room is %lld", who, (long long)written[1], (long long)vert_capacity_out);
    if (n_rings) LARS_HIP_TRY(hipMemcpyAsync(rings_out, d_rings_out, (size_t)n_rings * sizeof(lars_outline_ring), hipMemcpyDeviceToHost, s));
    if (written[1]) LARS_HIP_TRY(hipMemcpyAsync(verts_out, d_verts_out, 2 * (size_t)written[1] * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

// zonal_statistics of a host plane
int zonal_stats(const char *who, const float *x, const ZoneSource &src, const uint8_t *valid, float threshold, int want_hist, const ZoneOutputs &out)
{
    reset_zone_outputs(src, out.bad_labels);
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || src.h <= 0 || src.w <= 0) return fail(LARS_ERR_INVALID, "%s: x must be a non-empty [h][w] float32 array", who);
    LARS_TRY(check_zone_records(who, src, out.stats, out.medians));
    LARS_TRY(check_zone_source(who, src, LARS_ZONES_MAX));
    const size_t npix = src.npix();
    float *dx;
    uint8_t *dvalid;
    ZoneBufs B;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        dx = d.take<float>(npix);
        dvalid = valid ? d.take<uint8_t>(npix) : nullptr;
        B = plan_zones(d, src, 1u);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, npix * sizeof(float), hipMemcpyHostToDevice, s));
    if (valid) LARS_HIP_TRY(hipMemcpyAsync(dvalid, valid, npix, hipMemcpyHostToDevice, s));
    const ZonePlanes in = {{dx, nullptr, nullptr}, 1u, dvalid, {threshold, threshold, threshold}, want_hist};
    LARS_TRY(run_zones(who, src, B, in, out, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

// The calls that want the labels and no statistics: the labels step, the outlines where the source asks for them, the wait.
int labels_only(const char *who, const ZoneSource &src, ThreadCtx *c, int64_t *bad_labels = nullptr)
{
    ZoneLabelBufs B;
    LARS_TRY(ws_plan(c, [&](Carver &d) { B = plan_zone_labels(d, src); }));
    int64_t nzones = 0;
    LARS_TRY(zone_labels(who, src, B, nullptr, nullptr, &nzones, bad_labels, c->stream));
    if (src.outlines()) LARS_TRY(trace_zone_outlines(who, src, B, nzones, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    return LARS_OK;
}

// label_regions, and region_outlines where outlines are given: the labels stay in the workspace for the tracer
int label_regions_call(const char *who, const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                       int *label_bytes_out, lars_region *table, int64_t capacity, int64_t *n_regions, lars_outlines *outlines,
                       int64_t *traced_vertices = nullptr, int64_t tq = 0)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    const ZoneSource src = ZoneSource::of(h, w, ZoneRegions{mask, 0, 0, 0.0f, connectivity, min_pixels, capacity, table, n_regions, labels, label_bytes,
                                                            label_bytes_out, outlines, tq, traced_vertices});
    reset_zone_outputs(src, nullptr);
    if (!mask || !labels) return fail(LARS_ERR_INVALID, "%s: mask and labels are required", who);
    LARS_TRY(check_zone_source(who, src, 0x7FFFFFFF));
    return labels_only(who, src, c);
}

}  // namespace

void reset_zone_outputs(const ZoneSource &src, int64_t *bad_labels)
{
    if (bad_labels) *bad_labels = -1;
    if (src.kind == ZoneSource::REGIONS && src.regions.n_regions) *src.regions.n_regions = -1;
}

int check_zone_records(const char *who, const ZoneSource &src, const void *stats, const void *medians)
{
    if (stats && medians) return LARS_OK;
    return src.kind == ZoneSource::RASTER ? fail(LARS_ERR_INVALID, "%s: zones, their records and their medians are required", who)
                                          : fail(LARS_ERR_INVALID, "%s: the zones' records and medians are required", who);
}

int check_zone_source(const char *who, const ZoneSource &src, int64_t most_regions)
{
    if (src.margin2 < -1 || src.margin2 > LARS_ZONE_MARGIN2_MAX)
        return fail(LARS_ERR_INVALID, "%s: margin2 must be 0 to %d, or -1 for no margin, got %lld", who, LARS_ZONE_MARGIN2_MAX, (long long)src.margin2);
    if (src.margin2 >= 0 && src.outlines())
        return fail(LARS_ERR_INVALID, "%s: outlines are traced from regions that are connected; a margin may break them apart", who);
    return src.kind == ZoneSource::RASTER     ? check_raster(who, src)
           : src.kind == ZoneSource::POLYGONS ? check_polygons(who, src.polys, src.h, src.w)
                                              : check_regions(who, src.regions, src.h, src.w, most_regions);
}

ZoneBufs plan_zones(Carver &c, const ZoneSource &src, uint32_t mask)
{
    ZoneBufs B;
    B.lab = plan_zone_labels(c, src);
    B.st = plan_zone_stats(c, src.npix(), src.rows(), mask);
    return B;
}

int run_zones(const char *who, const ZoneSource &src, const ZoneBufs &B, const ZonePlanes &in, const ZoneOutputs &out, hipStream_t s)
{
    int64_t nzones = 0;
    LARS_TRY(zone_labels(who, src, B.lab, in.plane, in.valid, &nzones, out.bad_labels, s));
    if (nzones) LARS_TRY(zone_stages(who, src, B, in, out, nzones, s));
    if (src.outlines()) LARS_TRY(trace_zone_outlines(who, src, B.lab, nzones, s));
    return LARS_OK;
}

}  // namespace lars

using namespace lars;

extern "C" {

int lars_h_zonal_stats_margin_f32(const float *x, const void *zones, int zone_bytes, const uint8_t *valid, int64_t h, int64_t w, int64_t nzones,
                                  float threshold, int want_hist, lars_stats *stats, float *medians, int64_t *bad_labels, int64_t margin2)
{
    return zonal_stats(margin2 == -1 ? "lars_h_zonal_stats_f32" : "lars_h_zonal_stats_margin_f32", x,
                       ZoneSource::raster(h, w, zones, zone_bytes, nzones).shrunk_by(margin2), valid, threshold, want_hist, {stats, medians, bad_labels});
}

int lars_h_zonal_stats_f32(const float *x, const void *zones, int zone_bytes, const uint8_t *valid, int64_t h, int64_t w, int64_t nzones,
                           float threshold, int want_hist, lars_stats *stats, float *medians, int64_t *bad_labels)
{
    return lars_h_zonal_stats_margin_f32(x, zones, zone_bytes, valid, h, w, nzones, threshold, want_hist, stats, medians, bad_labels, -1);
}

int lars_h_zonal_stats_polygons_margin_f32(const float *x, const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                           const int32_t *poly_starts, int64_t npolys, const uint8_t *valid, int64_t h, int64_t w, float threshold,
                                           int want_hist, lars_stats *stats, float *medians, void *labels_out, int label_bytes, int64_t margin2)
{
    const ZonePolys P = {verts, nverts, ring_starts, nrings, poly_starts, npolys, labels_out, label_bytes};
    return zonal_stats(margin2 == -1 ? "lars_h_zonal_stats_polygons_f32" : "lars_h_zonal_stats_polygons_margin_f32", x, ZoneSource::of(h, w, P).shrunk_by(margin2),
                       valid, threshold, want_hist, {stats, medians, nullptr});
}

int lars_h_zonal_stats_polygons_f32(const float *x, const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                    const int32_t *poly_starts, int64_t npolys, const uint8_t *valid, int64_t h, int64_t w, float threshold,
                                    int want_hist, lars_stats *stats, float *medians, void *labels_out, int label_bytes)
{
    return lars_h_zonal_stats_polygons_margin_f32(x, verts, nverts, ring_starts, nrings, poly_starts, npolys, valid, h, w, threshold, want_hist, stats, medians,
                                                  labels_out, label_bytes, -1);
}

int lars_h_zonal_stats_regions_outlines_simplified_f32(const float *x, const uint8_t *mask, int mode, float t, int connectivity, int64_t min_pixels,
                                                       const uint8_t *valid, int64_t h, int64_t w, float threshold, int want_hist, int64_t capacity,
                                                       lars_stats *stats, float *medians, lars_region *table, int64_t *n_regions, void *labels_out,
                                                       int label_bytes, int *label_bytes_out, lars_outlines *outlines, int64_t *traced_vertices, int64_t tq)
{
    const char *who = tq        ? "lars_h_zonal_stats_regions_outlines_simplified_f32"
                      : outlines ? "lars_h_zonal_stats_regions_outlines_f32"
                                 : "lars_h_zonal_stats_regions_f32";
    if (tq && !outlines) return fail(LARS_ERR_INVALID, "%s: outlines == NULL", who);
    const ZoneRegions G = {mask, 0, mode, t, connectivity, min_pixels, capacity, table, n_regions, labels_out, label_bytes, label_bytes_out, outlines, tq,
                           traced_vertices};
    return zonal_stats(who, x, ZoneSource::of(h, w, G), valid, threshold, want_hist, {stats, medians, nullptr});
}

int lars_h_zonal_stats_regions_outlines_f32(const float *x, const uint8_t *mask, int mode, float t, int connectivity, int64_t min_pixels,
                                            const uint8_t *valid, int64_t h, int64_t w, float threshold, int want_hist, int64_t capacity,
                                            lars_stats *stats, float *medians, lars_region *table, int64_t *n_regions, void *labels_out,
                                            int label_bytes, int *label_bytes_out, lars_outlines *outlines)
{
    return lars_h_zonal_stats_regions_outlines_simplified_f32(x, mask, mode, t, connectivity, min_pixels, valid, h, w, threshold, want_hist, capacity, stats,
                                                              medians, table, n_regions, labels_out, label_bytes, label_bytes_out, outlines, nullptr, 0);
}

int lars_h_zonal_stats_regions_margin_f32(const float *x, const uint8_t *mask, int mode, float t, int connectivity, int64_t min_pixels,
                                          const uint8_t *valid, int64_t h, int64_t w, float threshold, int want_hist, int64_t capacity, lars_stats *stats,
                                          float *medians, lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out,
                                          int64_t margin2)
{
    const ZoneRegions G = {mask, 0, mode, t, connectivity, min_pixels, capacity, table, n_regions, labels_out, label_bytes, label_bytes_out, nullptr};
    return zonal_stats("lars_h_zonal_stats_regions_margin_f32", x, ZoneSource::of(h, w, G).shrunk_by(margin2), valid, threshold, want_hist,
                       {stats, medians, nullptr});
}

int lars_h_zonal_stats_regions_f32(const float *x, const uint8_t *mask, int mode, float t, int connectivity, int64_t min_pixels,
                                   const uint8_t *valid, int64_t h, int64_t w, float threshold, int want_hist, int64_t capacity, lars_stats *stats,
                                   float *medians, lars_region *table, int64_t *n_regions, void *labels_out, int label_bytes, int *label_bytes_out)
{
    return lars_h_zonal_stats_regions_outlines_f32(x, mask, mode, t, connectivity, min_pixels, valid, h, w, threshold, want_hist, capacity, stats, medians, table,
                                                   n_regions, labels_out, label_bytes, label_bytes_out, nullptr);
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

int lars_h_region_outlines_simplified(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                                      int *label_bytes_out, lars_region *table, int64_t capacity, int64_t *n_regions, lars_outlines *outlines,
                                      int64_t *traced_vertices, int64_t tq)
{
    const char *who = tq ? "lars_h_region_outlines_simplified" : "lars_h_region_outlines";
    if (!outlines) return fail(LARS_ERR_INVALID, "%s: outlines == NULL", who);
    return label_regions_call(who, mask, h, w, connectivity, min_pixels, label_bytes, labels, label_bytes_out, table, capacity, n_regions, outlines,
                              traced_vertices, tq);
}

int lars_h_outline_simplify(const lars_outline_ring *rings, int64_t n_rings, const int32_t *verts, int64_t n_vertices, int64_t tq, int64_t h, int64_t w,
                            lars_outline_ring *rings_out, int32_t *verts_out, int64_t vert_capacity_out, int64_t *counts_out, int64_t *rounds_out)
{
    return simplify_host_outlines("lars_h_outline_simplify", rings, n_rings, verts, n_vertices, tq, h, w, rings_out, verts_out, vert_capacity_out, counts_out,
                                  rounds_out);
}

int lars_h_rasterize_zones_margin(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                                  int64_t npolys, int64_t h, int64_t w, int zone_bytes, void *labels, int64_t margin2)
{
    const char *who = margin2 == -1 ? "lars_h_rasterize_zones" : "lars_h_rasterize_zones_margin";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!labels) return fail(LARS_ERR_INVALID, "%s: labels == NULL", who);
    const ZoneSource src = ZoneSource::of(h, w, ZonePolys{verts, nverts, ring_starts, nrings, poly_starts, npolys, labels, zone_bytes}).shrunk_by(margin2);
    LARS_TRY(check_zone_source(who, src, LARS_ZONES_MAX));
    return labels_only(who, src, c);
}

int lars_h_rasterize_zones(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                           int64_t npolys, int64_t h, int64_t w, int zone_bytes, void *labels)
{
    return lars_h_rasterize_zones_margin(verts, nverts, ring_starts, nrings, poly_starts, npolys, h, w, zone_bytes, labels, -1);
}

int lars_h_shrink_zones(const void *zones, int zone_bytes, int64_t h, int64_t w, int64_t nzones, int64_t margin2, void *out, int64_t *bad_labels)
{
    static const char *who = "lars_h_shrink_zones";
    if (bad_labels) *bad_labels = -1;
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!zones || !out || h <= 0 || w <= 0) return fail(LARS_ERR_INVALID, "%s: zones and out must be non-empty [h][w] label rasters", who);
    if (margin2 < 0) return fail(LARS_ERR_INVALID, "%s: margin2 must be 0 to %d, got %lld", who, LARS_ZONE_MARGIN2_MAX, (long long)margin2);
    ZoneSource src = ZoneSource::raster(h, w, zones, zone_bytes, nzones).shrunk_by(margin2);
    src.raster_out = out;
    LARS_TRY(check_zone_source(who, src, LARS_ZONES_MAX));
    if (!aligned_to(zones, (uintptr_t)zone_bytes) || !aligned_to(out, (uintptr_t)zone_bytes)) return fail(LARS_ERR_INVALID, "%s: the labels are not aligned", who);
    return labels_only(who, src, c, bad_labels);
}

}  // extern "C"
