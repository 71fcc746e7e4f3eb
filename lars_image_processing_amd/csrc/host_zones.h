// The zone half of the host entry points, as host_image.cpp sees it (host_zones.cpp): where a call's labels come from, the device
// buffers of a call with zones, and their run.
#pragma once
#include "common.h"

namespace lars {

// Polygons as the entry points take them (include/lars_hip.h "zones from polygons").
struct ZonePolys {
    const double *verts; int64_t nverts;
    const int32_t *ring_starts; int64_t nrings;
    const int32_t *poly_starts; int64_t npolys;
    void *labels_out; int label_bytes;     // host [h][w] labels back, or null
};

// Regions (include/lars_hip.h "zones from regions"): their number is known only once the labels exist, the buffers are sized by
// the capacity of the caller's arrays.
struct ZoneRegions {
    const uint8_t *mask;                   // host [h][w] foreground, or null: the plane `source` above (mode 1) or below (mode 2) t
    int source, mode;
    float t;
    int connectivity;
    int64_t min_pixels, capacity;
    lars_region *table_out;                // host [capacity]
    int64_t *n_regions;
    void *labels_out; int label_bytes; int *label_bytes_out;     // host [h][w] labels back, or null; label_bytes 0: the narrowest
    lars_outlines *outlines;               // the regions' rings and vertices back as well (outlines.hip), or null
    int64_t simplify_tq = 0;               // ... simplified on the device before they come down (outline_simplify.hip): sixteenths of a pixel, 0: as traced
    int64_t *traced_vertices = nullptr;    // ... and the count the tracer wrote, or null
};

// Where the labels of a call come from: exactly one of an uploaded raster, the rasteriser (zone_raster.hip) and the labeller
// (regions.hip).  With a margin (zone_margin.hip) the labels are shrunk on the device before anything reads them: the stages and
// every labels_out see the shrunk ones.
struct ZoneSource {
    enum Kind { RASTER, POLYGONS, REGIONS } kind;
    int64_t h, w;
    const void *labels; int label_bytes; int64_t nzones;         // RASTER: host [h][w] labels 0 .. nzones, label_bytes wide
    ZonePolys polys;                                              // POLYGONS
    ZoneRegions regions;                                          // REGIONS
    int64_t margin2 = -1;                                         // the squared margin 0 .. LARS_ZONE_MARGIN2_MAX, or -1: none
    void *raster_out = nullptr;                                   // RASTER: host [h][w] labels back at label_bytes, or null

    static ZoneSource raster(int64_t h, int64_t w, const void *labels, int label_bytes, int64_t nzones)
    {
        ZoneSource s = {RASTER, h, w, labels, label_bytes, nzones, {}, {}};
        return s;
    }
    static ZoneSource of(int64_t h, int64_t w, const ZonePolys &P)
    {
        ZoneSource s = {POLYGONS, h, w, nullptr, 0, 0, P, {}};
        return s;
    }
    static ZoneSource of(int64_t h, int64_t w, const ZoneRegions &G)
    {
        ZoneSource s = {REGIONS, h, w, nullptr, 0, 0, {}, G};
        return s;
    }
    ZoneSource shrunk_by(int64_t m2) const
    {
        ZoneSource s = *this;
        s.margin2 = m2;
        return s;
    }
    size_t npix() const { return (size_t)h * (size_t)w; }
    // the rows of the caller's per-zone arrays, which is also the stride of their three parts
    int64_t rows() const { return kind == RASTER ? nzones : kind == POLYGONS ? polys.npolys : regions.capacity; }
    // the width of the labels on the device: as given, or the int32 the device writes
    int zone_bytes() const { return kind == RASTER ? label_bytes : 4; }
    lars_outlines *outlines() const { return kind == REGIONS ? regions.outlines : nullptr; }
};

// The device buffers of a source: what makes the labels, and the labels.
struct ZoneLabelBufs {
    void *labels;                  // [npix] labels, zone_bytes() wide: what the zone stages read and what goes back to the caller
    void *raw;                     // ... as uploaded or made: the same buffer without a margin, the one the margin shrinks with it
    int32_t *made;                 // ... raw where the device wrote it, null for an uploaded raster
    uint8_t *margin_g;             // [npix] the column distances of the margin (zone_margin.hip), where there is one
    uint64_t *margin_counts;       // RASTER with a margin: [nzones + 2], the count of bad labels before they can be shrunk away
    void *narrow;                  // the labels at the width the caller wants them back in, where that is not 4
    double *verts;                 // POLYGONS
    int32_t *rings, *polys;
    void *raster_scratch;
    uint8_t *mask;                 // REGIONS: [npix] the foreground
    lars_region *table;            // [capacity]
    int64_t *count;                // R
    int64_t *outline_counts;       // [3] the tracer's counts, where the outlines are wanted
    void *label_scratch;
};

// The device buffers of the four stages (zonal.hip)
struct ZoneStatBufs {
    uint64_t *counts;              // [nzones + 1], then the count of bad labels
    uint64_t *ends, *cursors;      // [nzones + 1] each
    float *out[3];                 // the values of each index, zone by zone
    lars_stats *stats;             // [3][nzones]
    float *med;                    // [3][nzones][2]
    void *sel;                     // select scratch of the large zones
};

struct ZoneBufs { ZoneLabelBufs lab; ZoneStatBufs st; };

// What the stages read, on the device, and what they leave on the host
struct ZonePlanes {
    const float *plane[3];         // those of mask
    uint32_t mask;
    const uint8_t *valid;          // [npix] or null
    float thr[3];                  // the coverage thresholds
    int want_hist;
};
struct ZoneOutputs {
    lars_stats *stats;             // [3][rows()]
    float *medians;                // [3][rows()][2]
    int64_t *bad_labels;           // or null
};

// *bad_labels and the regions' *n_regions, where given, are -1 until the call knows better
void reset_zone_outputs(const ZoneSource &src, int64_t *bad_labels);
// What needs no device.  most_regions: the capacity the caller's use of the labels allows (LARS_ZONES_MAX where the stages follow)
int check_zone_records(const char *who, const ZoneSource &src, const void *stats, const void *medians);
int check_zone_source(const char *who, const ZoneSource &src, int64_t most_regions);
ZoneBufs plan_zones(Carver &c, const ZoneSource &src, uint32_t mask);
// The labels onto the device, the four stages, the records down (rows outside in.mask untouched) and the outlines where wanted.  The
// last copies are on the stream when this returns: the caller waits.
int run_zones(const char *who, const ZoneSource &src, const ZoneBufs &B, const ZonePlanes &in, const ZoneOutputs &out, hipStream_t s);

}  // namespace lars
