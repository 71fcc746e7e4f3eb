// Zones from polygons (DESIGN.md "Zones from polygons"): the label raster zonal.hip reads, made on the device from plot outlines
// (analyze_index per plot, process-images.py:492-513, for callers who hold outlines and no raster).
//
// The definition.  Coordinates are pixel units, pixel (row i, column j) has the centre (j + 0.5, i + 0.5).  A polygon is the pool of
// the edges of its rings (rings close implicitly; a zero-length edge counts for nothing).  An edge with y0 == y1 crosses no row;
// otherwise (xa, ya) is its end with the smaller y, (xb, yb) the other, it crosses row i iff ya <= cy < yb and its crossing is
//     xc = xa + ((cy - ya) * (xb - xa)) / (yb - ya)        float64, every operation rounded once, in this order.
// Pixel (i, j) is inside iff the number of crossings of row i with xc <= cx is odd.  Polygon k labels its pixels k + 1, the largest
// label wins, a pixel in no polygon is 0.
//
// Three kernels and a narrowing copy:
//   k_zr_bounds  one workgroup per polygon: the rows and the 32-column words its crossings can touch, and how many jobs that makes
//   k_zr_starts  jobs[p] -> the first job of polygon p (one workgroup, wg_scan_array)
//   k_zr_fill    one workgroup per job = (polygon, band of ZR_ROWS rows, tile of ZR_WORDS words): the threads stride over the
//                polygon's edges; an edge's crossing with a row of the band becomes the first column whose centre is not left of it,
//                clipped to the tile -- a column left of the tile flips the tile's first bit (the parity it carries in), one right of
//                it is dropped -- and flips that bit of the row's bitmap in LDS.  A prefix XOR along the row turns crossings into
//                inside bits, and the lanes raise the labels of the inside pixels with atomicMax.
//   k_zr_narrow  int32 labels -> uint8 / uint16 for callers who want the raster on the host
//
// Nothing depends on which wave arrives first: XOR and max commute.  The work is rows x edges + covered pixels, without a sort and
// without a cap on the crossings of a row.  The vertices are read once per job, straight from memory (a polygon's vertices are a
// few cache lines, or a stream every thread takes a 256th of), so nothing is staged.
//
// Every index read from the ring arrays is clamped to the vertex array, every row and column to the raster: arrays that do not
// describe polygons give wrong labels, never an access outside the buffers.
#include "common.h"
#include "device_common.h"
#include "wg_device.h"

namespace lars {

namespace {

#define ZR_ROWS 8                       // rows of a job: the edges are read once per band
#define ZR_WORDS 256                    // 32-column words of a job's tile: 8192 columns, 8 KiB of LDS for the band
#define ZR_THREADS 256
#define ZR_EDGES 4                      // edges a thread loads before it works on them

struct ZrBox { int r0, r1, w0, w1; };   // rows r0 .. r1 - 1, words w0 .. w1 - 1 (empty when r1 <= r0 or w1 <= w0)

__device__ inline int zr_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// a double -> an int in lo .. hi; NaN gives lo
__device__ inline int zr_to_int(double v, int lo, int hi)
{
    if (!(v > (double)lo)) return lo;
    if (v >= (double)hi) return hi;
    return (int)v;
}

// ===========================================================================
// 1. per polygon: the rows and words of its crossings (one row / one column of margin: the box only bounds the work)
// ===========================================================================
__global__ __launch_bounds__(256) void k_zr_bounds(const double *__restrict__ verts, int nverts, const int *__restrict__ ring_starts, int nrings,
                                                   const int *__restrict__ poly_starts, int npolys, int h, int w, ZrBox *__restrict__ boxes,
                                                   unsigned long long *__restrict__ jobs)
{
    __shared__ double s_box[4][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p = blockIdx.x;                                                    // < npolys: the grid is the polygons
    const int v0 = zr_clampi(ring_starts[zr_clampi(poly_starts[p], 0, nrings)], 0, nverts);
    const int v1 = zr_clampi(ring_starts[zr_clampi(poly_starts[p + 1], 0, nrings)], 0, nverts);
    double xmin = __builtin_inf(), xmax = -__builtin_inf(), ymin = __builtin_inf(), ymax = -__builtin_inf();
    const double2 *vert2 = reinterpret_cast<const double2 *>(verts);             // 16-byte aligned: the entry point checks it
    for (int v = v0 + (int)threadIdx.x; v < v1; v += 256) {
        const double2 q = vert2[v];
        xmin = fmin(xmin, q.x); xmax = fmax(xmax, q.x);
        ymin = fmin(ymin, q.y); ymax = fmax(ymax, q.y);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        xmin = fmin(xmin, __shfl_xor(xmin, off)); xmax = fmax(xmax, __shfl_xor(xmax, off));
        ymin = fmin(ymin, __shfl_xor(ymin, off)); ymax = fmax(ymax, __shfl_xor(ymax, off));
    }
    if (lane == 0) { s_box[wv][0] = xmin; s_box[wv][1] = xmax; s_box[wv][2] = ymin; s_box[wv][3] = ymax; }
    __syncthreads();
    if (threadIdx.x) return;
    for (int k = 1; k < 4; ++k) {
        xmin = fmin(xmin, s_box[k][0]); xmax = fmax(xmax, s_box[k][1]);
        ymin = fmin(ymin, s_box[k][2]); ymax = fmax(ymax, s_box[k][3]);
    }
    // rows with ymin <= i + 0.5 < ymax lie in floor(ymin) - 1 .. floor(ymax) + 1; the crossings' columns in floor(xmin) - 1 .. floor(xmax) + 2
    // (a crossing lies between its edge's ends up to a few roundings of at most 2e9: far less than a column)
    ZrBox b;
    b.r0 = zr_to_int(floor(ymin) - 1.0, 0, h);
    b.r1 = zr_to_int(floor(ymax) + 2.0, 0, h);
    const int c0 = zr_to_int(floor(xmin) - 1.0, 0, w), c1 = zr_to_int(floor(xmax) + 3.0, 0, w);
    b.w0 = c0 >> 5;
    b.w1 = (c1 + 31) >> 5;
    if (!(ymin < ymax) || v1 - v0 < 3) b.r1 = b.r0;                             // no edge crosses a row
    boxes[p] = b;
    const unsigned long long bands = b.r1 > b.r0 ? (unsigned long long)((b.r1 - b.r0 + ZR_ROWS - 1) / ZR_ROWS) : 0ull;
    const unsigned long long tiles = b.w1 > b.w0 ? (unsigned long long)((b.w1 - b.w0 + ZR_WORDS - 1) / ZR_WORDS) : 0ull;
    jobs[p] = bands * tiles;
}

// ===========================================================================
// 2. jobs[p] -> the number of jobs before polygon p; jobs[npolys] = all of them
// ===========================================================================
__global__ __launch_bounds__(1024) void k_zr_starts(unsigned long long *__restrict__ jobs, int npolys)
{
    const unsigned long long total = wg_scan_array<unsigned long long>(
        (long long)npolys, [&](long long i) { return jobs[i]; }, [&](long long i, unsigned long long before) { jobs[i] = before; });
    if (threadIdx.x == 0) jobs[npolys] = total;
}

// ===========================================================================
// 3. the labels of one job
// ===========================================================================
__global__ __launch_bounds__(ZR_THREADS) void k_zr_fill(const double *__restrict__ verts, int nverts, const int *__restrict__ ring_starts, int nrings,
                                                        const int *__restrict__ poly_starts, int npolys, const ZrBox *__restrict__ boxes,
                                                        const unsigned long long *__restrict__ starts, int h, int w, int *__restrict__ labels)
{
    __shared__ unsigned int s_bits[ZR_ROWS][ZR_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long total = starts[npolys];
    for (unsigned long long job = blockIdx.x; job < total; job += gridDim.x) {   // block-uniform: every thread meets every barrier
        int lo = 0, hi = npolys - 1;                                             // the last polygon whose first job is <= job
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (starts[mid] <= job) lo = mid; else hi = mid - 1;
        }
        const int p = lo;
        const ZrBox b = boxes[p];
        const unsigned long long local = job - starts[p];
        const unsigned long long tiles = (unsigned long long)((b.w1 - b.w0 + ZR_WORDS - 1) / ZR_WORDS);
        if (b.r1 <= b.r0 || b.w1 <= b.w0) continue;                              // never: such a polygon has no job
        const int row0 = b.r0 + (int)(local / tiles) * ZR_ROWS;
        const int word0 = b.w0 + (int)(local % tiles) * ZR_WORDS;
        const int nrows = min(ZR_ROWS, b.r1 - row0), nwords = min(ZR_WORDS, b.w1 - word0);
        const int col0 = word0 * 32, col1 = min(col0 + nwords * 32, w);          // the tile's columns col0 .. col1 - 1
        if (nrows <= 0 || nwords <= 0 || row0 < 0 || row0 + nrows > h || col0 < 0 || col1 <= col0) continue;   // never, with boxes of k_zr_bounds
        for (int i = tid; i < nrows * ZR_WORDS; i += ZR_THREADS)
            if ((i & (ZR_WORDS - 1)) < nwords) s_bits[i / ZR_WORDS][i & (ZR_WORDS - 1)] = 0u;
        __syncthreads();

        // the crossings
        const int ring_lo = zr_clampi(poly_starts[p], 0, nrings), ring_hi = zr_clampi(poly_starts[p + 1], 0, nrings);
        const int v0 = zr_clampi(ring_starts[ring_lo], 0, nverts), v1 = zr_clampi(ring_starts[ring_hi], 0, nverts);
        const double first = (double)col0 + 0.5, last = (double)(col1 - 1) + 0.5;
        const double2 *vert2 = reinterpret_cast<const double2 *>(verts);
        const double cy_first = (double)row0 + 0.5, cy_last = (double)(row0 + nrows - 1) + 0.5;
        for (int vb = v0 + tid; vb < v1; vb += ZR_EDGES * ZR_THREADS) {
            // the loads of ZR_EDGES edges first, so that they are in flight together: a polygon of thousands of vertices is a chain of
            // loads otherwise (a trace showed 78 dependent steps per thread on 20 000 vertices)
            double2 e0[ZR_EDGES], e1[ZR_EDGES];
#pragma unroll
            for (int u = 0; u < ZR_EDGES; ++u) {
                const int v = vb + u * ZR_THREADS;
                e0[u] = e1[u] = make_double2(0.0, 0.0);                          // y0 == y1: crosses no row
                if (v >= v1) continue;
                int r = ring_lo, rh = ring_hi - 1;                               // the ring of vertex v: the last one that starts at or before it
                while (r < rh) {
                    const int mid = (r + rh + 1) >> 1;
                    if (ring_starts[mid] <= v) r = mid; else rh = mid - 1;
                }
                const int ring_end = ring_starts[r + 1];
                const int nxt = zr_clampi(v + 1 == ring_end ? ring_starts[r] : v + 1, 0, nverts - 1);
                e0[u] = vert2[v];
                e1[u] = vert2[nxt];
            }
#pragma unroll
            for (int u = 0; u < ZR_EDGES; ++u) {
                const double x0 = e0[u].x, y0 = e0[u].y, x1 = e1[u].x, y1 = e1[u].y;
                if (y0 == y1) continue;
                const bool up = y0 < y1;
                const double xa = up ? x0 : x1, ya = up ? y0 : y1, xb = up ? x1 : x0, yb = up ? y1 : y0;
                if (!(ya <= cy_last && cy_first < yb)) continue;                 // crosses no row of this band
                for (int k = 0; k < nrows; ++k) {
                    const double cy = (double)(row0 + k) + 0.5;
                    if (!(ya <= cy && cy < yb)) continue;
                    const double xc = xa + ((cy - ya) * (xb - xa)) / (yb - ya);
                    // the first column j with xc <= j + 0.5, clipped to the tile
                    int col;
                    if (!(xc > first)) col = col0;
                    else if (xc > last) continue;
                    else {
                        const double f = floor(xc);                              // col0 <= f <= col1 - 1
                        col = (int)f + (xc > f + 0.5 ? 1 : 0);
                        if (col < col0 || col >= col1) continue;                 // never: first < xc <= last
                    }
                    const int bit = col - col0;
                    atomicXor(&s_bits[k][bit >> 5], 1u << (bit & 31));
                }
            }
        }
        __syncthreads();

        // crossings -> inside bits: bit j becomes the XOR of the bits 0 .. j of its row.  A wave takes a row at a time, 64 words a step
        for (int k = wv; k < nrows; k += ZR_THREADS / 64) {
            unsigned int carry = 0u;
            for (int i0 = 0; i0 < nwords; i0 += 64) {
                const int i = i0 + lane;
                unsigned int x = i < nwords ? s_bits[k][i] : 0u;
                x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
                const unsigned long long odd = __ballot((x >> 31) != 0u);        // words that hand an odd parity on
                if ((carry + (unsigned int)__builtin_popcountll(odd & below)) & 1u) x = ~x;
                carry = (carry + (unsigned int)__builtin_popcountll(odd)) & 1u;
                if (i < nwords) s_bits[k][i] = x;
            }
        }
        __syncthreads();

        // the labels: a lane takes a pixel, 64 columns a step
        for (int k = wv; k < nrows; k += ZR_THREADS / 64) {
            int *row = labels + (size_t)(row0 + k) * (size_t)w;
            for (int c = col0; c < col1; c += 64) {
                const int col = c + lane;
                const int i = ((c - col0) >> 5) + (lane >> 5);
                const unsigned int word = i < nwords ? s_bits[k][i] : 0u;
                const bool in = col < col1 && ((word >> (lane & 31)) & 1u);
                if (in) atomicMax(&row[col], p + 1);
            }
        }
        __syncthreads();                                                         // the next job clears the bitmap
    }
}

// ===========================================================================
// 4. int32 labels -> uint8 / uint16
// ===========================================================================
template <typename LAB>
__global__ __launch_bounds__(256) void k_zr_narrow(const int *__restrict__ labels, long long npix, LAB *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) out[i] = (LAB)labels[i];
}

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" size_t lars_zone_rasterize_scratch_bytes(int64_t npolys)
{
    if (npolys < 1 || npolys > LARS_ZONES_MAX) return 0;
    Carver c(nullptr);
    c.take<ZrBox>((size_t)npolys);
    c.take<unsigned long long>((size_t)npolys + 1);
    return c.bytes();
}

extern "C" int lars_d_zone_rasterize(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                                     int64_t npolys, int64_t h, int64_t w, int32_t *labels, void *scratch, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!verts || !ring_starts || !poly_starts || !labels || !scratch || npolys < 1 || npolys > LARS_ZONES_MAX || nrings < npolys ||
        nverts < 3 * nrings || nverts > LARS_ZONE_VERTS_MAX || h <= 0 || w <= 0 || h > (1 << 24) || w > (1 << 24))
        return fail(LARS_ERR_INVALID, "lars_d_zone_rasterize: bad arguments (1 to %d polygons of one ring or more, rings of three vertices or more, "
                                      "at most %d vertices, a raster of 1 to 2^24 on each side)", LARS_ZONES_MAX, LARS_ZONE_VERTS_MAX);
    if (!aligned_to(verts, 16) || !aligned_to(labels, 4) || !aligned_to(scratch, 256))
        return fail(LARS_ERR_INVALID, "lars_d_zone_rasterize: verts must be 16-byte, labels 4-byte and scratch 256-byte aligned");
    hipStream_t s = pick_stream(c, stream);
    Carver cv(scratch);
    ZrBox *boxes = cv.take<ZrBox>((size_t)npolys);
    unsigned long long *jobs = cv.take<unsigned long long>((size_t)npolys + 1);
    LARS_HIP_TRY(hipMemsetAsync(labels, 0, (size_t)h * (size_t)w * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_zr_bounds, dim3((unsigned int)npolys), dim3(256), 0, s, verts, (int)nverts, ring_starts, (int)nrings, poly_starts,
                       (int)npolys, (int)h, (int)w, boxes, jobs);
    hipLaunchKernelGGL(k_zr_starts, dim3(1), dim3(1024), 0, s, jobs, (int)npolys);
    // the grid needs no count from the device: workgroups stride over the jobs, and those past the last job leave at once
    const int64_t bands = (h + ZR_ROWS - 1) / ZR_ROWS, tiles = (((w + 31) >> 5) + ZR_WORDS - 1) / ZR_WORDS;
    const int64_t most = npolys * bands * tiles;
    hipLaunchKernelGGL(k_zr_fill, dim3((unsigned int)(most < 16384 ? most : 16384)), dim3(ZR_THREADS), 0, s, verts, (int)nverts, ring_starts, (int)nrings,
                       poly_starts, (int)npolys, boxes, jobs, (int)h, (int)w, labels);
    return launch_check("lars_d_zone_rasterize");
}

extern "C" int lars_d_zone_labels_narrow(const int32_t *labels, int64_t npix, int zone_bytes, void *out, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!labels || !out || npix <= 0 || (zone_bytes != 1 && zone_bytes != 2) || !aligned_to(out, (uintptr_t)zone_bytes))
        return fail(LARS_ERR_INVALID, "lars_d_zone_labels_narrow: bad arguments (labels of 1 or 2 bytes out)");
    hipStream_t s = pick_stream(c, stream);
    const dim3 grid(grid_1d(npix)), block(256);
    if (zone_bytes == 1) hipLaunchKernelGGL((k_zr_narrow<uint8_t>), grid, block, 0, s, labels, (long long)npix, static_cast<uint8_t *>(out));
    else hipLaunchKernelGGL((k_zr_narrow<uint16_t>), grid, block, 0, s, labels, (long long)npix, static_cast<uint16_t *>(out));
    return launch_check("lars_d_zone_labels_narrow");
}
