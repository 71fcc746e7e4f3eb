// Zones from regions (DESIGN.md "Zones from regions"): the label raster zonal.hip reads, made on the device from a foreground mask by
// connected-component labelling -- the canopy patches, gaps and wet spots of an index map nobody drew outlines for.
//
// The definition.  mask[h][w], nonzero = foreground, h * w < 2^31.  Two foreground pixels are neighbours when they share an edge
// (connectivity 4) or an edge or a corner (8).  A region is a maximal connected set of foreground pixels; regions are numbered
// 1 .. R in raster order of their first pixel (their smallest flat index y * w + x).  Regions of fewer than min_pixels pixels become
// 0 and the others keep their order.  Per region: area, bounding box (row0, col0, row1, col1; half-open) and the sums of the pixel
// rows and columns.  Integer arithmetic throughout: the result is this definition bit for bit on every run.
//
// A union-find over the raster whose root is always the smaller flat index, so the root of a region is its first pixel and the
// numbering is a prefix sum over the root flags: no sort.  The stages are launches; no workgroup ever waits for another.
//   k_rg_local    one workgroup per RG_T x RG_T tile: every foreground pixel starts as itself in LDS, joins its left / upper (and
//                 diagonal) neighbours by compare-and-retry unions, and the flattened parents go out as flat indices (-1: background)
//   k_rg_seam     one thread per pixel just below a horizontal tile border or just right of a vertical one: the same unions on the
//                 global parents with atomicMin, the diagonal across a tile corner included
//   k_rg_flatten  roots[i] = the root of pixel i (written into the label raster: the parents are only read)
//   k_rg_area     area per root into the parent array (zeroed in between), equal roots of a wave counted before the atomic
//   k_rg_totals / k_rg_scan_totals / k_rg_number
//                 flag = root and area >= min_pixels; per-chunk totals, their scan (and R), then the per-chunk scan: the root's slot
//                 receives its new id, the table row its area and an empty box
//   k_rg_relabel  labels[i] = id of its root, and the box and the coordinate sums of each region, a wave's run of one id folded
//                 in registers before the atomics
//
// Every index read from the parent array is used only while 0 <= parent < the index it was read at: parents only ever decrease,
// so every walk ends on its own, and an array that is no forest gives wrong labels, never an access outside the buffers.
#include "common.h"
#include "device_common.h"
#include "wg_device.h"

namespace lars {

namespace {

#define RG_T 32                         // tile edge of the local pass: 1024 pixels, 4 KiB of LDS
#define RG_THREADS 256
#define RG_ROWS 16                      // rows of a wave's strip of 64 columns (area and relabel passes)
#define RG_ROUNDS 8                     // a numbering chunk is RG_ROUNDS * 256 pixels

#define RG_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define RG_DEV __HIP_MEMORY_SCOPE_AGENT

template <int SCOPE>
__device__ inline int rg_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// the root of foreground pixel x: parents are >= 0 and never above their child, a root is its own parent
template <int SCOPE>
__device__ inline int rg_find(const int *P, int x)
{
    int q = rg_load<SCOPE>(P + x);
    while (q >= 0 && q < x) {
        x = q;
        q = rg_load<SCOPE>(P + x);
    }
    return x;
}

// Joins the trees of the foreground pixels a and b; the smaller root wins.  The atomicMin's answer says whether b was still a root
// when it was linked; if not, the walk goes on from what b pointed at.  The larger of the two roots falls every round.
template <int SCOPE>
__device__ inline void rg_union(int *P, int a, int b)
{
    for (;;) {
        a = rg_find<SCOPE>(P, a);
        b = rg_find<SCOPE>(P, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(P + b, a, __ATOMIC_RELAXED, SCOPE);
        if (old == b || old < 0) return;                                         // old < 0: never, b is foreground
        b = old;
    }
}

// ===========================================================================
// 1. the tiles
// ===========================================================================
template <bool CONN8>
__global__ __launch_bounds__(RG_THREADS) void k_rg_local(const uint8_t *__restrict__ mask, int h, int w, int tiles_x, long long ntiles,
                                                         int *__restrict__ parent)
{
    __shared__ int s_lab[RG_T * RG_T];
    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {        // block-uniform: every thread meets every barrier
        const int ty0 = (int)(tile / tiles_x) * RG_T, tx0 = (int)(tile % tiles_x) * RG_T;
        const int th = min(RG_T, h - ty0), tw = min(RG_T, w - tx0);              // the ragged tiles of the last row and column
        for (int k = tid; k < RG_T * RG_T; k += RG_THREADS) {
            const int ly = k / RG_T, lx = k % RG_T;
            const bool fg = ly < th && lx < tw && mask[(size_t)(ty0 + ly) * (size_t)w + (size_t)(tx0 + lx)] != 0;
            s_lab[k] = fg ? k : -1;                                              // local order is raster order inside the tile
        }
        __syncthreads();
        for (int k = tid; k < RG_T * RG_T; k += RG_THREADS) {
            if (rg_load<RG_WG>(s_lab + k) < 0) continue;
            const int ly = k / RG_T, lx = k % RG_T;
            if (lx > 0 && rg_load<RG_WG>(s_lab + k - 1) >= 0) rg_union<RG_WG>(s_lab, k, k - 1);
            if (ly > 0 && rg_load<RG_WG>(s_lab + k - RG_T) >= 0) rg_union<RG_WG>(s_lab, k, k - RG_T);
            if (CONN8 && ly > 0) {
                if (lx > 0 && rg_load<RG_WG>(s_lab + k - RG_T - 1) >= 0) rg_union<RG_WG>(s_lab, k, k - RG_T - 1);
                if (lx < RG_T - 1 && rg_load<RG_WG>(s_lab + k - RG_T + 1) >= 0) rg_union<RG_WG>(s_lab, k, k - RG_T + 1);
            }
        }
        __syncthreads();
        for (int k = tid; k < RG_T * RG_T; k += RG_THREADS) {
            const int ly = k / RG_T, lx = k % RG_T;
            if (ly >= th || lx >= tw) continue;
            int out = -1;
            if (s_lab[k] >= 0) {
                const int r = rg_find<RG_WG>(s_lab, k);                          // 0 <= r <= k: a pixel of this tile
                out = (int)((long long)(ty0 + r / RG_T) * w + (tx0 + r % RG_T));
            }
            parent[(size_t)(ty0 + ly) * (size_t)w + (size_t)(tx0 + lx)] = out;
        }
        __syncthreads();                                                         // the next tile overwrites the labels
    }
}

// ===========================================================================
// 2. the seams
// ===========================================================================
__device__ inline void rg_join(int *P, int a, int b)
{
    if (rg_load<RG_DEV>(P + b) >= 0) rg_union<RG_DEV>(P, a, b);
}

// jobs 0 .. nh - 1: pixel (y, x) of the first row of a tile row (y = RG_T, 2 RG_T, ..) with the row above it;
// jobs nh .. nh + nv - 1: pixel (y, x) of the first column of a tile column with the column left of it.  The diagonal across a tile
// corner is one of the row jobs' pairs; pairs met twice are joined twice, which changes nothing.
template <bool CONN8>
__global__ __launch_bounds__(256) void k_rg_seam(int *__restrict__ parent, int h, int w, long long nh, long long nv)
{
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nh + nv; j += (long long)gridDim.x * 256) {
        if (j < nh) {
            const int y = (int)(j / w + 1) * RG_T, x = (int)(j % w);             // 1 <= y < h by the count of the jobs
            const int a = (int)((long long)y * w + x), b = a - w;
            if (rg_load<RG_DEV>(parent + a) < 0) continue;
            rg_join(parent, a, b);
            if (CONN8 && x > 0) rg_join(parent, a, b - 1);
            if (CONN8 && x + 1 < w) rg_join(parent, a, b + 1);
        } else {
            const long long k = j - nh;
            const int x = (int)(k / h + 1) * RG_T, y = (int)(k % h);             // 1 <= x < w
            const int a = (int)((long long)y * w + x), b = a - 1;
            if (rg_load<RG_DEV>(parent + a) < 0) continue;
            rg_join(parent, a, b);
            if (CONN8 && y > 0) rg_join(parent, a, b - w);
            if (CONN8 && y + 1 < h) rg_join(parent, a, b + w);
        }
    }
}

// ===========================================================================
// 3. roots
// ===========================================================================
__global__ __launch_bounds__(256) void k_rg_flatten(const int *__restrict__ parent, long long npix, int *__restrict__ roots)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        int x = (int)i, q = parent[i];
        const bool fg = q >= 0;
        while (q >= 0 && q < x) {
            x = q;
            q = parent[x];
        }
        roots[i] = fg ? x : -1;
    }
}

// A wave walks strips of 64 columns x RG_ROWS rows, so that the row is one value for the wave; strips are wave-strided, and every
// lane stays in every ballot (a lane right of the picture holds no key).
struct RgStrips {
    long long strips, strip, step;
    int ncs, lane;
    __device__ RgStrips(int h, int w)
    {
        ncs = (w + 63) / 64;
        strips = (long long)ncs * ((h + RG_ROWS - 1) / RG_ROWS);
        lane = threadIdx.x & 63;
        strip = (long long)blockIdx.x * (RG_THREADS / 64) + (threadIdx.x >> 6);
        step = (long long)gridDim.x * (RG_THREADS / 64);
    }
    __device__ int col0() const { return (int)(strip % ncs) * 64; }
    __device__ int row0() const { return (int)(strip / ncs) * RG_ROWS; }
};

// ===========================================================================
// 4. areas, at the roots
// ===========================================================================
__global__ __launch_bounds__(RG_THREADS) void k_rg_area(const int *__restrict__ roots, int h, int w, long long npix, unsigned int *__restrict__ area)
{
    RgStrips S(h, w);
    int held = -1;
    unsigned int held_n = 0;
    for (; S.strip < S.strips; S.strip += S.step) {
        const int x = S.col0() + S.lane, y0 = S.row0(), y1 = min(h, y0 + RG_ROWS);
        for (int y = y0; y < y1; ++y) {
            int key = x < w ? roots[(size_t)y * (size_t)w + (size_t)x] : -1;
            if ((long long)key >= npix) key = -1;                                // never: a root is a pixel
            unsigned long long todo = __ballot(key >= 0);
            while (todo) {
                const int z = __shfl(key, __builtin_ctzll(todo), 64);
                const unsigned long long same = __ballot(key == z);
                if (z != held) {
                    if (S.lane == 0 && held_n) atomicAdd(&area[held], held_n);
                    held = z;
                    held_n = 0;
                }
                held_n += (unsigned int)__builtin_popcountll(same);
                todo &= ~same;
            }
        }
    }
    if (S.lane == 0 && held_n) atomicAdd(&area[held], held_n);
}

// ===========================================================================
// 5. numbering: a device-wide exclusive scan of the flags in three launches
// ===========================================================================
__device__ inline bool rg_flag(const int *roots, const unsigned int *area, long long i, unsigned int min_pixels)
{
    return roots[i] == (int)i && area[i] >= min_pixels;
}

__global__ __launch_bounds__(256) void k_rg_totals(const int *__restrict__ roots, const unsigned int *__restrict__ area, long long npix,
                                                   unsigned int min_pixels, long long nchunks, unsigned int *__restrict__ totals)
{
    __shared__ unsigned int s_w[4];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        unsigned int n = 0;
        for (int r = 0; r < RG_ROUNDS; ++r) {
            const long long i = (c * RG_ROUNDS + r) * 256 + threadIdx.x;
            n += (i < npix && rg_flag(roots, area, i, min_pixels)) ? 1u : 0u;
        }
        unsigned int total;
        wg_exscan<256, unsigned int>(n, s_w, &total);
        if (threadIdx.x == 0) totals[c] = total;
    }
}

__global__ __launch_bounds__(1024) void k_rg_scan_totals(unsigned int *__restrict__ totals, long long nchunks, long long *__restrict__ count_out)
{
    const unsigned int total = wg_scan_array<unsigned int>(
        nchunks, [&](long long i) { return totals[i]; }, [&](long long i, unsigned int before) { totals[i] = before; });
    if (threadIdx.x == 0) *count_out = (long long)total;
}

// area[i] of a counted root becomes its id 1 .. R, every other slot 0; table rows below the capacity get their area and an empty box
__global__ __launch_bounds__(256) void k_rg_number(const int *__restrict__ roots, unsigned int *__restrict__ area, long long npix,
                                                   unsigned int min_pixels, long long nchunks, const unsigned int *__restrict__ before,
                                                   lars_region *__restrict__ table, long long capacity)
{
    __shared__ unsigned int s_w[4];
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        unsigned int carry = before[c];
        for (int r = 0; r < RG_ROUNDS; ++r) {
            const long long i = (c * RG_ROUNDS + r) * 256 + threadIdx.x;
            const bool f = i < npix && rg_flag(roots, area, i, min_pixels);
            unsigned int total;
            const unsigned int ex = wg_exscan<256, unsigned int>(f ? 1u : 0u, s_w, &total);
            if (i < npix) {
                const unsigned int n = area[i], id = carry + ex + 1u;
                area[i] = f ? id : 0u;
                if (f && (long long)id <= capacity) {
                    lars_region t;
                    t.area = (int64_t)n;
                    t.bbox[0] = 0x7FFFFFFF; t.bbox[1] = 0x7FFFFFFF; t.bbox[2] = 0; t.bbox[3] = 0;
                    t.row_sum = 0; t.col_sum = 0;
                    table[id - 1u] = t;
                }
            }
            carry += total;
        }
    }
}

// ===========================================================================
// 6. labels and the table
// ===========================================================================
__device__ inline unsigned int rg_bit_positions(unsigned long long m)            // the sum of the positions of the set bits
{
    return (unsigned int)__builtin_popcountll(m & 0xAAAAAAAAAAAAAAAAull) + ((unsigned int)__builtin_popcountll(m & 0xCCCCCCCCCCCCCCCCull) << 1) +
           ((unsigned int)__builtin_popcountll(m & 0xF0F0F0F0F0F0F0F0ull) << 2) + ((unsigned int)__builtin_popcountll(m & 0xFF00FF00FF00FF00ull) << 3) +
           ((unsigned int)__builtin_popcountll(m & 0xFFFF0000FFFF0000ull) << 4) + ((unsigned int)__builtin_popcountll(m & 0xFFFFFFFF00000000ull) << 5);
}

struct RgHeld {                          // what a wave holds for the id it met last: all of it wave-uniform
    unsigned int id;
    int r0, r1, c0, c1;                  // inclusive
    unsigned long long rsum, csum;
    __device__ void start(unsigned int z) { id = z; r0 = c0 = 0x7FFFFFFF; r1 = c1 = -1; rsum = csum = 0; }
    __device__ void flush(lars_region *table, int lane) const
    {
        if (!id || r1 < 0) return;
        lars_region *t = table + (id - 1u);
        if (lane == 0) atomicMin(&t->bbox[0], r0);
        if (lane == 1) atomicMin(&t->bbox[1], c0);
        if (lane == 2) atomicMax(&t->bbox[2], r1 + 1);
        if (lane == 3) atomicMax(&t->bbox[3], c1 + 1);
        if (lane == 4) atomicAdd(reinterpret_cast<unsigned long long *>(&t->row_sum), rsum);
        if (lane == 5) atomicAdd(reinterpret_cast<unsigned long long *>(&t->col_sum), csum);
    }
};

__global__ __launch_bounds__(RG_THREADS) void k_rg_relabel(int *__restrict__ labels, const unsigned int *__restrict__ ids, int h, int w, long long npix,
                                                           lars_region *__restrict__ table, long long capacity)
{
    RgStrips S(h, w);
    RgHeld H;
    H.start(0u);
    for (; S.strip < S.strips; S.strip += S.step) {
        const int x0 = S.col0(), x = x0 + S.lane, y0 = S.row0(), y1 = min(h, y0 + RG_ROWS);
        for (int y = y0; y < y1; ++y) {
            unsigned int id = 0u;
            if (x < w) {
                const size_t i = (size_t)y * (size_t)w + (size_t)x;
                const int r = labels[i];
                if (r >= 0 && (long long)r < npix) id = ids[r];
                labels[i] = (int)id;
            }
            const unsigned int key = (long long)id <= capacity ? id : 0u;        // rows past the capacity do not exist
            unsigned long long todo = __ballot(key != 0u);
            while (todo) {
                const unsigned int z = __shfl(key, __builtin_ctzll(todo), 64);
                const unsigned long long same = __ballot(key == z);
                if (z != H.id) {
                    H.flush(table, S.lane);
                    H.start(z);
                }
                const unsigned int n = (unsigned int)__builtin_popcountll(same);
                H.r0 = min(H.r0, y); H.r1 = max(H.r1, y);
                H.c0 = min(H.c0, x0 + (int)__builtin_ctzll(same)); H.c1 = max(H.c1, x0 + 63 - (int)__builtin_clzll(same));
                H.rsum += (unsigned long long)y * n;
                H.csum += (unsigned long long)x0 * n + rg_bit_positions(same);
                todo &= ~same;
            }
        }
    }
    H.flush(table, S.lane);
}

// ===========================================================================
// the mask of the picture routes
// ===========================================================================
// given may be mask itself: a thread reads and writes its own pixel only
__global__ __launch_bounds__(256) void k_rg_mask(const float *__restrict__ x, const uint8_t *given, const uint8_t *__restrict__ valid,
                                                 long long npix, float t, int below, uint8_t *mask)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        bool in = (!given || given[i] != 0) && (!valid || valid[i] != 0);
        if (in && x) in = below ? x[i] < t : x[i] > t;                           // false for a NaN either way
        mask[i] = in ? 1 : 0;
    }
}

long long rg_chunks(long long npix) { return (npix + RG_ROUNDS * 256 - 1) / (RG_ROUNDS * 256); }

unsigned int rg_grid(long long blocks, long long most) { return (unsigned int)(blocks < 1 ? 1 : blocks < most ? blocks : most); }

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" size_t lars_region_label_scratch_bytes(int64_t h, int64_t w)
{
    if (h < 1 || w < 1 || h > 0x7FFFFFFF / w) return 0;                          // h * w < 2^31
    Carver c(nullptr);
    c.take<int>((size_t)(h * w));
    c.take<unsigned int>((size_t)rg_chunks(h * w) + 1);
    return c.bytes();
}

extern "C" int lars_d_region_label(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int32_t *labels,
                                   lars_region *table, int64_t capacity, int64_t *count_dev, void *scratch, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!mask || !labels || !count_dev || !scratch || h < 1 || w < 1 || h > 0x7FFFFFFF / w || (connectivity != 4 && connectivity != 8) ||
        min_pixels < 1 || capacity < 0 || (capacity > 0 && !table))
        return fail(LARS_ERR_INVALID, "lars_d_region_label: bad arguments (a raster of 1 or more on each side and fewer than 2^31 pixels, connectivity 4 or 8, "
                                      "min_pixels >= 1, a table of capacity >= 0)");
    if (!aligned_to(labels, 4) || !aligned_to(table, 8) || !aligned_to(count_dev, 8) || !aligned_to(scratch, 256))
        return fail(LARS_ERR_INVALID, "lars_d_region_label: labels must be 4-byte, table and count 8-byte and scratch 256-byte aligned");
    hipStream_t s = pick_stream(c, stream);
    const long long npix = h * w, nchunks = rg_chunks(npix);
    Carver cv(scratch);
    int *parent = cv.take<int>((size_t)npix);
    unsigned int *totals = cv.take<unsigned int>((size_t)nchunks + 1);
    unsigned int *area = reinterpret_cast<unsigned int *>(parent);               // the parents are done with when the areas begin
    const unsigned int minpix = (unsigned int)(min_pixels < 0x7FFFFFFF ? min_pixels : 0x7FFFFFFF);   // no region has 2^31 - 1 pixels

    const int tiles_x = (int)((w + RG_T - 1) / RG_T);
    const long long ntiles = (long long)tiles_x * ((h + RG_T - 1) / RG_T);
    const long long nh = ((h - 1) / RG_T) * w, nv = ((w - 1) / RG_T) * h;
    const dim3 tile_grid(rg_grid(ntiles, 65536)), pix_grid(grid_1d(npix)), chunk_grid(rg_grid(nchunks, 65536));
    const dim3 strip_grid(rg_grid((((w + 63) / 64) * ((h + RG_ROWS - 1) / RG_ROWS) + 3) / 4, 8192));
    const int ih = (int)h, iw = (int)w;
    if (connectivity == 8) hipLaunchKernelGGL((k_rg_local<true>), tile_grid, dim3(RG_THREADS), 0, s, mask, ih, iw, tiles_x, ntiles, parent);
    else hipLaunchKernelGGL((k_rg_local<false>), tile_grid, dim3(RG_THREADS), 0, s, mask, ih, iw, tiles_x, ntiles, parent);
    if (nh + nv > 0) {
        if (connectivity == 8) hipLaunchKernelGGL((k_rg_seam<true>), dim3(grid_1d(nh + nv)), dim3(256), 0, s, parent, ih, iw, nh, nv);
        else hipLaunchKernelGGL((k_rg_seam<false>), dim3(grid_1d(nh + nv)), dim3(256), 0, s, parent, ih, iw, nh, nv);
    }
    hipLaunchKernelGGL(k_rg_flatten, pix_grid, dim3(256), 0, s, parent, npix, labels);
    LARS_HIP_TRY(hipMemsetAsync(area, 0, (size_t)npix * sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_rg_area, strip_grid, dim3(RG_THREADS), 0, s, labels, ih, iw, npix, area);
    hipLaunchKernelGGL(k_rg_totals, chunk_grid, dim3(256), 0, s, labels, area, npix, minpix, nchunks, totals);
    hipLaunchKernelGGL(k_rg_scan_totals, dim3(1), dim3(1024), 0, s, totals, nchunks, reinterpret_cast<long long *>(count_dev));
    hipLaunchKernelGGL(k_rg_number, chunk_grid, dim3(256), 0, s, labels, area, npix, minpix, nchunks, totals, table, (long long)capacity);
    hipLaunchKernelGGL(k_rg_relabel, strip_grid, dim3(RG_THREADS), 0, s, labels, area, ih, iw, npix, table, (long long)capacity);
    return launch_check("lars_d_region_label");
}

extern "C" int lars_d_region_mask_f32(const float *x, const uint8_t *given, const uint8_t *valid, int64_t npix, float t, int below,
                                      uint8_t *mask, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if ((!x && !given) || !mask || npix <= 0) return fail(LARS_ERR_INVALID, "lars_d_region_mask_f32: a plane or a given mask, and the mask out, are required");
    hipLaunchKernelGGL(k_rg_mask, dim3(grid_1d(npix)), dim3(256), 0, pick_stream(c, stream), x, given, valid, (long long)npix, t, below, mask);
    return launch_check("lars_d_region_mask_f32");
}
