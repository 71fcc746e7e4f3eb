// Zonal statistics (DESIGN.md "Zonal statistics"): one record per plot from a label raster.  labels[i] in 0 .. Z says which
// zone pixel i belongs to (0 = none); for zone z the record and the two middle order statistics are those of
// S_z = plane[valid & (labels == z)], by the rules of k_array_stats / the radix select of arrays.hip
// (process-images.py:492-513 on each zone's values, process-ndvi.py:97 for the histogram).
//
// Four stages, a segmented count / scatter / select:
//   k_zone_count    counts[z] = |S_z| (entry 0: label 0 and invalid pixels), bad = labels outside 0 .. Z
//   k_zone_offsets  ends[j] = counts[1] + .. + counts[j]: zone z owns the slots ends[z - 1] .. ends[z] - 1
//   k_zone_scatter  every valid pixel of a zone takes a slot of its zone's segment; up to three planes share the slot
//   k_zone_stats    one workgroup per zone: the record and the median pair of its segment
//
// Neighbouring pixels mostly share a label, so the count and the scatter aggregate per wave before they touch memory: take
// the first live lane's label, ballot the lanes that hold it, let that lane add the popcount, retire those lanes, until no
// lane is left -- one to three atomics per 64 pixels on a plot map instead of 64 on one address.  The loop's condition is a
// ballot, so every lane of the wave stays in it until it is empty.  A lane takes one pixel: labels are 1, 2 or 4 bytes
// wide, a wave's load is one to four cache lines either way, and no tail needs a path of its own.
//
// Order inside a segment is whatever the atomics gave: the double sums depend on it (within the mean's tolerance), nothing
// else does.
#include <string.h>

#include "common.h"
#include "device_common.h"
#include "wg_device.h"

namespace lars {

namespace {

#define ZONE_NONE 0xFFFFFFFFu                    // a lane with nothing to add: past the end, or a label outside 0 .. Z

// label of pixel i as a key: 0 .. Z, or ZONE_NONE (counted in `bad`) outside that range
template <typename LAB>
__device__ inline unsigned int zone_key(const LAB *__restrict__ labels, long long i, unsigned int nzones, bool &bad)
{
    const long long v = (long long)labels[i];
    bad = v < 0 || v > (long long)nzones;
    return bad ? ZONE_NONE : (unsigned int)v;
}

// ===========================================================================
// 1. counts
// ===========================================================================
// A wave keeps the label it met last and what it counted for it in registers (both wave-uniform) and goes to memory when the
// label changes: inside a large plot that is one atomic per wave, not one per 64 pixels.
template <typename LAB>
__global__ __launch_bounds__(256) void k_zone_count(const LAB *__restrict__ labels, const uint8_t *__restrict__ valid, long long npix,
                                                    unsigned int nzones, unsigned long long *__restrict__ counts,
                                                    unsigned long long *__restrict__ bad_out)
{
    const int lane = threadIdx.x & 63;
    unsigned int held = ZONE_NONE;
    unsigned long long held_count = 0, nbad = 0, nzero = 0;
    const long long first = (long long)blockIdx.x * 256 + (threadIdx.x & ~63);
    for (long long i0 = first; i0 < npix; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + lane;
        unsigned int key = ZONE_NONE;
        bool bad = false;
        if (i < npix) {
            key = zone_key<LAB>(labels, i, nzones, bad);
            if (!bad && valid && !valid[i]) key = 0u;
        }
        nbad += (unsigned long long)__builtin_popcountll(__ballot(bad));
        // entry 0 is the one address every wave of a plot map would meet at (the paths between the plots): it stays in a register
        // until the wave is done -- with it in the loop below this kernel took 2.8 ms on 2000 plots at 4096x4096, ten times the scatter
        nzero += (unsigned long long)__builtin_popcountll(__ballot(key == 0u));
        unsigned long long todo = __ballot(key != ZONE_NONE && key != 0u);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const unsigned int z = __shfl(key, leader, 64);
            const unsigned long long same = __ballot(key == z);
            if (z != held) {
                if (lane == 0 && held_count) atomicAdd(&counts[held], held_count);
                held = z;
                held_count = 0;
            }
            held_count += (unsigned long long)__builtin_popcountll(same);
            todo &= ~same;
        }
    }
    if (lane == 0 && held_count) atomicAdd(&counts[held], held_count);
    if (lane == 0 && nzero) atomicAdd(&counts[0], nzero);
    if (lane == 0 && nbad) atomicAdd(bad_out, nbad);
}

// ===========================================================================
// 2. segment ends (an inclusive scan of counts[1 .. Z]; ends[0] = 0) and the cursors
// ===========================================================================
__global__ __launch_bounds__(256) void k_zone_offsets(const unsigned long long *__restrict__ counts, unsigned int nzones,
                                                      unsigned long long *__restrict__ ends, unsigned long long *__restrict__ cursors)
{
    __shared__ unsigned long long s_cum[4];
    const int tid = threadIdx.x;
    const unsigned int per = (nzones + 255u) / 256u;             // consecutive zones per thread
    const unsigned int z0 = 1u + (unsigned int)tid * per;
    unsigned long long local = 0;
    for (unsigned int j = 0; j < per; ++j)
        if (z0 + j <= nzones) local += counts[z0 + j];
    unsigned long long run = wg_exscan<256>(local, s_cum);
    for (unsigned int j = 0; j < per; ++j) {
        const unsigned int z = z0 + j;
        if (z > nzones) break;
        run += counts[z];
        ends[z] = run;
        cursors[z] = 0ull;
    }
    if (tid == 0) { ends[0] = 0ull; cursors[0] = 0ull; }
}

// ===========================================================================
// 3. scatter
// ===========================================================================
struct ScatterParams {
    const float *plane[3];
    float *out[3];
    const uint8_t *valid;
    long long npix;
    unsigned int nzones;
    const unsigned long long *ends;
    unsigned long long *cursors;
};

template <typename LAB>
__global__ __launch_bounds__(256) void k_zone_scatter(const LAB *__restrict__ labels, ScatterParams P)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long first = (long long)blockIdx.x * 256 + (threadIdx.x & ~63);
    for (long long i0 = first; i0 < P.npix; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + lane;
        unsigned int key = ZONE_NONE;
        if (i < P.npix) {
            bool bad;
            key = zone_key<LAB>(labels, i, P.nzones, bad);
            if (key == 0u || (P.valid && !P.valid[i])) key = ZONE_NONE;   // in no zone, or no picture
        }
        unsigned long long todo = __ballot(key != ZONE_NONE);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const unsigned int z = __shfl(key, leader, 64);
            const unsigned long long same = __ballot(key == z);
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(&P.cursors[z], (unsigned long long)__builtin_popcountll(same));
            base = __shfl(base, leader, 64);
            if (key == z) {
                const unsigned long long slot = P.ends[z - 1] + base + (unsigned long long)__builtin_popcountll(same & below);
                // counts taken from these labels and this mask never trip this; counts from anywhere else must not write outside the segment
                if (slot < P.ends[z])
                    for (int k = 0; k < 3; ++k)
                        if (P.plane[k]) P.out[k][slot] = P.plane[k][i];
            }
            todo &= ~same;
        }
    }
}

// ===========================================================================
// 4. one record and one median pair per zone
// ===========================================================================
// A workgroup takes a zone, zones are grid-strided.  The record follows k_array_stats; the rank (n - 1) / 2 comes from a
// radix select over KeyOf<float>'s key, eight bits a pass with the histogram in LDS, and the rank n / 2 from the count of the
// keys up to the selected one and the smallest key above it, as k_sel_next / k_sel_finish form it.
__global__ __launch_bounds__(256) void k_zone_stats(const float *__restrict__ values, const unsigned long long *__restrict__ ends,
                                                    unsigned int nzones, float thr, int want_hist, unsigned long long split,
                                                    lars_stats *__restrict__ stats, float *__restrict__ medians)
{
    __shared__ unsigned int s_hist[LARS_HIST_BINS];
    __shared__ HistCell<float> s_edges[LARS_HIST_CELLS];
    __shared__ StatPartial s_part[4];
    __shared__ unsigned int s_bins[256];
    __shared__ unsigned long long s_w[8];                                       // the scans' and the reductions' words
    __shared__ unsigned int s_prefix;
    __shared__ unsigned long long s_rank;
    const int tid = threadIdx.x;
    hist_cells_init<float>(s_edges, tid);
    __syncthreads();
    for (unsigned int z = 1u + blockIdx.x; z <= nzones; z += gridDim.x) {       // block-uniform: every thread meets every barrier
        const unsigned long long lo = ends[z - 1], n = ends[z] - lo;
        if (n > split) continue;                                                // the host runs the array kernels on this segment
        lars_stats *out = stats + (z - 1);
        const float *x = values + lo;
        if (tid < LARS_HIST_BINS) s_hist[tid] = 0;
        __syncthreads();
        StatPartial p;
        p.init();
        for (unsigned long long i = tid; i < n; i += 256) {
            const float v = x[i];
            if (!p.push(v, thr)) continue;
            if (want_hist && v >= -1.0f && v <= 1.0f) atomicAdd(&s_hist[hist_bin_cell<float>(v, s_edges)], 1u);
        }
        p.block_reduce(s_part);
        if (tid == 0) p.to_stats(out, (double)thr);
        if (tid < LARS_HIST_BINS) out->hist[tid] = want_hist ? (unsigned long long)s_hist[tid] : 0ull;
        if (n == 0) {                                                           // an empty zone: count 0 says so, the pair is never read
            if (tid < 2) medians[2 * (size_t)(z - 1) + tid] = __builtin_bit_cast(float, 0x7FC00000u);
            __syncthreads();
            continue;
        }
        // radix select of rank k0 = (n - 1) / 2
        if (tid == 0) { s_prefix = 0u; s_rank = (n - 1) / 2; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            s_bins[tid] = 0u;
            __syncthreads();
            const unsigned int prefix = s_prefix;
            for (unsigned long long i = tid; i < n; i += 256) {
                const unsigned int key = f32_key(x[i]);
                if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_bins[(key >> shift) & 0xFFu], 1u);
            }
            __syncthreads();
            const unsigned long long c = s_bins[tid], k = s_rank;
            const unsigned long long before = wg_exscan<256>(c, s_w);
            if (c && k >= before && k < before + c) {                           // exactly one thread
                s_prefix = prefix | ((unsigned int)tid << shift);
                s_rank = k - before;
            }
            __syncthreads();
        }
        // keys up to the selected one, and the smallest key above it
        const unsigned int sel = s_prefix;
        unsigned long long c_le = 0, nxt = ~0ull;
        for (unsigned long long i = tid; i < n; i += 256) {
            const unsigned long long key = f32_key(x[i]);
            if (key <= sel) ++c_le;
            else nxt = key < nxt ? key : nxt;
        }
        wg_count_le_next<256>(c_le, nxt, s_w);
        if (tid == 0) {
            const unsigned long long k0 = (n - 1) / 2, k1 = n / 2;
            const float v1 = key_f32(sel);
            float v2 = v1;
            if (k1 != k0 && k1 >= c_le) v2 = key_f32((unsigned int)nxt);   // k1 >= c_le: a key above the selected one exists
            medians[2 * (size_t)(z - 1)] = v1;
            medians[2 * (size_t)(z - 1) + 1] = v2;
        }
        __syncthreads();
    }
}

bool zone_args_ok(const void *zones, int zone_bytes, int64_t npix, int64_t nzones)
{
    if (!zones || npix <= 0 || nzones < 1 || nzones > LARS_ZONES_MAX) return false;
    if (zone_bytes != 1 && zone_bytes != 2 && zone_bytes != 4) return false;
    return aligned_to(zones, (uintptr_t)zone_bytes);
}

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" int lars_d_zone_count(const void *zones, int zone_bytes, const uint8_t *valid, int64_t npix, int64_t nzones, uint64_t *counts_dev,
                                 uint64_t *bad_dev, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!zone_args_ok(zones, zone_bytes, npix, nzones) || !counts_dev || !bad_dev)
        return fail(LARS_ERR_INVALID, "lars_d_zone_count: bad arguments (labels of 1, 2 or 4 bytes, 1 to %d zones)", LARS_ZONES_MAX);
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)(nzones + 1) * sizeof(uint64_t), s));
    LARS_HIP_TRY(hipMemsetAsync(bad_dev, 0, sizeof(uint64_t), s));
    const dim3 grid(grid_1d(npix)), block(256);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts_dev), *bad = reinterpret_cast<unsigned long long *>(bad_dev);
    if (zone_bytes == 1)
        hipLaunchKernelGGL((k_zone_count<uint8_t>), grid, block, 0, s, static_cast<const uint8_t *>(zones), valid, (long long)npix, (unsigned int)nzones, cnt, bad);
    else if (zone_bytes == 2)
        hipLaunchKernelGGL((k_zone_count<uint16_t>), grid, block, 0, s, static_cast<const uint16_t *>(zones), valid, (long long)npix, (unsigned int)nzones, cnt, bad);
    else
        hipLaunchKernelGGL((k_zone_count<int32_t>), grid, block, 0, s, static_cast<const int32_t *>(zones), valid, (long long)npix, (unsigned int)nzones, cnt, bad);
    return launch_check("lars_d_zone_count");
}

extern "C" int lars_d_zone_offsets(const uint64_t *counts_dev, int64_t nzones, uint64_t *offsets_dev, uint64_t *cursors_dev, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!counts_dev || !offsets_dev || !cursors_dev || nzones < 1 || nzones > LARS_ZONES_MAX)
        return fail(LARS_ERR_INVALID, "lars_d_zone_offsets: bad arguments (1 to %d zones)", LARS_ZONES_MAX);
    hipLaunchKernelGGL(k_zone_offsets, dim3(1), dim3(256), 0, pick_stream(c, stream), reinterpret_cast<const unsigned long long *>(counts_dev),
                       (unsigned int)nzones, reinterpret_cast<unsigned long long *>(offsets_dev), reinterpret_cast<unsigned long long *>(cursors_dev));
    return launch_check("lars_d_zone_offsets");
}

extern "C" int lars_d_zone_scatter(const float *const planes[3], uint32_t index_mask, const void *zones, int zone_bytes, const uint8_t *valid,
                                   int64_t npix, int64_t nzones, const uint64_t *offsets_dev, uint64_t *cursors_dev, float *const out[3], void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!zone_args_ok(zones, zone_bytes, npix, nzones) || !planes || !out || !offsets_dev || !cursors_dev || !index_mask || (index_mask & ~LARS_MASK_ALL))
        return fail(LARS_ERR_INVALID, "lars_d_zone_scatter: bad arguments (labels of 1, 2 or 4 bytes, 1 to %d zones, a non-empty index mask)", LARS_ZONES_MAX);
    ScatterParams P;
    memset(&P, 0, sizeof P);
    for (int k = 0; k < 3; ++k) {
        if (!((index_mask >> k) & 1u)) continue;
        if (!planes[k] || !out[k]) return fail(LARS_ERR_INVALID, "lars_d_zone_scatter: index %d needs planes[%d] and out[%d]", k, k, k);
        P.plane[k] = planes[k];
        P.out[k] = out[k];
    }
    P.valid = valid; P.npix = npix; P.nzones = (unsigned int)nzones;
    P.ends = reinterpret_cast<const unsigned long long *>(offsets_dev);
    P.cursors = reinterpret_cast<unsigned long long *>(cursors_dev);
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(cursors_dev, 0, (size_t)(nzones + 1) * sizeof(uint64_t), s));
    const dim3 grid(grid_1d(npix)), block(256);
    if (zone_bytes == 1) hipLaunchKernelGGL((k_zone_scatter<uint8_t>), grid, block, 0, s, static_cast<const uint8_t *>(zones), P);
    else if (zone_bytes == 2) hipLaunchKernelGGL((k_zone_scatter<uint16_t>), grid, block, 0, s, static_cast<const uint16_t *>(zones), P);
    else hipLaunchKernelGGL((k_zone_scatter<int32_t>), grid, block, 0, s, static_cast<const int32_t *>(zones), P);
    return launch_check("lars_d_zone_scatter");
}

extern "C" int lars_d_zone_stats(const float *values, const uint64_t *offsets_dev, const uint64_t *counts_dev, int64_t nzones, float threshold,
                                 int want_hist, int64_t split_pixels, lars_stats *stats_dev, float *medians_dev, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!values || !offsets_dev || !counts_dev || !stats_dev || !medians_dev || nzones < 1 || nzones > LARS_ZONES_MAX || split_pixels < 1)
        return fail(LARS_ERR_INVALID, "lars_d_zone_stats: bad arguments (1 to %d zones, split_pixels >= 1)", LARS_ZONES_MAX);
    const unsigned int nb = nzones < 4096 ? (unsigned int)nzones : 4096u;
    // the segment of zone z is offsets[z - 1] .. offsets[z] - 1, so its size is counts[z]: the kernel reads the offsets alone
    hipLaunchKernelGGL(k_zone_stats, dim3(nb), dim3(256), 0, pick_stream(c, stream), values, reinterpret_cast<const unsigned long long *>(offsets_dev),
                       (unsigned int)nzones, threshold, want_hist, (unsigned long long)split_pixels, stats_dev, medians_dev);
    return launch_check("lars_d_zone_stats");
}
