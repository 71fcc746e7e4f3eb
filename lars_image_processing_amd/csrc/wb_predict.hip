// White-balance tables of uint8 RGNir tiles from a SAMPLE of each tile.
//
// The exact pre-pass reads every tile a second time for six integers per tile (p2 and p98 of three channels).  Here a
// fraction of the tile (2, 3 or 4 sixteenths, whole 4 KiB segments at hashed positions, one per stratum of the tile) is
// counted into channel histograms; per channel and mark the value v whose bin holds the mark in the sample's CDF is the
// prediction.  A mark is confident when both edges of that bin lie at least k standard errors away from the mark, the
// standard error measured from the spread of the edge CDFs between 16 interleaved groups of segments (correlated imagery:
// a thousand segments are a thousand observations, not a million), never below the binomial figure.  A tile whose six marks
// are confident gets percentiles (double)v and the table k_wb_table would build from them, and is marked predicted; every
// other tile takes the exact pass in the same call (the gated kernels of fused_v2.hip / fused.hip).
//
// A prediction is never trusted: the plane-writing kernel that runs on it counts, over all pixels, how many samples lie
// below and up to each predicted value (k_fused_u8c3, VERIFY), and a tile whose counts do not prove all six percentiles is
// repaired on the exact route before anyone sees it (lars_d_fused_verified).  Every other reader settles the predicted tiles
// with the exact pass first (lars_d_wb_settle).  Results are bit-identical by construction.
#include "common.h"
#include "device_common.h"
#include "wg_device.h"
#include "wb_predict_device.h"

namespace lars {

constexpr int WBP_GROUPS = 16;
constexpr unsigned int WBP_SEG_BYTES = 4096;

__host__ __device__ inline unsigned int wbp_mix(unsigned int x)
{
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}
// Segment of sample i (of nsample) in a tile of nseg segments: a hashed position inside the i-th of nsample strata
__host__ __device__ inline unsigned int wbp_segment(unsigned int tile, unsigned int i, unsigned int nseg, unsigned int nsample)
{
    const unsigned int start = (unsigned int)(((unsigned long long)i * nseg) / nsample);
    const unsigned int end = (unsigned int)(((unsigned long long)(i + 1) * nseg) / nsample);
    return start + wbp_mix(i * 0x9E3779B9u + tile * 0x85EBCA6Bu + 0x1234567u) % (end - start);
}

// One workgroup per (group, tile): group g counts samples g, g + 16, ... into 32 lane-private copies of the three histograms (96 KiB
// of LDS, conflict-free as k_chan_hist_u8c3_v2's) and stores its 768 counts.  Four waves share a segment, a quarter (1 KiB) per wave and
// load; wave (sub, quarter) reads the quarter of samples k = sub + 4 n, n = 0, 1, ...  Byte o of a tile belongs to channel o % 3; 4096,
// 1024 and 16 are all 1 modulo 3.
// The loads of a wave form a ring of WBP_RING, as k_chan_hist_u8c3_v2's: a slot is counted and filled again at once, so that eleven or
// twelve loads stay in flight while the LDS atomics run (the first form issued four, waited for all four and counted them with nothing
// in flight: 4.0 TB/s, profiles/wb_lean_pre_pass_trace.txt).  The segments of a chunk of 48 loads are worked out once, one per lane
// (wbp_segment divides twice), and handed out through v_readlane; a load takes its segment as the scalar offset.  12 divides the loads
// per wave at 2, 3 and 4 sixteenths of a 4096 x 4096 tile (24, 36, 48); what is left over goes one load at a time.
constexpr int WBP_RING = 12;
constexpr int WBP_CHUNK = 48;
template <int POLICY>
__global__ __launch_bounds__(1024) void k_wb_sample_hist(const uint8_t *__restrict__ tiles, long long npix, unsigned int nseg,
                                                         unsigned int nsample, unsigned int *__restrict__ ghist)
{
    __shared__ unsigned int s_h[3 * 256 * 32];             // 96 KiB
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * 256 * 32; i += 1024) s_h[i] = 0;
    __syncthreads();

    const unsigned int tile = blockIdx.y, group = blockIdx.x;
    const uint8_t *base = tiles + (long long)tile * npix * 3;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(base), 0, (int)(nseg * WBP_SEG_BYTES), 0x00020000);
    const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane(tid >> 6), lane = (unsigned int)tid & 63u;    // scalar loop counts
    const unsigned int sub = wave >> 2, quarter = wave & 3u;
    const unsigned int per_group = nsample / WBP_GROUPS;
    const unsigned int nloads = per_group > sub ? (per_group - sub + 3u) / 4u : 0u;      // samples k = sub + 4 n < per_group
    const unsigned int lane_off = ((unsigned int)tid & 31u) << 2;
    const unsigned int voff = quarter * 1024u + lane * 16u;
    // the channel of the lane's first byte is (seg + quarter + lane) % 3: the three rotations of the channel offsets, picked by seg % 3
    const unsigned int pl = (quarter + lane) % 3u;
    const unsigned int o0 = pl * 32768u, o1 = ((pl + 1u) % 3u) * 32768u, o2 = ((pl + 2u) % 3u) * 32768u;
    char *hb = reinterpret_cast<char *>(s_h);
#define WBP_ADD(word, shift, choff)                                                                     \
    atomicAdd(reinterpret_cast<unsigned int *>(hb + (choff) + ((((word) >> (shift)) & 0xFFu) << 7) + lane_off), 1u)
    auto count = [&](const sl_u32x4 &w, unsigned int seg) {                             // seg: uniform over the wave
        const unsigned int s3 = seg % 3u;
        const unsigned int c0 = s3 == 0u ? o0 : s3 == 1u ? o1 : o2, c1 = s3 == 0u ? o1 : s3 == 1u ? o2 : o0,
                           c2 = s3 == 0u ? o2 : s3 == 1u ? o0 : o1;
        WBP_ADD(w.x, 0, c0); WBP_ADD(w.x, 8, c1); WBP_ADD(w.x, 16, c2); WBP_ADD(w.x, 24, c0);
        WBP_ADD(w.y, 0, c1); WBP_ADD(w.y, 8, c2); WBP_ADD(w.y, 16, c0); WBP_ADD(w.y, 24, c1);
        WBP_ADD(w.z, 0, c2); WBP_ADD(w.z, 8, c0); WBP_ADD(w.z, 16, c1); WBP_ADD(w.z, 24, c2);
        WBP_ADD(w.w, 0, c0); WBP_ADD(w.w, 8, c1); WBP_ADD(w.w, 16, c2); WBP_ADD(w.w, 24, c0);
    };
    for (unsigned int cb = 0; cb < nloads; cb += (unsigned int)WBP_CHUNK) {
        const unsigned int cn = nloads - cb < (unsigned int)WBP_CHUNK ? nloads - cb : (unsigned int)WBP_CHUNK;
        // lane l: the segment of the chunk's load l
        unsigned int segv = 0u;
        if (lane < cn) segv = wbp_segment(tile, (sub + 4u * (cb + lane)) * WBP_GROUPS + group, nseg, nsample);
        auto seg_of = [&](unsigned int i) {                                             // i < cn, uniform
            return (unsigned int)__builtin_amdgcn_readlane((int)segv, (int)i);
        };
        const unsigned int rounds = cn / (unsigned int)WBP_RING;
        if (rounds > 0u) {
            sl_u32x4 w[WBP_RING];
#pragma unroll
            for (int j = 0; j < WBP_RING; ++j) w[j] = stream_load_b128<POLICY>(rsrc, voff, seg_of((unsigned int)j) * WBP_SEG_BYTES);
            for (unsigned int r = 0; r + 1u < rounds; ++r) {
#pragma unroll
                for (int j = 0; j < WBP_RING; ++j) {
                    count(w[j], seg_of(r * (unsigned int)WBP_RING + (unsigned int)j));
                    __builtin_amdgcn_sched_barrier(0);
                    w[j] = stream_load_b128<POLICY>(rsrc, voff, seg_of((r + 1u) * (unsigned int)WBP_RING + (unsigned int)j) * WBP_SEG_BYTES);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int j = 0; j < WBP_RING; ++j) {
                count(w[j], seg_of((rounds - 1u) * (unsigned int)WBP_RING + (unsigned int)j));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        for (unsigned int i = rounds * (unsigned int)WBP_RING; i < cn; ++i) {
            const unsigned int seg = seg_of(i);
            count(stream_load_b128<POLICY>(rsrc, voff, seg * WBP_SEG_BYTES), seg);
        }
    }
#undef WBP_ADD
    __syncthreads();
    if (tid < 768) {
        const unsigned int *row = s_h + tid * 32;
        unsigned int v = 0;
        for (int j = 0; j < 32; ++j) v += row[(j + tid) & 31];
        ghist[((long long)tile * WBP_GROUPS + group) * 768 + tid] = v;
    }
}

// One workgroup of 256 threads per tile: pooled histogram -> six predicted values -> the twelve edge CDFs of every group -> confidence.
// hook: tuning().wb_predict (2: every prediction one value off; 3: the gate always passes).
__global__ __launch_bounds__(256) void k_wb_decide(const unsigned int *__restrict__ ghist, int kk, int hook, int rgn_variant,
                                                   unsigned int *__restrict__ head, unsigned int *__restrict__ pred,
                                                   uint8_t *__restrict__ predv, unsigned int *__restrict__ counts,
                                                   uint8_t *__restrict__ table, double *__restrict__ pcts)
{
    __shared__ unsigned int s_g[WBP_GROUPS][768];          // 48 KiB
    __shared__ unsigned int s_scan[4];
    __shared__ unsigned int s_v[6], s_before[6], s_bin[6], s_n[3];
    __shared__ double s_f[12][WBP_GROUPS];
    __shared__ int s_ok[12];
    __shared__ int s_conf;
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x;
    const unsigned int *g = ghist + tile * WBP_GROUPS * 768;
    for (int i = tid; i < WBP_GROUPS * 768; i += 256) (&s_g[0][0])[i] = g[i];
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
        unsigned int local = 0;
        for (int j = 0; j < WBP_GROUPS; ++j) local += s_g[j][c * 256 + tid];
        unsigned int total = 0;
        const unsigned int before = wg_exscan<256>(local, s_scan, &total);
        if (tid == 0) s_n[c] = total;
        for (int k = 0; k < 2; ++k) {
            long long lo, hi;
            double t;
            wb_mark_ranks(total ? (long long)total : 1, k, lo, hi, t);
            if (local && (unsigned long long)lo >= before && (unsigned long long)lo < (unsigned long long)before + local) {
                s_v[c * 2 + k] = (unsigned int)tid; s_before[c * 2 + k] = before; s_bin[c * 2 + k] = local;
            }
        }
    }
    __syncthreads();
    // thread (mark m, edge e, group j): the group's CDF at the edge -- below v (e = 0) or up to v (e = 1)
    if (tid < 12 * WBP_GROUPS) {
        const int m = tid / (2 * WBP_GROUPS), e = (tid / WBP_GROUPS) & 1, j = tid % WBP_GROUPS, c = m >> 1;
        const unsigned int *h = &s_g[j][c * 256];
        const unsigned int end = s_n[c] ? s_v[m] + (unsigned int)e : 0u;
        unsigned int cum = 0, all = 0;
        for (unsigned int b = 0; b < 256u; ++b) {
            const unsigned int x = h[(b + (unsigned int)j * 8u) & 255u];            // rotated start keeps the groups' banks apart
            all += x;
            cum += ((b + (unsigned int)j * 8u) & 255u) < end ? x : 0u;
        }
        s_f[m * 2 + e][j] = all ? (double)cum / (double)all : -1.0;
    }
    __syncthreads();
    if (tid < 12) {
        const int m = tid >> 1, e = tid & 1, c = m >> 1;
        const double q = ((m & 1) == 0 ? 2.0 : 98.0) / 100.0;
        bool ok = s_n[c] != 0u;
        double mean = 0.0;
        for (int j = 0; j < WBP_GROUPS; ++j) { ok = ok && s_f[tid][j] >= 0.0; mean += s_f[tid][j]; }
        mean /= WBP_GROUPS;
        double ss = 0.0;
        for (int j = 0; j < WBP_GROUPS; ++j) ss += (s_f[tid][j] - mean) * (s_f[tid][j] - mean);
        if (ok) {
            const double n = (double)s_n[c];
            double se = sqrt(ss / (double)(WBP_GROUPS * (WBP_GROUPS - 1)));
            const double floor_se = sqrt(q * (1.0 - q) / n);
            if (se < floor_se) se = floor_se;
            const double f = ((double)s_before[m] + (e ? (double)s_bin[m] : 0.0)) / n;      // the pooled CDF at the edge
            const double margin = e ? f - q : q - f;
            // no sample can lie below 0 or above 255: those edges cannot be crossed
            ok = (e == 0 && s_v[m] == 0u) || (e == 1 && s_v[m] == 255u) || margin >= (double)kk * se;
        }
        s_ok[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        bool conf = s_n[0] && s_n[1] && s_n[2];
        for (int i = 0; i < 12; ++i) conf = conf && (s_ok[i] || hook == 3);
        if (conf && hook == 2)
            for (int m = 0; m < 6; ++m) s_v[m] = s_v[m] < 255u ? s_v[m] + 1u : 254u;
        s_conf = conf ? 1 : 0;
        pred[tile] = conf ? 1u : 0u;
        if (conf) atomicAdd(&head[0], 1u);
    }
    __syncthreads();
    if (tid < 12) counts[tile * 12 + tid] = 0u;
    if (tid < 8) predv[tile * 8 + tid] = tid < 6 ? (uint8_t)s_v[tid] : (uint8_t)0;
    if (!s_conf) return;
    if (tid < 6) pcts[tile * 6 + tid] = (double)s_v[tid];
    for (int c = 0; c < 3; ++c)
        wb_fill_table_u8(table + (tile * 3 + c) * 256, tid, (double)s_v[c * 2], (double)s_v[c * 2 + 1], rgn_variant);
}

WbPredictScratch wb_predict_carve(void *base, long long ntiles)
{
    Carver cv(base);
    WbPredictScratch p;
    p.head = cv.take<unsigned int>(4);
    p.pred = cv.take<unsigned int>((size_t)ntiles);
    p.predv = cv.take<uint8_t>((size_t)ntiles * 8);
    p.counts = cv.take<unsigned int>((size_t)ntiles * 12);
    p.ghist = cv.take<unsigned int>((size_t)ntiles * WBP_GROUPS * 768);
    p.bytes = cv.bytes();
    return p;
}

// Segments of a tile and of its sample (a multiple of 16, at least one per group); 0 = the tile is too small to sample
static unsigned int wbp_sample_segments(long long npix, unsigned int *nseg_out)
{
    const long long nseg = npix * 3 / WBP_SEG_BYTES;
    *nseg_out = (unsigned int)nseg;
    if (nseg < WBP_GROUPS) return 0;
    long long n = (nseg * tuning().wb_predict_sixteenths / 16 + WBP_GROUPS - 1) / WBP_GROUPS * WBP_GROUPS;
    if (n < WBP_GROUPS) n = WBP_GROUPS;
    if (n > nseg) n = nseg / WBP_GROUPS * WBP_GROUPS;
    return (unsigned int)n;
}

}  // namespace lars

using namespace lars;

extern "C" size_t lars_wb_predict_scratch_bytes(int64_t ntiles)
{
    return ntiles > 0 ? wb_predict_carve(nullptr, ntiles).bytes : 0;
}

extern "C" int lars_d_wb_predict(const void *tiles, int64_t ntiles, int64_t npix, int channels, int dtype, uint32_t *hist, uint8_t *table,
                                 double *percentiles, int rgn_variant, void *scratch, int *predicted, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!tiles || !hist || !table || !percentiles || !scratch || !predicted || ntiles <= 0 || ntiles > 65535 || npix <= 0 || channels < 3 ||
        dtype != LARS_U8)
        return fail(LARS_ERR_INVALID, "lars_d_wb_predict: bad arguments");
    hipStream_t s = pick_stream(c, stream);
    const WbPredictScratch ps = wb_predict_carve(scratch, ntiles);
    unsigned int nseg = 0;
    const unsigned int nsample = wbp_sample_segments(npix, &nseg);
    // what the gated exact pass (k_chan_hist_u8c3_v2) serves, large enough tiles only
    const bool can = tuning().wb_predict != 0 && channels == 3 && (ntiles == 1 || (npix & 3) == 0) &&
                     (reinterpret_cast<uintptr_t>(tiles) & 3) == 0 && (long long)npix * 3 < (1ll << 30) && tuning().hist_impl != 1 &&
                     npix >= tuning().wb_predict_min_pixels && nsample > 0;
    *predicted = can ? 1 : 0;
    // head, pred: nothing confident, nothing missed, nothing predicted
    LARS_HIP_TRY(hipMemsetAsync(ps.head, 0, (size_t)(reinterpret_cast<char *>(ps.predv) - reinterpret_cast<char *>(ps.head)), s));
    if (!can) {
        LARS_TRY(lars_d_channel_hist(tiles, ntiles, npix, channels, dtype, hist, stream));
        return lars_d_wb_table(hist, ntiles, npix, dtype, table, percentiles, rgn_variant, stream);
    }
    LARS_HIP_TRY(hipMemsetAsync(hist, 0, (size_t)ntiles * 768 * sizeof(uint32_t), s));      // a predicted tile's rows stay zero until it is counted
    const dim3 grid(WBP_GROUPS, (unsigned)ntiles);
    if (stream_loads_nt(true))
        hipLaunchKernelGGL((k_wb_sample_hist<LOAD_NT>), grid, dim3(1024), 0, s, static_cast<const uint8_t *>(tiles), (long long)npix, nseg, nsample, ps.ghist);
    else
        hipLaunchKernelGGL((k_wb_sample_hist<LOAD_PLAIN>), grid, dim3(1024), 0, s, static_cast<const uint8_t *>(tiles), (long long)npix, nseg, nsample, ps.ghist);
    hipLaunchKernelGGL(k_wb_decide, dim3((unsigned)ntiles), dim3(256), 0, s, ps.ghist, tuning().wb_predict_k, tuning().wb_predict, rgn_variant,
                       ps.head, ps.pred, ps.predv, ps.counts, table, percentiles);
    WbGate G;
    G.pred = ps.pred; G.predv = ps.predv; G.counts = ps.counts; G.mode = WB_GATE_REFUSED;
    wb_exact_gated_launch(static_cast<const uint8_t *>(tiles), ntiles, npix, hist, table, percentiles, rgn_variant, G, nullptr, 0u, nullptr, s);
    return launch_check("lars_d_wb_predict");
}

extern "C" int lars_d_wb_settle(const void *tiles, int64_t ntiles, int64_t npix, uint32_t *hist, uint8_t *table, double *percentiles,
                                int rgn_variant, void *scratch, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!tiles || !hist || !table || !percentiles || !scratch || ntiles <= 0 || ntiles > 65535 || npix <= 0)
        return fail(LARS_ERR_INVALID, "lars_d_wb_settle: bad arguments");
    hipStream_t s = pick_stream(c, stream);
    const WbPredictScratch ps = wb_predict_carve(scratch, ntiles);
    WbGate G;
    G.pred = ps.pred; G.predv = ps.predv; G.counts = ps.counts; G.mode = WB_GATE_PREDICTED;
    wb_exact_gated_launch(static_cast<const uint8_t *>(tiles), ntiles, npix, hist, table, percentiles, rgn_variant, G, nullptr, 0u, nullptr, s);
    LARS_HIP_TRY(hipMemsetAsync(ps.pred, 0, (size_t)ntiles * sizeof(unsigned int), s));
    return launch_check("lars_d_wb_settle");
}

extern "C" int lars_wb_predict_report(const void *scratch, int64_t ntiles, int64_t *confident, int64_t *missed)
{
    if (!scratch || ntiles <= 0 || !confident || !missed) return fail(LARS_ERR_INVALID, "lars_wb_predict_report: bad arguments");
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    unsigned int head[4] = {0, 0, 0, 0};
    LARS_HIP_TRY(hipMemcpyAsync(head, wb_predict_carve(const_cast<void *>(scratch), ntiles).head, sizeof(head), hipMemcpyDeviceToHost, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    *confident = head[0];
    *missed = head[1];
    return LARS_OK;
}
