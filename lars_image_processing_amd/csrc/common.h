// Internal helpers shared by the translation units of liblars_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "host_common.h"

namespace lars {

// ---- error plumbing (set_error / fail / LARS_TRY: host_common.h) -----------

#define LARS_HIP_TRY(expr)                                                          \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess)                                                       \
            return ::lars::fail(_e == hipErrorOutOfMemory ? LARS_ERR_OOM : LARS_ERR_HIP, \
                                "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                __FILE__, __LINE__);                                \
    } while (0)

// ---- per-thread context ---------------------------------------------------
struct ThreadCtx {
    int device = -1;           // -1: not initialised yet
    hipStream_t stream = nullptr;
    void *ws = nullptr;        // grow-only device workspace of the host entry points
    size_t ws_bytes = 0;
    void *scratch = nullptr;   // small device scratch of the device entry points
    size_t scratch_bytes = 0;
    void *outline = nullptr;   // the tracer's area of the host entry points that trace outlines (outlines.hip): sized by the edge count,
    size_t outline_bytes = 0;  // which is known only once the labels, which stand in ws, exist
    int64_t u16_win_tiles = 0; // tiles of the last lars_d_wb_prepare if it took the value-window route and nothing has reserved the
                               // scratch since (lars_u16_window_report reads its flags and windows there), else 0
};

int ensure_ctx(ThreadCtx **out);                 // initialises device 0 on first use
int ws_reserve(ThreadCtx *c, size_t bytes);      // grow-only; synchronises when it grows
int scratch_reserve(ThreadCtx *c, size_t bytes);
int outline_reserve(ThreadCtx *c, size_t bytes);

// One allocation cut into buffers.  take<T>(count) gives the next 256-byte aligned stretch of count elements; on a null
// base it only counts.  A plan (a function that lists the buffers of an area once) therefore runs twice: on Carver(nullptr)
// for the size, on the area for the pointers.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *b) : base(static_cast<char *>(b)) {}
    template <typename T>
    T *take(size_t count)
    {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return (off + 255) & ~(size_t)255; }   // the 256-byte aligned end
};

// plan(Carver &) on the calling thread's workspace: sized on a null carver, reserved, then pointed
template <typename Plan>
int ws_plan(ThreadCtx *c, Plan &&plan)
{
    Carver size(nullptr);
    plan(size);
    LARS_TRY(ws_reserve(c, size.bytes() + 256));
    Carver cv(c->ws);
    plan(cv);
    return LARS_OK;
}
inline hipStream_t pick_stream(ThreadCtx *c, void *stream) {
    return stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
}

// ---- device-side shared pieces ---------------------------------------------
// 2^32: the fixed-point scale of the statistics accumulators.
#define LARS_FX_SCALE 4294967296.0
#define LARS_FX_INV (1.0 / 4294967296.0)

// While a fused launch is in flight a lars_stats record is used as its own
// accumulator: sum / sumsq hold int64 fixed point, min / max hold order-
// preserving uint64 keys.  k_stats_finalize converts in place.
struct StatsAccView {
    unsigned long long sum_fx;
    unsigned long long sumsq_fx;
    unsigned long long count;
    unsigned long long above;
    unsigned long long nans;
    unsigned long long min_key;      // f64_key of the running minimum
    unsigned long long max_key;
    double threshold;
    unsigned int index_id;
    unsigned int reserved;
    unsigned long long hist[LARS_HIST_BINS];
};
static_assert(sizeof(StatsAccView) == sizeof(lars_stats), "accumulator view must alias lars_stats");

__host__ __device__ inline unsigned int f32_key(float x) {
    unsigned int b = __builtin_bit_cast(unsigned int, x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float key_f32(unsigned int k) {
    unsigned int b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __builtin_bit_cast(float, b);
}
__host__ __device__ inline unsigned long long f64_key(double x) {
    unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double key_f64(unsigned long long k) {
    unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __builtin_bit_cast(double, b);
}

// numpy.histogram(bins=50, range=(-1,1)) edges: linspace computes
// arange(51) * (2/50) + (-1) in float64, pins the last edge to 1, then casts to
// the sample dtype.
__host__ __device__ inline double hist_edge_f64(int i) {
    return i >= LARS_HIST_BINS ? 1.0 : (double)i * (2.0 / 50.0) + (-1.0);
}

// white-balance table blob of a uint16 tile: [3][65536] uint8 table | uint32 thr[3][260] | double par[3][2]
#define LARS_U16_THR_OFFSET 196608
#define LARS_U16_PAR_OFFSET (196608 + 3 * 260 * 4)
#define LARS_U16_BLOB_BYTES (196608 + 4096)

// launch geometry helpers (host)
int launch_check(const char *what);
void align_release();                            // drops the calling thread's cached FFT plan (lars_shutdown)

// tuning knobs: what each does and its default.  Their names and allowed values: the KNOBS table in runtime.cpp (lars_set_tuning).
struct Tuning {
    int fused_impl = 0;        // generation of the fused kernels: automatic, fused.hip or fused_v2.hip
    int hist_impl = 2;         // generation of the channel-histogram kernel
    int nt_stores = 0;         // non-temporal stores for the float32 planes
    int blocks_per_tile = 0;   // workgroups (chunks) per tile; 0 = automatic
    int load_policy = 0;       // cache policy of the streaming tile loads (stream_load.h): each kernel's measured choice, plain everywhere, or nt everywhere
    int selq_window = 1;       // one-pass medians (select_q.hip): predicted windows, always two passes, or wrong windows (test hook)
    int selq_list_wgs = 0;     // workgroups per launch of the classic select passes over the tiles a window missed (0 = 2048)
    int last_fused_kernel = 0; // read-only: the kernel family lars_d_fused launched last -- 1 k_fused_u8c3, 2 k_fused_v2, 3 uint16, 4 generic, 5 RGBA uint8
    int u16_hist_impl = 5;     // uint16 percentiles (u16.hip): one full pass on value windows (counts below + histograms inside), always two
                               // radix passes, or a test hook (value windows that miss: every tile is flagged and takes the two passes as well)
    int out_stride_planes = 0; // laboratory build (LARS_LAB_LAYOUT) only: k > 1 = the fused kernel steps k x npix from tile to tile in its index planes
    int joint_depth = 6;       // joint.hip: 12-byte loads in flight per lane of the counting kernel
    int joint_win_depth = 15;  // joint_win.hip: loads in flight per lane of the windowed counting kernel (which also sets how often it sweeps)
    int jpeg_subseq_bits = 512;  // jpeg_decode.hip: bits of entropy data per lane of the self-synchronising decode
    int jpeg_last_rounds = 0;  // read-only: rounds of k_jd_pass that decoded anything in the last lars_h_decode_jpeg_u8 / lars_h_thumbnail_jpeg_u8 (+100: k_jd_finish ran)
    int tiff_strip_bytes = 65536;  // tiff_encode.hip: uncompressed bytes of a strip when the caller names no rows_per_strip (Pillow's / libtiff's 64 KiB)
    int deflate_matching = 0;  // png.hip, tiff_encode.hip: the Deflate coder searches each segment for repeats (deflate_lz_device.h) or codes literals only
    int joint_window = 1;      // joint_win.hip: windowed pair tables (one reader per tile chunk) where they fit, never, or test hooks (windows that miss)
    int zone_split_pixels = 131072;  // zonal.hip: a zone with more values than this is left out by k_zone_stats; the host runs the array statistics and the
                               // select over its segment instead (many workgroups for one zone instead of one)
    int wb_predict = 1;        // wb_predict.hip: white-balance tables of uint8 RGNir tiles predicted from a sample and proven while the planes are
                               // written (1), never (0), or test hooks: every prediction one value off (2), the confidence gate always passes (3)
    int wb_predict_sixteenths = 4;   // sixteenths of a tile the predictor samples: 2 (1/8), 3 or 4 (profiles/wb_predict_bench_ab.txt)
    int wb_predict_k = 3;      // a mark is confident when both edges of its bin are this many standard errors away from it
    int wb_predict_min_pixels = 1 << 20;   // smaller tiles always take the exact pass
};
Tuning &tuning();
// Does a kernel whose measured choice is `kernel_default_nt` (profiles/load_policy_kernels.txt) take its tile loads with nt now?
inline bool stream_loads_nt(bool kernel_default_nt)
{
    const int k = tuning().load_policy;
    return k == 0 ? kernel_default_nt : k == 2;
}

struct FusedParams;
#ifndef LARS_V2_STATS_THREADS
#define LARS_V2_STATS_THREADS 1024     // statistics-only second-generation kernels (tools/kbench.py A/B: 512 | 1024)
#endif
#ifndef LARS_V2_STATS_WAVES
#define LARS_V2_STATS_WAVES 8          // waves per SIMD the statistics-only kernels are compiled for (64 VGPRs)
#endif
// Per-tile state of the sampled white-balance tables (wb_predict.hip) as the gated kernels see it; every array starts at the launch's
// first tile.  pred == nullptr: no gate, every tile is served.
enum : int { WB_GATE_REFUSED = 0,      // serve the tiles the predictor refused (right after the prediction)
             WB_GATE_PREDICTED = 1,    // serve the tiles that run on a predicted table (settling them without a verified launch)
             WB_GATE_MISSED = 2 };     // serve the predicted tiles whose counts do not prove the prediction (repair after a verified launch)
struct WbGate {
    const unsigned int *pred = nullptr;     // [tile] 1 = the tile's table is predicted and not yet proven
    const uint8_t *predv = nullptr;         // [tile][8]: the predicted value of channel c's mark k at c * 2 + k
    unsigned int *counts = nullptr;         // [tile][12]: per channel #(x < v_lo), #(x <= v_lo), #(x < v_hi), #(x <= v_hi)
    int mode = WB_GATE_REFUSED;
};
int fused_v2_threads(bool any_out);
void fused_v2_launch(unsigned mask, bool wb, int stats, bool nt, dim3 grid, hipStream_t s, const FusedParams &P);
void chan_hist_v2_launch(const uint8_t *tiles, long long npix, unsigned int *hist, dim3 grid, hipStream_t s, int channels = 3,
                         const WbGate &gate = WbGate());
// fused.hip: the gated exact pass over the 3-channel uint8 tiles of one launch (rows of hist that the gate opens must be zero): channel
// histograms, then percentiles and tables; with stats, the records of the tiles served are put back to their opened state and *missed counts them
void wb_exact_gated_launch(const uint8_t *tiles, long long ntiles, long long npix, unsigned int *hist, uint8_t *table, double *pcts,
                           int rgn_variant, const WbGate &gate, lars_stats *stats, unsigned int stats_mask, unsigned int *missed, hipStream_t s);
// wb_predict.hip: the scratch of a batch cut into its arrays
struct WbPredictScratch {
    unsigned int *head;       // [4]: confident tiles, missed tiles of the last prediction
    unsigned int *pred;       // [ntiles]
    uint8_t *predv;           // [ntiles][8]
    unsigned int *counts;     // [ntiles][12]
    unsigned int *ghist;      // [ntiles][16 groups][768]: the sample's histograms
    size_t bytes;
};
WbPredictScratch wb_predict_carve(void *base, long long ntiles);
int selq_pass_launch(const uint8_t *tiles, const uint8_t *wb_table, long long ntiles, long long npix, int first,
                     const unsigned int bucket[4], unsigned long long *hist, hipStream_t s, unsigned streams);
size_t selq_tile_scratch_bytes(long long ntiles);
int selq_tile_medians_launch(const uint8_t *tiles, const uint8_t *wb_table, long long ntiles, long long npix, float *out_pairs,
                             void *scratch, hipStream_t s, bool first_pass_done, unsigned streams, bool windowed = false);
int selq_tile_prepare(void *scratch, long long ntiles, long long npix, hipStream_t s, unsigned int streams);
unsigned int *selq_tile_hist32(void *scratch, long long ntiles);
void fused_v2_sel_launch(unsigned mask, bool wb, int stats, dim3 grid, hipStream_t s, const FusedParams &P);
// fused.hip: grid sizing and the statistics records' init / finalize kernels, for the other translation units
int blocks_per_tile(long long work_items, long long ntiles, int threads = 256, long long target_total = 8192);
void stats_init_launch(lars_stats *stats, long long nrec, unsigned int mask, hipStream_t s);
void stats_finalize_launch(lars_stats *stats, long long nrec, unsigned int mask, long long npix, hipStream_t s);
int quot_check_launch(unsigned int max_den, unsigned long long *mismatches_dev, unsigned int *first_bad_dev, hipStream_t s);

}  // namespace lars
