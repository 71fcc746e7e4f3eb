// Nodata-aware processing of one image (DESIGN.md "Nodata-aware processing"): which pixels are picture, the channel
// histograms of those pixels only, and the fused pass that leaves zeros / NaN / transparent pixels everywhere else and
// hands the valid index values to the array statistics as one compacted stream per index.
//
// Reference semantics: the functions of fused.hip (process-images.py:424-447, :449-490, :492-513, :695, process-ndvi.py:97)
// run on the picture that holds only the valid pixels, img[valid][None, :, :], and scattered back.  What stands outside is
// numpy.ma's: masked samples take no part in np.percentile / mean / median / min / max / histogram, and matplotlib paints
// them with Colormap.set_bad's default (0, 0, 0, 0).
//
// All three kernels walk the image the same way: a lane takes four consecutive pixels (one 4-byte word of the mask, 12 or 16
// bytes of a 3- or 4-channel uint8 image in dword loads, 16-byte stores into the planes), a grid-stride loop takes the
// quads, and the npix % 4 pixels after the last quad are done one per lane by the first workgroup.  Images of other channel
// counts, uint16 images and image pointers that are not 4- / 16-byte aligned read their samples one by one.
//
// Built with -ffp-contract=off like fused.hip: the per-pixel arithmetic is fused_device.h's.
#include <string.h>

#include "common.h"
#include "device_common.h"
#include "fused_device.h"

namespace lars {

namespace {

struct Quad {
    unsigned int r[4], g[4], n[4], a[4];              // a: channel 3, or 1 where the image has none
};

// CF: 3 / 4 = uint8 image of that many channels behind an aligned pointer (dword loads); 0 = anything else
template <typename PIX, int CF>
__device__ inline void load_quad(const PIX *__restrict__ img, long long q, int C, Quad &p)
{
    if (CF == 3) {
        const unsigned int *w = reinterpret_cast<const unsigned int *>(reinterpret_cast<const uint8_t *>(img) + q * 12);
        const unsigned int w0 = w[0], w1 = w[1], w2 = w[2];
        // bytes: r0 g0 n0 r1 | g1 n1 r2 g2 | n2 r3 g3 n3
        p.r[0] = w0 & 0xFF; p.g[0] = (w0 >> 8) & 0xFF; p.n[0] = (w0 >> 16) & 0xFF;
        p.r[1] = w0 >> 24; p.g[1] = w1 & 0xFF; p.n[1] = (w1 >> 8) & 0xFF;
        p.r[2] = (w1 >> 16) & 0xFF; p.g[2] = w1 >> 24; p.n[2] = w2 & 0xFF;
        p.r[3] = (w2 >> 8) & 0xFF; p.g[3] = (w2 >> 16) & 0xFF; p.n[3] = w2 >> 24;
        p.a[0] = p.a[1] = p.a[2] = p.a[3] = 1u;
    } else if (CF == 4) {
        const fu32x4 w = *reinterpret_cast<const fu32x4 *>(reinterpret_cast<const uint8_t *>(img) + q * 16);
        for (int j = 0; j < 4; ++j) {
            p.r[j] = w[j] & 0xFF; p.g[j] = (w[j] >> 8) & 0xFF; p.n[j] = (w[j] >> 16) & 0xFF; p.a[j] = w[j] >> 24;
        }
    } else {
        for (int j = 0; j < 4; ++j) {
            const PIX *s = img + (q * 4 + j) * C;
            p.r[j] = s[0]; p.g[j] = s[1]; p.n[j] = s[2]; p.a[j] = C > 3 ? (unsigned int)s[3] : 1u;
        }
    }
}

__device__ inline unsigned int derive_valid(unsigned int r, unsigned int g, unsigned int n, unsigned int a, unsigned int user,
                                            int use_alpha, int has_nodata, unsigned int nodata)
{
    bool v = user != 0u;
    if (use_alpha) v = v && a != 0u;
    if (has_nodata) v = v && !(r == nodata && g == nodata && n == nodata);
    return v ? 1u : 0u;
}

// ===========================================================================
// 1. validity: one byte per pixel (1 = picture) and |V|
// ===========================================================================
// user may be null (every pixel allowed) and may be `out` itself: a lane reads its word before it writes it
template <typename PIX, int CF>
__global__ __launch_bounds__(256) void k_valid_mask(const PIX *__restrict__ img, long long npix, int C, const uint8_t *user,
                                                    int use_alpha, int has_nodata, unsigned int nodata, uint8_t *out,
                                                    unsigned long long *__restrict__ count)
{
    __shared__ unsigned int s_count;
    const int tid = threadIdx.x;
    if (tid == 0) s_count = 0;
    __syncthreads();
    const long long nquads = npix >> 2;
    unsigned int mine = 0;
    for (long long q = (long long)blockIdx.x * 256 + tid; q < nquads; q += (long long)gridDim.x * 256) {
        Quad p;
        load_quad<PIX, CF>(img, q, C, p);
        const unsigned int u = user ? reinterpret_cast<const unsigned int *>(user)[q] : 0x01010101u;
        unsigned int word = 0;
        for (int j = 0; j < 4; ++j)
            word |= derive_valid(p.r[j], p.g[j], p.n[j], p.a[j], (u >> (8 * j)) & 0xFFu, use_alpha, has_nodata, nodata) << (8 * j);
        reinterpret_cast<unsigned int *>(out)[q] = word;
        mine += __builtin_popcount(word);
    }
    if (blockIdx.x == 0 && tid < (int)(npix & 3)) {
        const long long i = nquads * 4 + tid;
        const PIX *s = img + i * C;
        const unsigned int v = derive_valid(s[0], s[1], s[2], C > 3 ? (unsigned int)s[3] : 1u, user ? user[i] : 1u, use_alpha,
                                            has_nodata, nodata);
        out[i] = (uint8_t)v;
        mine += v;
    }
    // wave reduction, one LDS add per wave, one global atomic per workgroup
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0 && s_count) atomicAdd(count, (unsigned long long)s_count);
}

// ===========================================================================
// 2. channel histograms of the valid pixels (pre-pass of np.percentile, process-images.py:437)
// ===========================================================================
// uint8: one private [3][256] copy per wave in LDS, as k_chan_hist_u8c3 keeps them.  uint16: 3 x 65536 counters do not fit
// a workgroup's LDS share four times over, and one image spreads its samples over so many of them that global atomics hardly
// collide: they go straight to the [3][65536] table in memory.
template <typename PIX, int NVAL, int CF>
__global__ __launch_bounds__(256) void k_masked_hist(const PIX *__restrict__ img, long long npix, int C,
                                                     const uint8_t *__restrict__ valid, unsigned int *__restrict__ hist)
{
    __shared__ unsigned int s_h[NVAL == 256 ? 4 * 768 : 1];
    const int tid = threadIdx.x;
    if (NVAL == 256) {
        for (int i = tid; i < 4 * 768; i += 256) s_h[i] = 0;
        __syncthreads();
    }
    unsigned int *h = NVAL == 256 ? s_h + (tid >> 6) * 768 : hist;
    const long long nquads = npix >> 2;
    for (long long q = (long long)blockIdx.x * 256 + tid; q < nquads; q += (long long)gridDim.x * 256) {
        const unsigned int m = reinterpret_cast<const unsigned int *>(valid)[q];
        if (!m) continue;
        Quad p;
        load_quad<PIX, CF>(img, q, C, p);
        for (int j = 0; j < 4; ++j)
            if ((m >> (8 * j)) & 0xFFu) {
                atomicAdd(&h[p.r[j]], 1u);
                atomicAdd(&h[NVAL + p.g[j]], 1u);
                atomicAdd(&h[2 * NVAL + p.n[j]], 1u);
            }
    }
    if (blockIdx.x == 0 && tid < (int)(npix & 3)) {
        const long long i = nquads * 4 + tid;
        if (valid[i]) {
            const PIX *s = img + i * C;
            atomicAdd(&h[(unsigned int)s[0]], 1u);
            atomicAdd(&h[NVAL + (unsigned int)s[1]], 1u);
            atomicAdd(&h[2 * NVAL + (unsigned int)s[2]], 1u);
        }
    }
    if (NVAL == 256) {
        __syncthreads();
        for (int i = tid; i < 768; i += 256) {
            const unsigned int v = s_h[i] + s_h[768 + i] + s_h[2 * 768 + i] + s_h[3 * 768 + i];
            if (v) atomicAdd(&hist[i], v);
        }
    }
}

// ===========================================================================
// 3. the fused pass
// ===========================================================================
struct MaskedParams {
    const void *img;
    const uint8_t *valid;
    long long npix;
    int channels;
    const uint8_t *wb_table;       // [3][NVAL] (the head of the uint16 blob) or null: indices of the raw samples
    unsigned int mask;
    float *out_index[3];
    uint8_t *out_wb;
    unsigned int *out_rgba[3];
    const unsigned int *cmap_lut[3];
    float *compact[3];             // the valid values of each index, in any order, or null
    unsigned long long *cursor;    // values handed out so far: one counter serves every index, their valid pixels are the same
};

#define LARS_QUIET_NAN_BITS 0x7FC00000u

struct PixelOut {
    unsigned int wb;               // r | g << 8 | n << 16 of the corrected pixel (0 outside)
    float x[3];
    unsigned int rgba[3];
};

// tab: the white-balance table the lanes look up (uint8: the workgroup's copy in LDS; uint16: the 192 KiB table in memory) or null
template <int NVAL>
__device__ inline void masked_pixel(const MaskedParams &P, const uint8_t *tab, unsigned int r, unsigned int g, unsigned int n, bool valid,
                                    PixelOut &o)
{
    const float nan = __builtin_bit_cast(float, LARS_QUIET_NAN_BITS);
    o.wb = 0u;
    o.x[0] = o.x[1] = o.x[2] = nan;
    o.rgba[0] = o.rgba[1] = o.rgba[2] = 0u;       // Colormap.set_bad's default
    if (!valid) return;
    if (tab) {
        r = tab[r]; g = tab[NVAL + g]; n = tab[2 * NVAL + n];
        o.wb = r | (g << 8) | (n << 16);
    }
    // pixel_math's values (fused_device.h) without its accumulators: the statistics come from the compacted values
    if (P.mask & 1u) o.x[0] = norm_diff((float)n, (float)r);
    if (P.mask & 6u) {
        const float gq = norm_diff((float)n, (float)g);
        o.x[1] = gq;
        o.x[2] = 0.0f - gq;        // (g-n)/(g+n) == -(n-g)/(n+g) bit for bit, and +0.0 where the quotient is zero
    }
    for (int k = 0; k < 3; ++k)
        if (((P.mask >> k) & 1u) && P.cmap_lut[k]) o.rgba[k] = P.cmap_lut[k][cmap_index(o.x[k])];
}

template <typename PIX, int NVAL, int CF>
__global__ __launch_bounds__(256) void k_masked_fused(MaskedParams P)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const long long npix = P.npix;
    const int C = P.channels;
    const PIX *img = static_cast<const PIX *>(P.img);
    const long long nquads = npix >> 2;
    const bool compacting = P.compact[0] || P.compact[1] || P.compact[2];
    const unsigned long long below = (1ull << lane) - 1ull;

    __shared__ uint8_t s_tab[NVAL == 256 ? 768 : 4];
    const uint8_t *tab = P.wb_table;
    if (NVAL == 256 && P.wb_table) {                  // wave-uniform: every lane reaches the barrier or none does
        for (int i = tid; i < 768; i += 256) s_tab[i] = P.wb_table[i];
        __syncthreads();
        tab = s_tab;
    }

    // every lane of a wave stays in the loop until the wave's last quad is done: the ballots below need them all
    const long long first = (long long)blockIdx.x * 256 + (tid & ~63);
    for (long long q0 = first; q0 < nquads; q0 += (long long)gridDim.x * 256) {
        const long long q = q0 + lane;
        const bool live = q < nquads;
        unsigned int m = 0;
        PixelOut o[4];
        if (live) {
            m = reinterpret_cast<const unsigned int *>(P.valid)[q];
            Quad p;
            if (m) load_quad<PIX, CF>(img, q, C, p);
            else for (int j = 0; j < 4; ++j) p.r[j] = p.g[j] = p.n[j] = p.a[j] = 0u;
            for (int j = 0; j < 4; ++j) masked_pixel<NVAL>(P, tab, p.r[j], p.g[j], p.n[j], (m >> (8 * j)) & 0xFFu, o[j]);
            if (P.out_wb) {
                uint8_t *w = P.out_wb + q * 4 * C;
                if (CF == 3) {
                    unsigned int *d = reinterpret_cast<unsigned int *>(w);
                    d[0] = o[0].wb | (o[1].wb << 24);
                    d[1] = (o[1].wb >> 8) | (o[2].wb << 16);
                    d[2] = (o[2].wb >> 16) | (o[3].wb << 8);
                } else if (CF == 4) {
                    const fu32x4 d = {o[0].wb, o[1].wb, o[2].wb, o[3].wb};      // channel 3 is zero: zeros_like, process-images.py:432
                    *reinterpret_cast<fu32x4 *>(w) = d;
                } else {
                    for (int j = 0; j < 4; ++j) {
                        uint8_t *d = w + j * C;
                        d[0] = (uint8_t)o[j].wb; d[1] = (uint8_t)(o[j].wb >> 8); d[2] = (uint8_t)(o[j].wb >> 16);
                        for (int c = 3; c < C; ++c) d[c] = 0;
                    }
                }
            }
            for (int k = 0; k < 3; ++k) {
                if (!((P.mask >> k) & 1u)) continue;
                if (P.out_index[k]) {
                    const float v[4] = {o[0].x[k], o[1].x[k], o[2].x[k], o[3].x[k]};
                    store_plane4(P.out_index[k] + q * 4, v, false);
                }
                if (P.out_rgba[k]) {
                    const fu32x4 d = {o[0].rgba[k], o[1].rgba[k], o[2].rgba[k], o[3].rgba[k]};
                    *reinterpret_cast<fu32x4 *>(P.out_rgba[k] + q * 4) = d;
                }
            }
        }
        if (compacting) {
            // wave-aggregated allocation: the wave counts its valid pixels, one lane moves the cursor once, and each pixel's
            // slot is the number of valid pixels in front of it in the wave (pixel j of every lane before pixel j + 1)
            unsigned int before[4], total = 0;
            for (int j = 0; j < 4; ++j) {
                const unsigned long long b = __ballot(((m >> (8 * j)) & 0xFFu) != 0u);
                before[j] = total + (unsigned int)__builtin_popcountll(b & below);
                total += (unsigned int)__builtin_popcountll(b);
            }
            if (total) {
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(P.cursor, (unsigned long long)total);
                base = __shfl(base, 0, 64);
                for (int j = 0; j < 4; ++j) {
                    if (!((m >> (8 * j)) & 0xFFu)) continue;
                    for (int k = 0; k < 3; ++k)
                        if (((P.mask >> k) & 1u) && P.compact[k]) P.compact[k][base + before[j]] = o[j].x[k];
                }
            }
        }
    }
    if (blockIdx.x == 0 && tid < (int)(npix & 3)) {
        const long long i = nquads * 4 + tid;
        const bool v = P.valid[i] != 0;
        const PIX *s = img + i * C;
        PixelOut o;
        masked_pixel<NVAL>(P, tab, v ? (unsigned int)s[0] : 0u, v ? (unsigned int)s[1] : 0u, v ? (unsigned int)s[2] : 0u, v, o);
        if (P.out_wb) {
            uint8_t *d = P.out_wb + i * C;
            d[0] = (uint8_t)o.wb; d[1] = (uint8_t)(o.wb >> 8); d[2] = (uint8_t)(o.wb >> 16);
            for (int c = 3; c < C; ++c) d[c] = 0;
        }
        unsigned long long slot = 0;
        if (v && compacting) slot = atomicAdd(P.cursor, 1ull);
        for (int k = 0; k < 3; ++k) {
            if (!((P.mask >> k) & 1u)) continue;
            if (P.out_index[k]) P.out_index[k][i] = o.x[k];
            if (P.out_rgba[k]) P.out_rgba[k][i] = o.rgba[k];
            if (v && P.compact[k]) P.compact[k][slot] = o.x[k];
        }
    }
}

// 3 / 4: a uint8 image of that many channels whose pointer allows the dword loads; 0: sample by sample
int channel_form(const void *img, int channels, int dtype)
{
    if (dtype != LARS_U8) return 0;
    if (channels == 3 && aligned_to(img, 4)) return 3;
    if (channels == 4 && aligned_to(img, 16)) return 4;
    return 0;
}

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" int lars_d_valid_mask(const void *img, int64_t npix, int channels, int dtype, const uint8_t *user_valid, int use_alpha,
                                 int has_nodata, int nodata, uint8_t *out_mask, uint64_t *count_dev, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out_mask || !count_dev || npix <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "lars_d_valid_mask: bad arguments");
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "lars_d_valid_mask: dtype must be LARS_U8 or LARS_U16");
    if (use_alpha && channels < 4) return fail(LARS_ERR_INVALID, "lars_d_valid_mask: the alpha rule needs 4 or more channels, got %d", channels);
    if (has_nodata && (nodata < 0 || nodata > (dtype == LARS_U8 ? 255 : 65535)))
        return fail(LARS_ERR_INVALID, "lars_d_valid_mask: nodata %d is outside the sample type's range", nodata);
    if (!aligned_to(out_mask, 4) || (user_valid && !aligned_to(user_valid, 4)) || !aligned_to(count_dev, 8))
        return fail(LARS_ERR_INVALID, "lars_d_valid_mask: the masks must be 4-byte aligned, the counter 8-byte aligned");
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(uint64_t), s));
    const dim3 grid(grid_1d(npix >> 2)), block(256);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(count_dev);
    const unsigned int nd = (unsigned int)nodata;
    const int form = channel_form(img, channels, dtype);
    if (form == 3)
        hipLaunchKernelGGL((k_valid_mask<uint8_t, 3>), grid, block, 0, s, static_cast<const uint8_t *>(img), (long long)npix, channels,
                           user_valid, use_alpha, has_nodata, nd, out_mask, cnt);
    else if (form == 4)
        hipLaunchKernelGGL((k_valid_mask<uint8_t, 4>), grid, block, 0, s, static_cast<const uint8_t *>(img), (long long)npix, channels,
                           user_valid, use_alpha, has_nodata, nd, out_mask, cnt);
    else if (dtype == LARS_U8)
        hipLaunchKernelGGL((k_valid_mask<uint8_t, 0>), grid, block, 0, s, static_cast<const uint8_t *>(img), (long long)npix, channels,
                           user_valid, use_alpha, has_nodata, nd, out_mask, cnt);
    else
        hipLaunchKernelGGL((k_valid_mask<uint16_t, 0>), grid, block, 0, s, static_cast<const uint16_t *>(img), (long long)npix, channels,
                           user_valid, use_alpha, has_nodata, nd, out_mask, cnt);
    return launch_check("lars_d_valid_mask");
}

extern "C" int lars_d_masked_channel_hist(const void *img, int64_t npix, int channels, int dtype, const uint8_t *valid,
                                          uint32_t *hist, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !valid || !hist || npix <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "lars_d_masked_channel_hist: bad arguments");
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "lars_d_masked_channel_hist: dtype must be LARS_U8 or LARS_U16");
    if (!aligned_to(valid, 4)) return fail(LARS_ERR_INVALID, "lars_d_masked_channel_hist: the mask must be 4-byte aligned");
    hipStream_t s = pick_stream(c, stream);
    const int nval = dtype == LARS_U8 ? 256 : 65536;
    LARS_HIP_TRY(hipMemsetAsync(hist, 0, (size_t)3 * nval * sizeof(uint32_t), s));
    const dim3 grid(grid_1d(npix >> 2)), block(256);
    const int form = channel_form(img, channels, dtype);
    if (form == 3)
        hipLaunchKernelGGL((k_masked_hist<uint8_t, 256, 3>), grid, block, 0, s, static_cast<const uint8_t *>(img), (long long)npix, channels, valid, hist);
    else if (form == 4)
        hipLaunchKernelGGL((k_masked_hist<uint8_t, 256, 4>), grid, block, 0, s, static_cast<const uint8_t *>(img), (long long)npix, channels, valid, hist);
    else if (dtype == LARS_U8)
        hipLaunchKernelGGL((k_masked_hist<uint8_t, 256, 0>), grid, block, 0, s, static_cast<const uint8_t *>(img), (long long)npix, channels, valid, hist);
    else
        hipLaunchKernelGGL((k_masked_hist<uint16_t, 65536, 0>), grid, block, 0, s, static_cast<const uint16_t *>(img), (long long)npix, channels, valid,
                           hist);
    return launch_check("lars_d_masked_channel_hist");
}

extern "C" int lars_d_masked_fused(const lars_fused_args *a, const uint8_t *valid, float *const compact[3], uint64_t *cursor_dev)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!a || !a->tiles || !valid || a->npix <= 0 || a->channels < 3) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: bad arguments");
    if (a->ntiles != 1) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: one image per call (ntiles == 1)");
    if (a->dtype != LARS_U8 && a->dtype != LARS_U16) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: dtype must be LARS_U8 or LARS_U16");
    if (a->index_mask & ~LARS_MASK_ALL) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: unknown index bits in mask");
    if (a->stats || a->flags)
        return fail(LARS_ERR_INVALID, "lars_d_masked_fused: no statistics here (lars_d_array_stats_f32 on the compacted values gives them)");
    if (a->out_wb && !a->wb_table) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: out_wb needs wb_table");
    bool compacting = false;
    MaskedParams P;
    memset(&P, 0, sizeof P);
    for (int k = 0; k < 3; ++k) {
        if (!((a->index_mask >> k) & 1u)) continue;
        if (a->out_rgba[k] && !a->cmap_lut[k]) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: out_rgba[%d] needs cmap_lut[%d]", k, k);
        if ((a->out_index[k] && !aligned_to(a->out_index[k], 16)) || (a->out_rgba[k] && !aligned_to(a->out_rgba[k], 16)))
            return fail(LARS_ERR_INVALID, "lars_d_masked_fused: the planes must be 16-byte aligned");
        P.out_index[k] = a->out_index[k];
        P.out_rgba[k] = reinterpret_cast<unsigned int *>(a->out_rgba[k]);
        P.cmap_lut[k] = a->out_rgba[k] ? reinterpret_cast<const unsigned int *>(a->cmap_lut[k]) : nullptr;
        P.compact[k] = compact ? compact[k] : nullptr;
        compacting = compacting || P.compact[k];
    }
    if (compacting && (!cursor_dev || !aligned_to(cursor_dev, 8))) return fail(LARS_ERR_INVALID, "lars_d_masked_fused: compact needs an 8-byte aligned cursor_dev");
    const int form = channel_form(a->tiles, a->channels, a->dtype);
    if (!aligned_to(valid, 4) || (a->out_wb && form && !aligned_to(a->out_wb, 16)))
        return fail(LARS_ERR_INVALID, "lars_d_masked_fused: the mask must be 4-byte, out_wb 16-byte aligned");
    hipStream_t s = pick_stream(c, a->stream);
    if (compacting) LARS_HIP_TRY(hipMemsetAsync(cursor_dev, 0, sizeof(uint64_t), s));
    P.img = a->tiles; P.valid = valid; P.npix = a->npix; P.channels = a->channels; P.wb_table = a->wb_table; P.mask = a->index_mask;
    P.out_wb = a->out_wb; P.cursor = reinterpret_cast<unsigned long long *>(cursor_dev);
    const dim3 grid(grid_1d(a->npix >> 2)), block(256);
    if (form == 3) hipLaunchKernelGGL((k_masked_fused<uint8_t, 256, 3>), grid, block, 0, s, P);
    else if (form == 4) hipLaunchKernelGGL((k_masked_fused<uint8_t, 256, 4>), grid, block, 0, s, P);
    else if (a->dtype == LARS_U8) hipLaunchKernelGGL((k_masked_fused<uint8_t, 256, 0>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((k_masked_fused<uint16_t, 65536, 0>), grid, block, 0, s, P);
    return launch_check("lars_d_masked_fused");
}
