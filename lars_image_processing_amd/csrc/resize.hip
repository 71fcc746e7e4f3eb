// LANCZOS down-scale in front of the hot path.
//
// Reference: preprocess_large_image(img_array, max_dimension=1024), process-images.py:398-422:
// PIL.Image.fromarray(img).resize((new_w, new_h), Image.Resampling.LANCZOS).  Pillow's algorithm
// (src/libImaging/Resample.c, 8 bits per channel): float64 weights of the truncated sinc per output
// sample, normalised, rounded to 22-bit fixed point; horizontal integer pass into a uint8
// intermediate, then the vertical pass; accumulators start at 2^21, result clip8(acc >> 22).
// Four-channel images are RGBA to Pillow and are premultiplied by alpha before and divided after
// (Image.resize: RGBA -> RGBa -> resize -> RGBA).
//
// The weights are computed on the host with the same double arithmetic and libm sin() as Pillow
// (-ffp-contract=off); the two passes and the alpha handling run on the GPU in integers, so the
// result is bit-identical to Pillow's (tests/golden/resize_outputs.npz: outputs of the reference).
//
// The gallery thumbnail (Image.thumbnail(size, LANCZOS, reducing_gap), process-images.py:186-189) runs the same passes
// over a fractional float box, after Pillow's integer Image.reduce (k_reduce, Reduce.c); the policy that picks the box,
// the reduce factors and the pass order is host Python (api.thumbnail_plan).
#include <algorithm>
#include <cmath>
#include <vector>

#include "codec_host.h"

namespace lars {

#define RS_PRECISION_BITS (32 - 8 - 2)

__device__ inline uint8_t rs_clip8(int acc)
{
    const int v = acc >> RS_PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one pass along x: in [rows][w_in][C] -> out [rows][w_out][C]
template <int C>
__global__ __launch_bounds__(256) void k_resample_h(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int rows, int w_in,
                                                    int w_out, int ksize, const int *__restrict__ bounds,
                                                    const int *__restrict__ kk)
{
    const long long n = (long long)rows * w_out;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / w_out), xx = (int)(i - (long long)y * w_out);
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const int *k = kk + (long long)xx * ksize;
        const uint8_t *p = in + ((long long)y * w_in + xmin) * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION_BITS - 1);
        for (int x = 0; x < cnt; ++x) {
            const int kv = k[x];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[x * C + c] * kv;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = rs_clip8(acc[c]);
    }
}

// one pass along y: in [h_in][w][C] -> out [h_out][w][C]
template <int C>
__global__ __launch_bounds__(256) void k_resample_v(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int h_in, int h_out,
                                                    int w, int ksize, const int *__restrict__ bounds, const int *__restrict__ kk)
{
    const long long n = (long long)h_out * w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int yy = (int)(i / w), x = (int)(i - (long long)yy * w);
        const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
        const int *k = kk + (long long)yy * ksize;
        const uint8_t *p = in + ((long long)ymin * w + x) * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION_BITS - 1);
        for (int y = 0; y < cnt; ++y) {
            const int kv = k[y];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[(long long)y * w * C + c] * kv;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = rs_clip8(acc[c]);
    }
}

// Pillow Convert.c rgbA2rgba / rgba2rgbA
__global__ __launch_bounds__(256) void k_premultiply_rgba(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, long long npix)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const unsigned int px = reinterpret_cast<const unsigned int *>(in)[i];
        const unsigned int a = px >> 24;
        unsigned int o = px & 0xFF000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned int t = ((px >> (8 * c)) & 0xFFu) * a + 128u;
            o |= ((((t >> 8) + t) >> 8) & 0xFFu) << (8 * c);
        }
        reinterpret_cast<unsigned int *>(out)[i] = o;
    }
}
__global__ __launch_bounds__(256) void k_unpremultiply_rgba(uint8_t *__restrict__ img, long long npix)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const unsigned int px = reinterpret_cast<unsigned int *>(img)[i];
        const unsigned int a = px >> 24;
        if (a == 0u || a == 255u) continue;
        unsigned int o = px & 0xFF000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned int v = (255u * ((px >> (8 * c)) & 0xFFu)) / a;
            v = v > 255u ? 255u : v;
            o |= v << (8 * c);
        }
        reinterpret_cast<unsigned int *>(img)[i] = o;
    }
}

// Resample.c: lanczos_filter / precompute_coeffs / normalize_coeffs_8bpc for the box (in0, in1) of an axis of in_size
// samples.  The box is float, as Pillow's C code holds it: in1 - in0 is a float subtraction.
static double rs_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
static double rs_lanczos(double x)
{
    if (-3.0 <= x && x < 3.0) return rs_sinc(x) * rs_sinc(x / 3);
    return 0.0;
}
static int rs_coeffs(int in_size, float in0, float in1, int out_size, std::vector<int> &bounds, std::vector<int> &kk)
{
    const double scale = (double)(in1 - in0) / out_size;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 3.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    kk.assign((size_t)out_size * ksize, 0);
    std::vector<double> k((size_t)ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = rs_lanczos((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const double v = k[x];
            kk[(size_t)xx * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << RS_PRECISION_BITS)) : (int)(0.5 + v * (1 << RS_PRECISION_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

// The passes of ImagingResampleInner: each runs only where its axis changes (need_h / need_v, Pillow's rule), horizontal
// first, or vertical first for Image.resize's tall-image branch.  Returns the buffer that holds the result (src when
// neither pass runs); tmp holds max(h * nw, nh * w) * C bytes.
template <int C>
static const uint8_t *launch_passes(hipStream_t s, const uint8_t *src, uint8_t *tmp, uint8_t *dst, int h, int w, int nh, int nw,
                                    bool need_h, bool need_v, bool vertical_first, const int *bh, const int *kh, int ksh,
                                    const int *bv, const int *kv, int ksv)
{
    auto grid = [](long long n) { return dim3((unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256)); };
    const uint8_t *cur = src;
    if (vertical_first && need_v) {
        uint8_t *o = need_h ? tmp : dst;
        hipLaunchKernelGGL((k_resample_v<C>), grid((long long)nh * w), dim3(256), 0, s, cur, o, h, nh, w, ksv, bv, kv);
        cur = o;
        h = nh;
    }
    if (need_h) {
        uint8_t *o = need_v && !vertical_first ? tmp : dst;
        hipLaunchKernelGGL((k_resample_h<C>), grid((long long)h * nw), dim3(256), 0, s, cur, o, h, w, nw, ksh, bh, kh);
        cur = o;
        w = nw;
    }
    if (need_v && !vertical_first) {
        hipLaunchKernelGGL((k_resample_v<C>), grid((long long)nh * w), dim3(256), 0, s, cur, dst, h, nh, w, ksv, bv, kv);
        cur = dst;
    }
    return cur;
}

// Reduce.c (ImagingReduce and ImagingReduceCorners, 8 bits per channel) over the box [x0, x0 + bw) x [y0, y0 + bh) of
// in [.][w_in][C]: output cell (ox, oy) = the fx x fy block from (x0 + ox * fx, y0 + oy * fy), clipped to the box (the
// partial cells of the last column and row), out = ((sum + n / 2) * mult) >> 24 in uint32 for the block's n pixels.
// mult = (uint32)(2^32 / (float)(256 n)) depends only on whether the cell is clipped in x, in y or both: the host
// computes the four values in float32 as Pillow does.  Adjacent lanes take adjacent cells of a row, so a wave reads
// one stretch of each source row.
template <int C>
__global__ __launch_bounds__(256) void k_reduce(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int w_in, int x0, int y0,
                                                int bw, int bh, int fx, int fy, int ow, int oh, unsigned int mult_full,
                                                unsigned int mult_x, unsigned int mult_y, unsigned int mult_xy)
{
    const long long n = (long long)oh * ow;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int oy = (int)(i / ow), ox = (int)(i - (long long)oy * ow);
        const int cw = min(fx, bw - ox * fx), ch = min(fy, bh - oy * fy);
        const uint8_t *p = in + ((long long)(y0 + oy * fy) * w_in + x0 + (long long)ox * fx) * C;
        unsigned int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0u;
        for (int y = 0; y < ch; ++y) {
            const uint8_t *row = p + (long long)y * w_in * C;
            for (int x = 0; x < cw; ++x) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += row[x * C + c];
            }
        }
        const bool px = cw < fx, py = ch < fy;
        const unsigned int mult = px ? (py ? mult_xy : mult_x) : (py ? mult_y : mult_full);
        const unsigned int amend = (unsigned int)(cw * ch) / 2u;
#pragma unroll
        for (int c = 0; c < C; ++c) out[i * C + c] = (uint8_t)(((acc[c] + amend) * mult) >> 24);
    }
}

// Reduce.c division_UINT32(n, 8)
static unsigned int rd_mult(long long n)
{
    const float max_int = 4294967296.0f;
    return (unsigned int)(max_int / (float)(unsigned int)(256 * n));
}

template <int C>
static void launch_reduce(hipStream_t s, const uint8_t *in, uint8_t *out, int w_in, const int rb[4], int fx, int fy, int ow, int oh)
{
    const int bw = rb[2] - rb[0], bh = rb[3] - rb[1];
    const int rx = bw % fx, ry = bh % fy;
    const unsigned int m_full = rd_mult((long long)fx * fy), m_x = rd_mult((long long)(rx ? rx : fx) * fy),
                       m_y = rd_mult((long long)fx * (ry ? ry : fy)), m_xy = rd_mult((long long)(rx ? rx : fx) * (ry ? ry : fy));
    const long long n = (long long)ow * oh;
    hipLaunchKernelGGL((k_reduce<C>), dim3((unsigned)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256)), dim3(256), 0, s, in, out, w_in,
                       rb[0], rb[1], bw, bh, fx, fy, ow, oh, m_full, m_x, m_y, m_xy);
}

}  // namespace lars

using namespace lars;

// Image.thumbnail(size, LANCZOS, reducing_gap) of a host uint8 image [h][w][channels] -- process-images.py:186-189, the
// gallery thumbnails -- on the numbers of api.thumbnail_plan: premultiply (channels 4), Image.reduce((fx, fy)) over
// reduce_box, the LANCZOS passes over the float box of the reduced image, un-premultiply.  One upload, one download.
// The body of lars_h_thumbnail_u8 in three steps (codec_host.h): the decoders' thumbnail entry points run the same
// steps on the decoded image, read in place on the device.
int lars::thumbnail_prepare(int64_t h, int64_t w, int channels, int fx, int fy, const int reduce_box[4], const float box[4],
                            int64_t new_h, int64_t new_w, int vertical_first, ThumbJob *Tp)
{
    if (!reduce_box || !box || h <= 0 || w <= 0 || new_h <= 0 || new_w <= 0 || h > (1 << 24) || w > (1 << 24) ||
        new_h > (1 << 24) || new_w > (1 << 24) || fx < 1 || fy < 1 || (long long)fx * fy >= (1 << 24))
        return fail(LARS_ERR_INVALID, "lars_h_thumbnail_u8: bad arguments");
    if (channels != 1 && channels != 3 && channels != 4)
        return fail(LARS_ERR_UNSUPPORTED, "lars_h_thumbnail_u8: 1, 3 or 4 channels (got %d)", channels);
    const int *rb = reduce_box;
    if (rb[0] < 0 || rb[1] < 0 || rb[2] > w || rb[3] > h || rb[2] <= rb[0] || rb[3] <= rb[1])
        return fail(LARS_ERR_INVALID, "lars_h_thumbnail_u8: reduce box (%d, %d, %d, %d) outside the %lld x %lld image", rb[0], rb[1], rb[2],
                    rb[3], (long long)w, (long long)h);
    ThumbJob &T = *Tp;
    T.h = h; T.w = w; T.new_h = new_h; T.new_w = new_w;
    T.channels = channels; T.fx = fx; T.fy = fy;
    for (int k = 0; k < 4; ++k) T.rb[k] = rb[k];
    T.vertical_first = vertical_first != 0;
    T.reduce = fx != 1 || fy != 1 || rb[0] != 0 || rb[1] != 0 || rb[2] != w || rb[3] != h;
    const int rw = T.rw = (rb[2] - rb[0] + fx - 1) / fx, rh = T.rh = (rb[3] - rb[1] + fy - 1) / fy;
    // `!(a < b)` also refuses NaN
    if (!(box[0] >= 0.0f) || !(box[1] >= 0.0f) || !(box[2] <= (float)rw) || !(box[3] <= (float)rh) || !(box[0] < box[2]) ||
        !(box[1] < box[3]))
        return fail(LARS_ERR_INVALID, "lars_h_thumbnail_u8: box outside the %d x %d reduced image", rw, rh);
    // ImagingResampleInner's need_horizontal / need_vertical
    T.need_h = new_w != rw || box[0] != 0.0f || box[2] != (float)new_w;
    T.need_v = new_h != rh || box[1] != 0.0f || box[3] != (float)new_h;
    T.ksh = T.need_h ? rs_coeffs(rw, box[0], box[2], (int)new_w, T.bh, T.kh) : 0;
    T.ksv = T.need_v ? rs_coeffs(rh, box[1], box[3], (int)new_h, T.bv, T.kv) : 0;
    return LARS_OK;
}

ThumbBufs lars::thumbnail_bufs(const ThumbJob &T, bool on_device, Carver &cv)
{
    const size_t C = (size_t)T.channels, in_bytes = (size_t)T.h * T.w * C;
    ThumbBufs B;
    B.in = on_device ? nullptr : cv.take<uint8_t>(in_bytes);     // a device image is read in place: no upload copy
    B.pre = T.channels == 4 ? cv.take<uint8_t>(in_bytes) : nullptr;
    B.red = cv.take<uint8_t>(T.reduce ? (size_t)T.rh * T.rw * C : 0);
    B.tmp = cv.take<uint8_t>(std::max((size_t)T.rh * T.new_w, (size_t)T.new_h * T.rw) * C);
    B.out = cv.take<uint8_t>((size_t)T.new_h * T.new_w * C);
    B.bh = cv.take<int>(T.bh.size());
    B.kh = cv.take<int>(T.kh.size());
    B.bv = cv.take<int>(T.bv.size());
    B.kv = cv.take<int>(T.kv.size());
    cv.take<char>(1024);                                         // the slack this workspace has always ended in
    return B;
}

int lars::thumbnail_run(ThreadCtx *c, const ThumbJob &T, const ThumbBufs &B, const uint8_t *img, bool on_device, uint8_t *out)
{
    const int channels = T.channels, rw = T.rw, rh = T.rh, nw = (int)T.new_w, nh = (int)T.new_h;
    hipStream_t s = c->stream;
    if (!on_device) LARS_HIP_TRY(hipMemcpyAsync(B.in, img, (size_t)T.h * T.w * channels, hipMemcpyHostToDevice, s));
    if (T.need_h) {
        LARS_HIP_TRY(hipMemcpyAsync(B.bh, T.bh.data(), T.bh.size() * 4, hipMemcpyHostToDevice, s));
        LARS_HIP_TRY(hipMemcpyAsync(B.kh, T.kh.data(), T.kh.size() * 4, hipMemcpyHostToDevice, s));
    }
    if (T.need_v) {
        LARS_HIP_TRY(hipMemcpyAsync(B.bv, T.bv.data(), T.bv.size() * 4, hipMemcpyHostToDevice, s));
        LARS_HIP_TRY(hipMemcpyAsync(B.kv, T.kv.data(), T.kv.size() * 4, hipMemcpyHostToDevice, s));
    }
    const uint8_t *cur = on_device ? img : B.in;
    if (channels == 4) {
        const long long npix = (long long)T.h * T.w;
        hipLaunchKernelGGL(k_premultiply_rgba, dim3((unsigned)((npix + 255) / 256 > 8192 ? 8192 : (npix + 255) / 256)), dim3(256), 0, s, cur,
                           B.pre, npix);
        cur = B.pre;
    }
    if (T.reduce) {
        if (channels == 1) launch_reduce<1>(s, cur, B.red, (int)T.w, T.rb, T.fx, T.fy, rw, rh);
        else if (channels == 3) launch_reduce<3>(s, cur, B.red, (int)T.w, T.rb, T.fx, T.fy, rw, rh);
        else launch_reduce<4>(s, cur, B.red, (int)T.w, T.rb, T.fx, T.fy, rw, rh);
        cur = B.red;
    }
    if (channels == 1)
        cur = launch_passes<1>(s, cur, B.tmp, B.out, rh, rw, nh, nw, T.need_h, T.need_v, T.vertical_first, B.bh, B.kh, T.ksh, B.bv, B.kv, T.ksv);
    else if (channels == 3)
        cur = launch_passes<3>(s, cur, B.tmp, B.out, rh, rw, nh, nw, T.need_h, T.need_v, T.vertical_first, B.bh, B.kh, T.ksh, B.bv, B.kv, T.ksv);
    else
        cur = launch_passes<4>(s, cur, B.tmp, B.out, rh, rw, nh, nw, T.need_h, T.need_v, T.vertical_first, B.bh, B.kh, T.ksh, B.bv, B.kv, T.ksv);
    if (channels == 4) {
        // cur is B.pre, B.red, B.tmp or B.out here: never the caller's image
        const long long npix = (long long)nh * nw;
        hipLaunchKernelGGL(k_unpremultiply_rgba, dim3((unsigned)((npix + 255) / 256 > 8192 ? 8192 : (npix + 255) / 256)), dim3(256), 0, s,
                           const_cast<uint8_t *>(cur), npix);
    }
    LARS_TRY(launch_check("lars_h_thumbnail_u8"));
    LARS_HIP_TRY(hipMemcpyAsync(out, cur, (size_t)nh * nw * channels, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

extern "C" int lars_h_thumbnail_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int fx, int fy, const int reduce_box[4],
                                   const float box[4], int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out) return fail(LARS_ERR_INVALID, "lars_h_thumbnail_u8: bad arguments");
    ThumbJob T;
    LARS_TRY(thumbnail_prepare(h, w, channels, fx, fy, reduce_box, box, new_h, new_w, vertical_first, &T));
    ThumbBufs B;
    LARS_TRY(ws_plan(c, [&](Carver &cv) { B = thumbnail_bufs(T, false, cv); }));
    return thumbnail_run(c, T, B, img, false, out);
}

// PIL.Image.resize((new_w, new_h), LANCZOS) of a host uint8 image [h][w][channels], channels 1, 3 or 4
// (4 = RGBA: premultiplied-alpha path) -- the arithmetic of preprocess_large_image, process-images.py:419-420: what
// lars_h_thumbnail_u8 computes with no reduce and the whole image as the box.
extern "C" int lars_h_resize_lanczos_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int64_t new_h, int64_t new_w,
                                        uint8_t *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out || h <= 0 || w <= 0 || new_h <= 0 || new_w <= 0 || h > (1 << 24) || w > (1 << 24))
        return fail(LARS_ERR_INVALID, "lars_h_resize_lanczos_u8: bad arguments");
    if (channels != 1 && channels != 3 && channels != 4)
        return fail(LARS_ERR_UNSUPPORTED, "lars_h_resize_lanczos_u8: 1, 3 or 4 channels (got %d)", channels);
    const int whole[4] = {0, 0, (int)w, (int)h};
    const float box[4] = {0.0f, 0.0f, (float)w, (float)h};
    return lars_h_thumbnail_u8(img, h, w, channels, 1, 1, whole, box, new_h, new_w, 0, out);
}
