// PNG encoding of 8-bit pictures on the device (index colormaps, palette pictures, the white-balanced image).
//
// Reference: every index picture the batch driver writes (backend-process.py:49-73) and every picture of the ZIP export
// (process-images.py:567-617) ends in Image.fromarray(...).save(png): zlib on one host thread.  Here the whole file is
// built on the GPU and only its bytes cross PCIe.  The pixels are exactly the input's; the compressed bytes are not zlib's
// (PNG does not fix them).
//
// Four kernels, all deterministic (no atomic decides where a byte goes):
//   k_png_filter   one workgroup per row: the five PNG filters (bpp = channels), libpng's heuristic (smallest sum of
//                  |byte as int8|, ties to the lowest filter id), filter byte + filtered row into one contiguous stream.
//   k_png_deflate  one workgroup per PNG_SEG bytes of that stream: symbol histogram in LDS, length-limited (15 bit)
//                  Huffman code lengths (Moffat-Katajainen + the max-code-length fix-up, on one lane), the dynamic block
//                  header with its code-length alphabet (16/17/18 runs), then every thread packs the codes of its
//                  sub-range at the bit offset a workgroup prefix sum gives it.  Literal-only coding (zlib's
//                  Z_HUFFMAN_ONLY strategy).  Every segment but the last ends in an empty stored block (sync flush) so
//                  that it ends on a byte boundary; a segment whose dynamic block would be larger is stored instead.
//                  Each segment also leaves its Adler-32 partial sums.
//   k_png_frame    one workgroup: exclusive scan of the chunk sizes, Adler-32 combine, signature, IHDR (+ PLTE, tRNS),
//                  IEND and the file length.
//   k_png_idat     one workgroup per segment: the segment's bytes become one IDAT chunk; the workgroup computes the
//                  chunk's CRC-32 (per-thread pieces shifted by x^(8 * bytes after them) mod P, then XOR).
#include <string.h>

#include "checksum_device.h"
#include "codec_host.h"
#include "deflate_device.h"
#include "deflate_lz_device.h"

namespace lars {

#define PNG_SEG DEFLATE_SEG                     // bytes of filtered stream per deflate block (one workgroup)
#define PNG_THREADS DEFLATE_THREADS
#define PNG_ZCAP DEFLATE_ZCAP                   // per-segment output capacity

__device__ inline unsigned int abs_s8(unsigned int v) { return v < 128u ? v : 256u - v; }

__device__ inline unsigned int paeth(unsigned int a, unsigned int b, unsigned int c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ inline unsigned int png_filtered(int f, unsigned int x, unsigned int a, unsigned int b, unsigned int c)
{
    switch (f) {
    case 0: return x;
    case 1: return (x - a) & 255u;
    case 2: return (x - b) & 255u;
    case 3: return (x - ((a + b) >> 1)) & 255u;
    default: return (x - paeth(a, b, c)) & 255u;
    }
}

// one workgroup per row: filt[y * (rowb + 1)] = filter id, then the filtered row
__global__ __launch_bounds__(PNG_THREADS) void k_png_filter(const uint8_t *__restrict__ img, long long rowb, int bpp,
                                                           uint8_t *__restrict__ filt)
{
    __shared__ unsigned long long red[5][PNG_THREADS];
    __shared__ int s_best;
    const long long y = blockIdx.x;
    const int tid = threadIdx.x;
    const uint8_t *row = img + y * rowb;
    const uint8_t *prev = y ? row - rowb : nullptr;
    unsigned long long sum[5] = {0, 0, 0, 0, 0};
    for (long long i = tid; i < rowb; i += PNG_THREADS) {
        const unsigned int x = row[i], a = i >= bpp ? row[i - bpp] : 0u, b = prev ? prev[i] : 0u,
                           c = (prev && i >= bpp) ? prev[i - bpp] : 0u;
#pragma unroll
        for (int f = 0; f < 5; ++f) sum[f] += abs_s8(png_filtered(f, x, a, b, c));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) red[f][tid] = sum[f];
    __syncthreads();
    for (int half = PNG_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half)
#pragma unroll
            for (int f = 0; f < 5; ++f) red[f][tid] += red[f][tid + half];
        __syncthreads();
    }
    if (tid == 0) {
        int best = 0;
        for (int f = 1; f < 5; ++f)
            if (red[f][0] < red[best][0]) best = f;
        s_best = best;
    }
    __syncthreads();
    const int best = s_best;
    uint8_t *dst = filt + y * (rowb + 1);
    if (tid == 0) dst[0] = (uint8_t)best;
    for (long long i = tid; i < rowb; i += PNG_THREADS) {
        const unsigned int x = row[i], a = i >= bpp ? row[i - bpp] : 0u, b = prev ? prev[i] : 0u,
                           c = (prev && i >= bpp) ? prev[i - bpp] : 0u;
        dst[1 + i] = (uint8_t)png_filtered(best, x, a, b, c);
    }
}

// one workgroup per segment of the filtered stream -> Z + seg * PNG_ZCAP, seglen[seg] bytes; adl[2 seg] = sum of the bytes,
// adl[2 seg + 1] = sum of (n - j) * byte_j, both mod ADLER_MOD (deflate_device.h)
__global__ __launch_bounds__(PNG_THREADS) void k_png_deflate(const uint8_t *__restrict__ filt, long long total, long long nseg,
                                                            uint8_t *__restrict__ Z, unsigned int *__restrict__ seglen,
                                                            unsigned int *__restrict__ adl)
{
    const long long seg = blockIdx.x;
    const long long base = seg * PNG_SEG;
    const int n = (int)(total - base < PNG_SEG ? total - base : PNG_SEG);
    deflate_segment(filt + base, n, seg == 0, seg == nseg - 1, Z + seg * PNG_ZCAP, seglen + seg, adl + 2 * seg);
}

// the same with string matching (deflate_lz_device.h), where the tuning knob deflate_matching is 1
__global__ __launch_bounds__(DLZ_THREADS) void k_png_deflate_lz(const uint8_t *__restrict__ filt, long long total, long long nseg,
                                                               uint8_t *__restrict__ Z, unsigned int *__restrict__ seglen,
                                                               unsigned int *__restrict__ adl)
{
    const long long seg = blockIdx.x;
    const long long base = seg * PNG_SEG;
    const int n = (int)(total - base < PNG_SEG ? total - base : PNG_SEG);
    deflate_lz_segment(filt + base, n, seg == 0, seg == nseg - 1, Z + seg * PNG_ZCAP, seglen + seg, adl + 2 * seg);
}

__device__ void put_be32(uint8_t *p, unsigned int v)
{
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// a chunk of the given type and data at p (length, type, data, CRC over type + data); returns its size
__device__ unsigned int put_chunk(const unsigned int *tab, uint8_t *p, const char *type, const uint8_t *data, unsigned int len,
                                  const uint8_t *palette_rgba, int pal_mode)
{
    put_be32(p, len);
    unsigned int crc = 0xFFFFFFFFu;
    for (int i = 0; i < 4; ++i) { p[4 + i] = (uint8_t)type[i]; crc = crc_update(tab, crc, (uint8_t)type[i]); }
    for (unsigned int i = 0; i < len; ++i) {
        // pal_mode 1: PLTE (the RGB of each entry), 2: tRNS (the alpha of each entry), 0: data as given
        const uint8_t b = pal_mode == 1 ? palette_rgba[(i / 3) * 4 + i % 3] : (pal_mode == 2 ? palette_rgba[i * 4 + 3] : data[i]);
        p[8 + i] = b;
        crc = crc_update(tab, crc, b);
    }
    put_be32(p + 8 + len, ~crc);
    return 12 + len;
}

#define PNG_FRAME_THREADS 1024

// chunk offsets, Adler-32, the file's fixed chunks and its length
__global__ __launch_bounds__(PNG_FRAME_THREADS) void k_png_frame(long long nseg, long long total, uint8_t *__restrict__ Z,
                                                                const unsigned int *__restrict__ seglen,
                                                                const unsigned int *__restrict__ adl,
                                                                unsigned long long *__restrict__ off, int w, int h,
                                                                int color_type, const uint8_t *__restrict__ palette_rgba,
                                                                int palette_len, unsigned long long head,
                                                                uint8_t *__restrict__ out, unsigned long long out_cap,
                                                                long long *__restrict__ out_len)
{
    __shared__ unsigned long long s_w[2 * PNG_FRAME_THREADS / 64];
    __shared__ unsigned int tab[256];
    const int tid = threadIdx.x;
    crc_table_fill(tab, tid, PNG_FRAME_THREADS);
    const long long per = (nseg + PNG_FRAME_THREADS - 1) / PNG_FRAME_THREADS;
    const long long lo = min(nseg, tid * per), hi = min(nseg, lo + per);
    unsigned long long s = 0, A = 0, B = 0;
    for (long long k = lo; k < hi; ++k) {
        s += 12ull + seglen[k];
        const long long o = k * PNG_SEG, nk = min((long long)PNG_SEG, total - o);
        adler_append(A, B, adl[2 * k], adl[2 * k + 1], (unsigned long long)(total - o - nk));
    }
    unsigned long long chunks;                              // the bytes of all IDAT chunks
    unsigned long long o = head + wg_exscan<PNG_FRAME_THREADS>(s, s_w, &chunks);
    for (long long k = lo; k < hi; ++k) {
        off[k] = o;
        o += 12ull + seglen[k];
    }
    adler_wg<PNG_FRAME_THREADS>(A, B, s_w);
    if (tid == 0) {
        uint8_t *zl = Z + (nseg - 1) * PNG_ZCAP + seglen[nseg - 1] - 4;
        put_be32(zl, adler_value(A, B, (unsigned long long)total));
        const unsigned long long file = head + chunks + 12ull;
        if (file > out_cap) { *out_len = -1; return; }
        const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        for (int i = 0; i < 8; ++i) out[i] = sig[i];
        uint8_t ihdr[13];
        put_be32(ihdr, (unsigned int)w);
        put_be32(ihdr + 4, (unsigned int)h);
        ihdr[8] = 8;
        ihdr[9] = (uint8_t)color_type;
        ihdr[10] = ihdr[11] = ihdr[12] = 0;
        unsigned int p = 8;
        p += put_chunk(tab, out + p, "IHDR", ihdr, 13, nullptr, 0);
        if (color_type == 3) {
            p += put_chunk(tab, out + p, "PLTE", nullptr, 3u * palette_len, palette_rgba, 1);
            p += put_chunk(tab, out + p, "tRNS", nullptr, (unsigned)palette_len, palette_rgba, 2);
        }
        put_chunk(tab, out + file - 12, "IEND", nullptr, 0, nullptr, 0);
        *out_len = (long long)file;
    }
}

// one workgroup per segment: its IDAT chunk at off[seg]
__global__ __launch_bounds__(PNG_THREADS) void k_png_idat(const uint8_t *__restrict__ Z, const unsigned int *__restrict__ seglen,
                                                         const unsigned long long *__restrict__ off, uint8_t *__restrict__ out,
                                                         unsigned long long out_cap)
{
    __shared__ unsigned int tab[256];
    __shared__ unsigned int x2n[32];
    __shared__ unsigned int part[PNG_THREADS / 64];
    const int tid = threadIdx.x;
    const long long seg = blockIdx.x;
    const unsigned int m = seglen[seg];
    const unsigned long long o = off[seg];
    if (o + 12ull + m > out_cap) return;         // k_png_frame refused the file (cannot happen within lars_png_bound)
    crc_table_fill(tab, tid, PNG_THREADS);
    if (tid == 0) crc_x2n_fill(x2n);
    const uint8_t *z = Z + seg * PNG_ZCAP;
    uint8_t *dst = out + o;
    for (unsigned int j = tid; j < m; j += PNG_THREADS) dst[8 + j] = z[j];
    if (tid == 0) {
        put_be32(dst, m);
        dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
    }
    __syncthreads();
    // CRC-32 of "IDAT" + data
    const unsigned int idat = 0x54414449u;       // "IDAT", first letter in the low byte
    const unsigned int crc = wg_crc32<PNG_THREADS>(m + 4u, [&](unsigned int j) { return j < 4 ? (idat >> (8 * j)) & 255u : (unsigned int)z[j - 4]; },
                                                   tab, x2n, part);
    if (tid == 0) put_be32(dst + 8 + m, crc);
}

static bool png_shape_ok(int64_t h, int64_t w, int channels)
{
    return h > 0 && w > 0 && h <= (1 << 24) && w <= (1 << 24) && (channels == 1 || channels == 3 || channels == 4);
}

// geometry and the device scratch of one picture: what lars_png_scratch_bytes counts and lars_d_encode_png_u8 points into
struct PngPlan {
    long long rowb, total, nseg;
    uint8_t *filt, *z;
    unsigned int *seglen, *adl;
    unsigned long long *off;
};

static PngPlan png_plan(int64_t h, int64_t w, int channels, Carver &cv)
{
    PngPlan P;
    P.rowb = (long long)w * channels;
    P.total = (long long)h * (P.rowb + 1);
    P.nseg = (P.total + PNG_SEG - 1) / PNG_SEG;
    P.filt = cv.take<uint8_t>((size_t)P.total);
    P.z = cv.take<uint8_t>((size_t)P.nseg * PNG_ZCAP);
    P.seglen = cv.take<unsigned int>((size_t)P.nseg);
    P.adl = cv.take<unsigned int>((size_t)P.nseg * 2);
    P.off = cv.take<unsigned long long>((size_t)P.nseg);
    return P;
}

static unsigned long long png_head_bytes(int color_type, int palette_len)
{
    return 8ull + 25ull + (color_type == 3 ? 24ull + 4ull * palette_len : 0ull);
}

// the argument checks of both encode entry points; pointers: the caller's own pointers are all set
static int png_encode_check(const char *who, bool pointers, int64_t h, int64_t w, int channels, const uint8_t *palette_rgba, int palette_len)
{
    if (!pointers || h <= 0 || w <= 0 || h > (1 << 24) || w > (1 << 24)) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    if (channels != 1 && channels != 3 && channels != 4) return fail(LARS_ERR_UNSUPPORTED, "%s: 1, 3 or 4 channels (got %d)", who, channels);
    if (palette_rgba && (channels != 1 || palette_len < 1 || palette_len > 256))
        return fail(LARS_ERR_INVALID, "%s: a palette needs one channel and 1..256 entries (got %d, %d)", who, channels, palette_len);
    return LARS_OK;
}

}  // namespace lars

using namespace lars;

extern "C" {

// worst case: every segment stored (5 header bytes each) or a dynamic block no larger; 12 bytes of framing per IDAT; zlib
// header and Adler-32; signature, IHDR, a 256-entry PLTE + tRNS for one channel, IEND
size_t lars_png_bound(int64_t h, int64_t w, int channels)
{
    if (!png_shape_ok(h, w, channels)) return 0;
    Carver none(nullptr);
    const PngPlan P = png_plan(h, w, channels, none);
    return (size_t)P.total + (size_t)P.nseg * (5 + 12) + 6 + png_head_bytes(channels == 1 ? 3 : 2, 256) + 12;
}

size_t lars_png_scratch_bytes(int64_t h, int64_t w, int channels)
{
    if (!png_shape_ok(h, w, channels)) return 0;
    Carver size(nullptr);
    png_plan(h, w, channels, size);
    return size.bytes();
}

int lars_d_encode_png_u8(const uint8_t *img, int64_t h, int64_t w, int channels, const uint8_t *palette_rgba, int palette_len,
                         uint8_t *out, size_t out_cap, int64_t *out_len_dev, void *scratch, void *stream)
{
    static const char *who = "lars_d_encode_png_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_TRY(png_encode_check(who, img && out && out_len_dev && scratch, h, w, channels, palette_rgba, palette_len));
    const size_t bound = lars_png_bound(h, w, channels);
    if (out_cap < bound) return fail(LARS_ERR_INVALID, "%s: out_cap %zu < lars_png_bound %zu", who, out_cap, bound);
    Carver cv(scratch);
    const PngPlan P = png_plan(h, w, channels, cv);
    if (P.nseg >= (1ll << 31)) return fail(LARS_ERR_UNSUPPORTED, "%s: %lld segments", who, P.nseg);
    const int color_type = palette_rgba ? 3 : (channels == 1 ? 0 : (channels == 3 ? 2 : 6));
    hipStream_t s = pick_stream(c, stream);
    hipLaunchKernelGGL(k_png_filter, dim3((unsigned)h), dim3(PNG_THREADS), 0, s, img, P.rowb, channels, P.filt);
    if (tuning().deflate_matching)
        hipLaunchKernelGGL(k_png_deflate_lz, dim3((unsigned)P.nseg), dim3(DLZ_THREADS), 0, s, P.filt, P.total, P.nseg, P.z, P.seglen, P.adl);
    else
        hipLaunchKernelGGL(k_png_deflate, dim3((unsigned)P.nseg), dim3(PNG_THREADS), 0, s, P.filt, P.total, P.nseg, P.z, P.seglen, P.adl);
    hipLaunchKernelGGL(k_png_frame, dim3(1), dim3(PNG_FRAME_THREADS), 0, s, P.nseg, P.total, P.z, P.seglen, P.adl, P.off, (int)w, (int)h,
                       color_type, palette_rgba, palette_rgba ? palette_len : 0, png_head_bytes(color_type, palette_len), out,
                       (unsigned long long)out_cap, reinterpret_cast<long long *>(out_len_dev));
    hipLaunchKernelGGL(k_png_idat, dim3((unsigned)P.nseg), dim3(PNG_THREADS), 0, s, P.z, P.seglen, P.off, out, (unsigned long long)out_cap);
    return launch_check(who);
}

// host image in, PNG file out: one upload, then the file's length (one small read) and its bytes
int lars_h_encode_png_u8(const uint8_t *img, int64_t h, int64_t w, int channels, const uint8_t *palette_rgba, int palette_len,
                         uint8_t *out, size_t out_cap, int64_t *out_len)
{
    static const char *who = "lars_h_encode_png_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_TRY(png_encode_check(who, img && out && out_len, h, w, channels, palette_rgba, palette_len));
    const size_t bound = lars_png_bound(h, w, channels);
    return encode_to_host(c, who, img, (size_t)h * w * channels, bound, lars_png_scratch_bytes(h, w, channels), 1024, out, out_cap, out_len,
                          [&](const uint8_t *d_in, uint8_t *d_out, int64_t *d_len, char *d_scr, uint8_t *d_pal, hipStream_t s) -> int {
                              if (palette_rgba) LARS_HIP_TRY(hipMemcpyAsync(d_pal, palette_rgba, (size_t)palette_len * 4, hipMemcpyHostToDevice, s));
                              return lars_d_encode_png_u8(d_in, h, w, channels, palette_rgba ? d_pal : nullptr, palette_len, d_out, bound, d_len, d_scr, s);
                          });
}

}  // extern "C"
