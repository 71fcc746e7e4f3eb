// Baseline JPEG encoding of 8-bit pictures on the device: the file Pillow (libjpeg-turbo) writes by default, byte for byte.
//
// Reference: the white-balanced camera picture saved as ..._corrected.jpg (process-rgn.py:47 with :72-73, read back by
// process-ndvi.py:114) and an upload stored in its own format (process-images.py:247, JPEG for a camera file).  Both end in
// Image.save(..., "JPEG") on one host thread.  Here the file is built on the GPU and only its bytes cross PCIe.
//
// The header (SOI .. SOS), the quantisation tables of the quality and the standard Huffman codes come from the host
// (jpeg_tables.cpp).  Kernels, all deterministic (no atomic decides where a bit goes):
//   k_je_setup      the tables and the header into device memory.
//   k_je_transform  one workgroup per JE_MCUS MCUs of an MCU row: colour conversion, edge repetition and downsampling
//                   into LDS (each pixel is read once), libjpeg's jfdctint (rows, then columns) and the quantisation in LDS,
//                   then int16 coefficients in zigzag order, in scan order, dummy blocks included.
//   k_je_size       one lane per block: the DC difference (the previous block of the component is at a fixed distance in
//                   scan order) and the exact bit count of the block's codes; exclusive scan inside the workgroup.
//   k_je_exscan64   one workgroup: exclusive 64-bit scan of the workgroup sums (and later of the FF counts).
//   k_je_zero       zeroes the words the codes will occupy.
//   k_je_write      one lane per block writes its codes at its bit offset: whole words stored, the first and the last word
//                   of a block (shared with its neighbours) combined with atomicOr.  The last block pads with 1 bits.
//   k_je_count      FF bytes per JE_CHUNK bytes of the stream.
//   k_je_stuff      header, the bytes with 00 after every FF at the offset the scan gives, EOI and the file's length.
#include <string.h>

#include <algorithm>

#include "codec_host.h"
#include "wg_device.h"
#include "jpeg_tables.h"

namespace lars {

#define JE_THREADS 256
#define JE_MCUS 16                               // MCUs of one MCU row per workgroup of k_je_transform
#define JE_MAXBLK (JE_MCUS * 6)                  // 4:2:0 has six blocks per MCU
#define JE_CHUNK 1024                            // stream bytes per workgroup of k_je_count / k_je_stuff: one word per lane

static_assert(JE_CHUNK == 4 * JE_THREADS, "one 32-bit word of the stream per lane");

typedef unsigned long long je_u64;

struct JeTables {
    JpegEncCodes codes;
    uint16_t div[2][64];                         // quantisation table entry << 3 (jfdctint leaves 8 x the DCT), natural order
    uint8_t zigzag[64];
    uint8_t head[LARS_JPEG_HEADER_MAX];
    int nhead;
};
static_assert(sizeof(JeTables) % 4 == 0 && sizeof(JeTables) <= 3584, "k_je_setup takes it by value, copies it word by word");

struct JeCtl {
    je_u64 total_bits;                           // of the codes, before the padding of the last byte
    je_u64 total_ff;                             // FF bytes of the stream: as many 00 go in
    unsigned int overflow;                       // a write fell outside its buffer (cannot happen within lars_jpeg_bound)
    unsigned int reserved;
};

__global__ __launch_bounds__(64) void k_je_setup(JeTables a, JeTables *T, JeCtl *ctl)
{
    const unsigned int *src = reinterpret_cast<const unsigned int *>(&a);
    unsigned int *dst = reinterpret_cast<unsigned int *>(T);
    for (unsigned int i = threadIdx.x; i < sizeof(JeTables) / 4; i += 64) dst[i] = src[i];
    if (threadIdx.x == 0) {
        ctl->total_bits = 0;
        ctl->total_ff = 0;
        ctl->overflow = 0;
        ctl->reserved = 0;
    }
}

// ------------------------------------------------------------------------------------------------- transform
// One 8-point pass of libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2): the first pass (rows) keeps 2 extra bits, the second
// (columns) takes them off again; together they leave 8 times the DCT.
__device__ inline int je_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

template <bool FIRST>
__device__ inline void je_fdct8(int d[8])
{
    const int n = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    } else {
        d[0] = je_descale(t10 + t11, 2);
        d[4] = je_descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = je_descale(z1 + t13 * 6270, n);
    d[6] = je_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = je_descale(a4 + z1 + z3, n);
    d[5] = je_descale(a5 + z2 + z4, n);
    d[3] = je_descale(a6 + z2 + z3, n);
    d[1] = je_descale(a7 + z1 + z4, n);
}

// a block of component 0 that lies beyond the component's own size in blocks: not transformed, AC 0, DC of the block before
__device__ inline bool je_dummy(const JpegEncGeo &g, int mx, int my, int b)
{
    if (b >= g.ny || g.ny == 1) return false;
    return mx * g.hs + b % g.hs >= g.wb[0] || my * g.vs + b / g.hs >= g.hb[0];
}

__global__ __launch_bounds__(JE_THREADS) void k_je_transform(const uint8_t *__restrict__ img, JpegEncGeo g, const JeTables *__restrict__ T,
                                                             short *__restrict__ coef)
{
    __shared__ int s[JE_MAXBLK][64];
    __shared__ unsigned short s_div[2][64];
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x;
    const int gpr = (g.mcux + JE_MCUS - 1) / JE_MCUS;        // workgroups per MCU row
    const int my = blockIdx.x / gpr, mx0 = (blockIdx.x % gpr) * JE_MCUS;
    const int nm = min(JE_MCUS, g.mcux - mx0);
    const int fh = g.ncomp == 3 ? g.hs : 1, fv = g.ncomp == 3 ? g.vs : 1;
    if (tid < 128) s_div[tid >> 6][tid & 63] = T->div[tid >> 6][tid & 63];
    if (tid < 64) s_zz[tid] = T->zigzag[tid];

    // samples - 128 of every block into LDS.  A task is one chroma sample: fh x fv pixels, consecutive lanes along the row.
    // Right edge: the last column repeats.  Bottom edge: pixel rows repeat up to a whole row group (fv rows); below that the
    // last DOWNSAMPLED row of each component repeats -- for chroma that is the average of the last row group, not row h - 1.
    const int crows = (g.h + fv - 1) / fv;
    for (int t = tid; t < nm * 64; t += JE_THREADS) {
        const int gy = t / (nm * 8), r = t % (nm * 8), m = r >> 3, gx = r & 7;
        const int cx = (mx0 + m) * 8 + gx, cy = my * 8 + gy;
        if (g.ncomp == 1) {
            const int px = min(cx, g.w - 1), py = min(cy, g.h - 1);
            s[m][gy * 8 + gx] = (int)img[(long long)py * g.w + px] - 128;
            continue;
        }
        const int cyc = min(cy, crows - 1);
        int sum_cb = 0, sum_cr = 0;
        for (int dy = 0; dy < fv; ++dy) {
            const int yr = min(cy * fv + dy, g.h - 1), cr = min(cyc * fv + dy, g.h - 1);
            for (int dx = 0; dx < fh; ++dx) {
                const int px = min(cx * fh + dx, g.w - 1);
                const uint8_t *p = img + ((long long)yr * g.w + px) * 3;
                int R = p[0], G = p[1], B = p[2];
                const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
                const int yy = gy * fv + dy, xx = gx * fh + dx;
                s[m * g.bpm + (yy >> 3) * g.hs + (xx >> 3)][(yy & 7) * 8 + (xx & 7)] = Y - 128;
                if (cr != yr) {
                    const uint8_t *q = img + ((long long)cr * g.w + px) * 3;
                    R = q[0], G = q[1], B = q[2];
                }
                sum_cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                sum_cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            }
        }
        if (fh == 2 && fv == 2) {                            // libjpeg's alternating bias along the output columns: 1, 2, 1, 2
            sum_cb = (sum_cb + 1 + (cx & 1)) >> 2;
            sum_cr = (sum_cr + 1 + (cx & 1)) >> 2;
        } else if (fh == 2) {                                // 0, 1, 0, 1
            sum_cb = (sum_cb + (cx & 1)) >> 1;
            sum_cr = (sum_cr + (cx & 1)) >> 1;
        }
        s[m * g.bpm + g.ny][gy * 8 + gx] = sum_cb - 128;
        s[m * g.bpm + g.ny + 1][gy * 8 + gx] = sum_cr - 128;
    }
    __syncthreads();

    const int nblk = nm * g.bpm;
    for (int t = tid; t < nblk * 8; t += JE_THREADS) {       // rows
        int *row = &s[t >> 3][(t & 7) * 8];
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = row[i];
        je_fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) row[i] = d[i];
    }
    __syncthreads();
    for (int t = tid; t < nblk * 8; t += JE_THREADS) {       // columns, then sign(c) * ((|c| + d / 2) / d)
        const int blk = t >> 3, col = t & 7;
        const unsigned short *dv = s_div[(g.ncomp == 3 && blk % g.bpm >= g.ny) ? 1 : 0];
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s[blk][i * 8 + col];
        je_fdct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned int q = dv[i * 8 + col], a = (unsigned int)abs(d[i]);
            const int mag = (int)((a + (q >> 1)) / q);
            s[blk][i * 8 + col] = d[i] < 0 ? -mag : mag;
        }
    }
    __syncthreads();

    short *dst = coef + ((long long)my * g.mcux + mx0) * g.bpm * 64;
    for (int e = tid; e < nblk * 64; e += JE_THREADS) {
        const int blk = e >> 6, k = e & 63, m = blk / g.bpm, b = blk % g.bpm;
        int v;
        if (je_dummy(g, mx0 + m, my, b)) {
            int j = b;
            while (je_dummy(g, mx0 + m, my, j)) --j;         // block 0 of an MCU is never a dummy
            v = k == 0 ? s[m * g.bpm + j][0] : 0;
        } else {
            v = s[blk][s_zz[k]];
        }
        dst[e] = (short)v;
    }
}

// ------------------------------------------------------------------------------------------------- entropy coding
__device__ inline int je_category(int v) { return 32 - __clz(abs(v)); }       // 0 for 0

// The codes of block gb, in order, to emit(value, bits): the Huffman code with its extra bits behind it, at most 27 bits.
template <typename Emit>
__device__ inline void je_block_codes(const short *__restrict__ coef, const JpegEncGeo &g, const JpegEncCodes &C, long long gb, Emit emit)
{
    const int b = (int)(gb % g.bpm);
    const int t = (g.ncomp == 3 && b >= g.ny) ? 1 : 0;
    // the previous block of the same component: the one before inside the MCU's luminance blocks, else one MCU back
    long long prev;
    if (b > 0 && b < g.ny) prev = gb - 1;
    else if (b == 0) prev = gb - g.bpm + g.ny - 1;
    else prev = gb - g.bpm;
    const uint4 *src = reinterpret_cast<const uint4 *>(coef + gb * 64);
    uint4 w = src[0];
    const int dc = (short)(w.x & 0xFFFFu);
    const int diff = dc - (prev >= 0 ? (int)coef[prev * 64] : 0);
    int n = je_category(diff);
    emit(((unsigned int)C.dc_code[t][n] << n) | ((unsigned int)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u)), C.dc_len[t][n] + n);
    int run = 0;
    for (int q = 0; q < 8; ++q) {
        if (q) w = src[q];
        const unsigned int word[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (q == 0 && i == 0) continue;
            const int v = (short)((word[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu);
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                emit(C.ac_code[t][0xF0], C.ac_len[t][0xF0]);
                run -= 16;
            }
            n = je_category(v);
            const int sym = run << 4 | n;
            emit(((unsigned int)C.ac_code[t][sym] << n) | ((unsigned int)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), C.ac_len[t][sym] + n);
            run = 0;
        }
    }
    if (run > 0) emit(C.ac_code[t][0], C.ac_len[t][0]);
}

__device__ inline void je_load_codes(JpegEncCodes *dst, const JeTables *T)
{
    static_assert(sizeof(JpegEncCodes) % 4 == 0, "copied word by word");
    const unsigned int *src = reinterpret_cast<const unsigned int *>(&T->codes);
    unsigned int *d = reinterpret_cast<unsigned int *>(dst);
    for (unsigned int i = threadIdx.x; i < sizeof(JpegEncCodes) / 4; i += JE_THREADS) d[i] = src[i];
    __syncthreads();
}

__global__ __launch_bounds__(JE_THREADS) void k_je_size(const short *__restrict__ coef, JpegEncGeo g, const JeTables *__restrict__ T,
                                                        unsigned int *__restrict__ loc, unsigned int *__restrict__ wgsum)
{
    __shared__ JpegEncCodes C;
    __shared__ unsigned int s_w[JE_THREADS / 64];
    je_load_codes(&C, T);
    const long long gb = (long long)blockIdx.x * JE_THREADS + threadIdx.x;
    unsigned int bits = 0;
    if (gb < g.nblocks) je_block_codes(coef, g, C, gb, [&](unsigned int, int n) { bits += (unsigned int)n; });
    unsigned int total;
    const unsigned int excl = wg_exscan<JE_THREADS>(bits, s_w, &total);
    if (gb < g.nblocks) loc[gb] = excl;
    if (threadIdx.x == 0) wgsum[blockIdx.x] = total;
}

// exclusive scan of in[0..n) into 64-bit sums by one workgroup, chunk after chunk.  n is given, or (bits != nullptr) it is
// the number of JE_CHUNK-byte chunks of a stream of *bits bits.
__global__ __launch_bounds__(1024) void k_je_exscan64(const unsigned int *__restrict__ in, je_u64 *__restrict__ out, long long n,
                                                      const je_u64 *bits, je_u64 *total)
{
    if (bits) n = min(n, (long long)(((*bits + 7) / 8 + JE_CHUNK - 1) / JE_CHUNK));
    const je_u64 sum = wg_scan_array<je_u64>(n, [&](long long i) { return in[i]; }, [&](long long i, je_u64 before) { out[i] = before; });
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(JE_THREADS) void k_je_zero(unsigned int *__restrict__ words, je_u64 cap_words, const JeCtl *ctl)
{
    const je_u64 n = min(cap_words, (ctl->total_bits + 31) / 32 + 1);
    for (je_u64 i = (je_u64)blockIdx.x * JE_THREADS + threadIdx.x; i < n; i += (je_u64)gridDim.x * JE_THREADS) words[i] = 0u;
}

// The stream is kept as 32-bit words whose most significant bit comes first.  A block owns every word that lies wholly inside
// its bits and shares its first and its last word with its neighbours: those two are ORed in, the others stored.
struct JeBitWriter {
    unsigned int *words;
    je_u64 wi, cap;
    je_u64 acc;
    int n;
    bool first;
    unsigned int *overflow;
    __device__ void word_out(unsigned int v, bool shared)
    {
        if (wi >= cap) {
            *overflow = 1u;
        } else if (shared) {
            atomicOr(&words[wi], v);
        } else {
            words[wi] = v;
        }
        ++wi;
    }
    __device__ void put(unsigned int value, int bits)
    {
        acc = (acc << bits) | value;
        n += bits;
        if (n >= 32) {
            n -= 32;
            word_out((unsigned int)(acc >> n), first);
            first = false;
        }
    }
    __device__ void finish()
    {
        if (n > 0) word_out((unsigned int)(acc << (32 - n)), true);
    }
};

__global__ __launch_bounds__(JE_THREADS) void k_je_write(const short *__restrict__ coef, JpegEncGeo g, const JeTables *__restrict__ T,
                                                         const unsigned int *__restrict__ loc, const je_u64 *__restrict__ wgoff,
                                                         unsigned int *words, je_u64 cap_words, JeCtl *ctl)
{
    __shared__ JpegEncCodes C;
    je_load_codes(&C, T);
    const long long gb = (long long)blockIdx.x * JE_THREADS + threadIdx.x;
    if (gb >= g.nblocks) return;
    const je_u64 at = wgoff[blockIdx.x] + loc[gb];
    // the bits before `at` in the first word are the neighbour's: they enter the accumulator as zeroes
    JeBitWriter bw = {words, at >> 5, cap_words, 0ull, (int)(at & 31), true, &ctl->overflow};
    je_block_codes(coef, g, C, gb, [&](unsigned int v, int n) { bw.put(v, n); });
    if (gb == g.nblocks - 1) {                               // the last byte is padded with 1 bits
        const int pad = (int)((8 - (ctl->total_bits & 7)) & 7);
        if (pad) bw.put((1u << pad) - 1u, pad);
    }
    bw.finish();
}

__device__ inline unsigned int je_stream_byte(unsigned int word, int j) { return (word >> (24 - 8 * j)) & 255u; }

__global__ __launch_bounds__(JE_THREADS) void k_je_count(const unsigned int *__restrict__ words, const JeCtl *ctl, unsigned int *__restrict__ ffcnt)
{
    __shared__ unsigned int s_w[JE_THREADS / 64];
    const je_u64 nbytes = (ctl->total_bits + 7) / 8;
    const je_u64 base = (je_u64)blockIdx.x * JE_CHUNK;
    if (base >= nbytes) return;
    const je_u64 at = base + 4ull * threadIdx.x;
    unsigned int n = 0;
    if (at < nbytes) {
        const unsigned int w = words[at >> 2];
        for (int j = 0; j < 4; ++j) n += (at + j < nbytes && je_stream_byte(w, j) == 255u) ? 1u : 0u;
    }
    unsigned int total;
    wg_exscan<JE_THREADS>(n, s_w, &total);
    if (threadIdx.x == 0) ffcnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(JE_THREADS) void k_je_stuff(const unsigned int *__restrict__ words, const je_u64 *__restrict__ ffoff,
                                                         const JeTables *__restrict__ T, JeCtl *ctl, uint8_t *__restrict__ out, je_u64 out_cap,
                                                         long long *out_len)
{
    __shared__ unsigned int s_w[JE_THREADS / 64];
    const je_u64 nbytes = (ctl->total_bits + 7) / 8;
    const je_u64 base = (je_u64)blockIdx.x * JE_CHUNK;
    const je_u64 nhead = (je_u64)T->nhead;
    if (blockIdx.x == 0) {
        const je_u64 len = nhead + nbytes + ctl->total_ff + 2;
        const bool fits = len <= out_cap && ctl->overflow == 0;
        if (fits)
            for (unsigned int i = threadIdx.x; i < nhead; i += JE_THREADS) out[i] = T->head[i];
        if (threadIdx.x == 0) {
            if (fits) {
                out[len - 2] = 0xFF;
                out[len - 1] = 0xD9;
            }
            *out_len = fits ? (long long)len : 0ll;
        }
    }
    if (base >= nbytes) return;
    const je_u64 at = base + 4ull * threadIdx.x;
    unsigned int w = 0, n = 0;
    if (at < nbytes) {
        w = words[at >> 2];
        for (int j = 0; j < 4; ++j) n += (at + j < nbytes && je_stream_byte(w, j) == 255u) ? 1u : 0u;
    }
    unsigned int total;
    const unsigned int excl = wg_exscan<JE_THREADS>(n, s_w, &total);
    if (at >= nbytes) return;
    je_u64 o = nhead + at + ffoff[blockIdx.x] + excl;
    for (int j = 0; j < 4 && at + j < nbytes; ++j) {
        const unsigned int b = je_stream_byte(w, j);
        if (o + (b == 255u ? 2 : 1) > out_cap) return;       // cannot happen within lars_jpeg_bound; block 0 reports it
        out[o++] = (uint8_t)b;
        if (b == 255u) out[o++] = 0;
    }
}

// the device scratch of one picture: what lars_jpeg_encode_scratch_bytes counts and lars_d_encode_jpeg_u8 points into
struct JePlan {
    je_u64 cap_words;
    long long nwg, nchunks;                      // workgroups of k_je_size / k_je_write; chunks of the longest stream
    JeTables *tables;
    JeCtl *ctl;
    short *coef;
    unsigned int *loc, *wgsum, *words, *ffcnt;
    je_u64 *wgoff, *ffoff;
};

static JePlan je_plan(const JpegEncGeo &g, Carver &cv)
{
    JePlan P;
    P.nwg = (g.nblocks + JE_THREADS - 1) / JE_THREADS;
    const je_u64 max_bits = (je_u64)g.nblocks * (je_u64)jpeg_enc_max_block_bits();
    P.cap_words = (max_bits + 31) / 32 + 2;
    P.nchunks = (long long)(((max_bits + 7) / 8 + JE_CHUNK - 1) / JE_CHUNK);
    P.tables = cv.take<JeTables>(1);
    P.ctl = cv.take<JeCtl>(1);
    P.coef = cv.take<short>((size_t)g.nblocks * 64);
    P.loc = cv.take<unsigned int>((size_t)g.nblocks);
    P.wgsum = cv.take<unsigned int>((size_t)P.nwg);
    P.wgoff = cv.take<je_u64>((size_t)P.nwg);
    P.words = cv.take<unsigned int>((size_t)P.cap_words);
    P.ffcnt = cv.take<unsigned int>((size_t)P.nchunks);
    P.ffoff = cv.take<je_u64>((size_t)P.nchunks);
    return P;
}

static int je_shape_fail(const char *who, int64_t h, int64_t w, int channels, int subsampling)
{
    return fail(LARS_ERR_UNSUPPORTED, "%s: 1 to 65500 on each side, 1 or 3 channels, subsampling 0 to 2, less than 2^31 samples (got %lld x %lld x %d, %d)",
                who, (long long)h, (long long)w, channels, subsampling);
}

}  // namespace lars

using namespace lars;

extern "C" {

size_t lars_jpeg_encode_scratch_bytes(int64_t h, int64_t w, int channels, int subsampling)
{
    JpegEncGeo g;
    if (!jpeg_enc_geometry(h, w, channels, subsampling, &g)) return 0;
    Carver size(nullptr);
    je_plan(g, size);
    return size.bytes();
}

int lars_d_encode_jpeg_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int quality, int subsampling, uint8_t *out,
                          size_t out_cap, int64_t *out_len_dev, void *scratch, void *stream)
{
    static const char *who = "lars_d_encode_jpeg_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out || !out_len_dev || !scratch) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    if (quality < 1 || quality > 100) return fail(LARS_ERR_INVALID, "%s: quality 1 to 100 (got %d)", who, quality);
    JpegEncGeo g;
    if (!jpeg_enc_geometry(h, w, channels, subsampling, &g)) return je_shape_fail(who, h, w, channels, subsampling);
    const size_t bound = lars_jpeg_bound(h, w, channels, subsampling);
    if (out_cap < bound) return fail(LARS_ERR_INVALID, "%s: out_cap %zu < lars_jpeg_bound %zu", who, out_cap, bound);
    Carver cv(scratch);
    const JePlan P = je_plan(g, cv);
    if (P.nwg >= (1ll << 31) || P.nchunks >= (1ll << 31)) return fail(LARS_ERR_UNSUPPORTED, "%s: %lld blocks", who, g.nblocks);

    JeTables A;
    memset(&A, 0, sizeof A);
    jpeg_enc_codes(&A.codes);
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        jpeg_enc_qtable(quality, t, q);
        for (int i = 0; i < 64; ++i) A.div[t][i] = (uint16_t)(q[i] << 3);
    }
    memcpy(A.zigzag, JE_ZIGZAG, 64);
    A.nhead = jpeg_enc_header(g, quality, A.head);

    hipStream_t s = pick_stream(c, stream);
    const unsigned int tgrid = (unsigned int)((long long)g.mcuy * ((g.mcux + JE_MCUS - 1) / JE_MCUS));
    const unsigned int zgrid = (unsigned int)std::min<je_u64>((P.cap_words + JE_THREADS - 1) / JE_THREADS, 4096);
    hipLaunchKernelGGL(k_je_setup, dim3(1), dim3(64), 0, s, A, P.tables, P.ctl);
    hipLaunchKernelGGL(k_je_transform, dim3(tgrid), dim3(JE_THREADS), 0, s, img, g, P.tables, P.coef);
    hipLaunchKernelGGL(k_je_size, dim3((unsigned)P.nwg), dim3(JE_THREADS), 0, s, P.coef, g, P.tables, P.loc, P.wgsum);
    hipLaunchKernelGGL(k_je_exscan64, dim3(1), dim3(1024), 0, s, P.wgsum, P.wgoff, P.nwg, (const je_u64 *)nullptr, &P.ctl->total_bits);
    hipLaunchKernelGGL(k_je_zero, dim3(zgrid), dim3(JE_THREADS), 0, s, P.words, P.cap_words, P.ctl);
    hipLaunchKernelGGL(k_je_write, dim3((unsigned)P.nwg), dim3(JE_THREADS), 0, s, P.coef, g, P.tables, P.loc, P.wgoff, P.words, P.cap_words, P.ctl);
    hipLaunchKernelGGL(k_je_count, dim3((unsigned)P.nchunks), dim3(JE_THREADS), 0, s, P.words, P.ctl, P.ffcnt);
    hipLaunchKernelGGL(k_je_exscan64, dim3(1), dim3(1024), 0, s, P.ffcnt, P.ffoff, P.nchunks, &P.ctl->total_bits, &P.ctl->total_ff);
    hipLaunchKernelGGL(k_je_stuff, dim3((unsigned)P.nchunks), dim3(JE_THREADS), 0, s, P.words, P.ffoff, P.tables, P.ctl, out, (je_u64)out_cap,
                       reinterpret_cast<long long *>(out_len_dev));
    return launch_check(who);
}

// host picture in, JPEG file out: one upload, then the file's length (one small read) and its bytes
int lars_h_encode_jpeg_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int quality, int subsampling, uint8_t *out,
                          size_t out_cap, int64_t *out_len)
{
    static const char *who = "lars_h_encode_jpeg_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out || !out_len) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    const size_t bound = lars_jpeg_bound(h, w, channels, subsampling), scr = lars_jpeg_encode_scratch_bytes(h, w, channels, subsampling);
    if (!bound || !scr) return je_shape_fail(who, h, w, channels, subsampling);
    return encode_to_host(c, who, img, (size_t)h * w * channels, bound, scr, 0, out, out_cap, out_len,
                          [&](const uint8_t *d_in, uint8_t *d_out, int64_t *d_len, char *d_scr, uint8_t *, hipStream_t s) -> int {
                              return lars_d_encode_jpeg_u8(d_in, h, w, channels, quality, subsampling, d_out, bound, d_len, d_scr, s);
                          });
}

}  // extern "C"
