// Baseline JPEG decoding (SOF0 / SOF1, Huffman, 8 bit, one interleaved scan) on the device.
//
// Reference: load_image_from_db (process-images.py:181-193) and backend-process.py:52 open every stored picture with
// Image.open(...) and np.array(img) or img.thumbnail(...): libjpeg on one host core.  Here the file goes up once and the
// pixels (or only the thumbnail, lars_h_thumbnail_jpeg_u8) come back.  The pixel arithmetic is libjpeg-turbo's JDCT_ISLOW
// (the SIMD code's narrowing, see jd_idct8) with fancy upsampling, integer for integer, so the array is the one Pillow returns.
//
// The Huffman scan is serial by nature.  It is cut into subsequences of S bits ("jpeg_subseq_bits"), one lane each, and
// the decoder states at their borders are found by iteration; a border counts only once it equals what the exact chain
// from the last true synchronisation point (scan start, restart marker) gives, so the speculation changes the speed,
// never the result.  The host parser (jpeg_parse.cpp) gives the tables and the byte range of the entropy data.
//   k_jd_setup      one workgroup: Huffman decode tables (9-bit look-up + canonical lists) and quantisation tables of
//                   the three components into scratch, from the kernel's own arguments.
//   k_jd_mark       one thread per byte of the entropy segment: kept (data) or dropped (the 00 of FF 00, fill FFs,
//                   restart markers), restart marker or not; counts per workgroup.  k_jd_exscan: their exclusive scans.
//   k_jd_compact    the data bytes in one contiguous stream, the stream offset at which each restart interval starts,
//                   the sequence check of the markers (RSTm follows RSTm-1).
//   k_jd_intervals  subsequences per restart interval (at least one), the marker count against the frame's;
//                   k_jd_subs: the table of subsequences (binary search of the interval).
//   k_jd_pass       round 0: every lane decodes its subsequence from the assumed state (block 0 of an MCU, coefficient
//                   0) -- true for the first subsequence of an interval -- counting blocks only, and records where and in
//                   which state it left.  Then, in every round, a lane whose recorded entry differs from what its
//                   predecessor left takes that as its entry and decodes again, over and over inside the workgroup
//                   (at most 256 times) until no border inside it moves; the border between two workgroups is taken up
//                   by the next round.  A round in which no lane decoded ends the iteration (later rounds return at
//                   once).  A stream that synchronises within a workgroup's 256 subsequences needs three rounds.
//   k_jd_finish     one wave, only when the last round still changed something: walks the borders in order and redoes
//                   what disagrees, serially.  Exact by construction, slow only for streams that never synchronise.
//   k_jd_check      an invalid code or a coefficient index past 63 on the exact chain: the smallest such subsequence.
//   k_jd_verify     block index at which every interval starts (scan of the block counts) against the frame's.
//   k_jd_write      every lane decodes its subsequence again from its true entry and writes coefficients: int16,
//                   natural order, [block in scan order][64], DC as the difference.
//   k_jd_mcu_sums   DC differences per MCU and component; their scan gives DC = prefix(MCU) - prefix(interval start) +
//                   the differences inside the MCU (unsigned arithmetic: the wrap cancels).
//   k_jd_idct       eight lanes per block: dequantise, column pass, row pass (workspace in LDS, padded against bank
//                   conflicts), narrowing by saturation as libjpeg-turbo's SIMD code does it, 8 bytes per lane into the
//                   component plane.
//   k_jd_color      one thread per pixel: fancy (triangle) upsampling of Cb / Cr where the chroma plane is wider than
//                   two samples, replication else, YCbCr -> RGB in 16-bit fixed point, [h][w][3] or [h][w].
// At 1/2, 1/4 and 1/8 scale (Pillow's draft; lars_*_jpeg_scaled_*) the entropy stage is the same and the scaling starts at
// the coefficients, as in libjpeg: a block becomes 4 x 4, 2 x 2 or 1 x 1 samples (the chroma blocks of 4:2:0 twice that,
// so that they need no upsampling), see "scaled decoding" below:
//   k_jd_idct_reduced<4 | 2>   four lanes per block, 64 blocks per workgroup: the rows a size reads, dequantised, into LDS;
//                   column pass, row pass, 4 or 2 bytes per lane into the component plane.
//   k_jd_idct_dc    1 x 1: one lane per block, the DC alone.
//   k_jd_color_scaled   one thread per pixel of the scaled picture: h2v1 triangle filter or replication for the chroma
//                   of 4:2:2, nothing for the others, then the colour arithmetic of k_jd_color.
// Every loop is bounded by the length of the data, every index is checked against its buffer; an error is a status code
// (LARS_JPGD_*) in device memory and every kernel after a failing one returns at once.
#include <string.h>

#include <algorithm>

#include "codec_host.h"
#include "jpeg_parse.h"
#include "wg_device.h"

namespace lars {

#define JD_ROUNDS 8                       // parallel rounds before k_jd_finish takes what is left
#define JD_LOOK 9                         // bits of the Huffman look-up table
#define JD_MARK_THREADS 1024
#define JD_INVALID_CODE 0xFFFFFFFFFFFFFFFEull
#define JD_INVALID_COEF 0xFFFFFFFFFFFFFFFDull
#define JD_IS_INVALID(x) ((x) >= JD_INVALID_COEF)

typedef unsigned long long jd_u64;

struct JdTablesArg {                      // by value to k_jd_setup: per component, DC tables 0..2 and AC tables 3..5
    uint16_t qt[3][64];
    uint8_t hcount[6][16];
    uint8_t hval[6][256];
};

struct JdHuff {
    uint16_t look[1 << JD_LOOK];          // (length << 8) | symbol of the code that starts these bits, 0: longer than JD_LOOK
    int maxcode[18];                      // largest code of length l (-1: none); [17] stops the search
    int valoff[17];                       // index into val of the first code of length l, minus that code
    uint8_t val[256];
};

struct JdTables {
    JdHuff huff[6];
    uint16_t qt[3][64];
    uint8_t zigzag[64];
};

struct JdCtl {
    int status[2];
    jd_u64 errkey;                        // smallest (subsequence << 2 | kind) of an invalid exit on the exact chain
    unsigned int changed[JD_ROUNDS + 1];
    unsigned int kept_total, mark_total, nsub_total, block_total, bad_marker;
};

struct JdSub {
    jd_u64 start, end, iend;              // bit positions in the compact stream: own range, end of the restart interval
    unsigned int interval, first;
};

struct JdGeo {
    int w, h, ncomp, hs, vs;              // sampling of component 0 (the others are 1 x 1)
    int bpm, ny;                          // blocks per MCU, of which component 0's
    int mcux, mcuy;
    unsigned int nmcu, nblocks, ri, nint; // ri: MCUs per restart interval (nmcu when there are no restarts)
    int pw[3], ph[3];                     // plane sizes in samples
    unsigned int poff[3];                 // plane offsets in bytes
    unsigned int pblocks[4];              // blocks of the planes before component c
};

__constant__ uint8_t c_jd_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ inline void jd_fail(JdCtl *ctl, int code, int detail)
{
    if (atomicCAS(&ctl->status[0], 0, code) == 0) ctl->status[1] = detail;
}

// ------------------------------------------------------------------------------------------------- tables
__global__ __launch_bounds__(64) void k_jd_setup(JdTablesArg a, JdTables *T)
{
    const int t = threadIdx.x;
    for (int i = t; i < 3 * 64; i += 64) T->qt[i / 64][i % 64] = a.qt[i / 64][i % 64];
    T->zigzag[t] = c_jd_zigzag[t];
    if (t >= 6) return;
    JdHuff *H = &T->huff[t];
    for (int i = 0; i < (1 << JD_LOOK); ++i) H->look[i] = 0;
    for (int i = 0; i < 256; ++i) H->val[i] = a.hval[t][i];
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = a.hcount[t][l - 1];
        H->valoff[l] = k - code;
        if (n) {
            if (l <= JD_LOOK) {
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (JD_LOOK - l), fill = 1 << (JD_LOOK - l);
                    for (int f = 0; f < fill && first + f < (1 << JD_LOOK); ++f)
                        H->look[first + f] = (uint16_t)(l << 8 | a.hval[t][(k + i) & 255]);
                }
            }
            k += n;
            code += n;
            H->maxcode[l] = code - 1;
        } else {
            H->maxcode[l] = -1;
        }
        code <<= 1;
    }
    H->maxcode[0] = -1;
    H->maxcode[17] = 0x7FFFFFFF;
    H->valoff[0] = 0;
}

// ------------------------------------------------------------------------------------------------- marker scan
// what byte i of the entropy segment is: bit 0 kept (data), bit 1 the FF of a restart marker
__device__ inline int jd_classify(const uint8_t *seg, long long n, long long i)
{
    const int cur = seg[i], prev = i > 0 ? seg[i - 1] : 0, next = i + 1 < n ? seg[i + 1] : 0x100;
    if (cur == 0xFF) {
        if (next == 0x00) return 1;
        if (next >= 0xD0 && next <= 0xD7) return 2;
        return 0;                                         // a fill byte, or the last byte of the segment
    }
    if (prev == 0xFF && (cur == 0x00 || (cur >= 0xD0 && cur <= 0xD7))) return 0;
    return 1;
}

__global__ __launch_bounds__(JD_MARK_THREADS) void k_jd_mark(const uint8_t *seg, long long n, unsigned int *keepcnt, unsigned int *markcnt)
{
    __shared__ unsigned int s_keep, s_mark;
    if (threadIdx.x == 0) s_keep = s_mark = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * JD_MARK_THREADS + threadIdx.x;
    const int c = i < n ? jd_classify(seg, n, i) : 0;
    const jd_u64 bk = __ballot(c & 1), bm = __ballot(c & 2);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_keep, (unsigned int)__popcll(bk));
        atomicAdd(&s_mark, (unsigned int)__popcll(bm));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        keepcnt[blockIdx.x] = s_keep;
        markcnt[blockIdx.x] = s_mark;
    }
}

// exclusive scan of in[0..n) by one workgroup per channel (blockIdx.x * stride), chunk after chunk; in == out is fine
__global__ __launch_bounds__(1024) void k_jd_exscan(const unsigned int *in, unsigned int *out, long long n, long long stride, unsigned int *total)
{
    in += (long long)blockIdx.x * stride;
    out += (long long)blockIdx.x * stride;
    const unsigned int sum = wg_scan_array<unsigned int>(n, [&](long long i) { return in[i]; }, [&](long long i, unsigned int before) { out[i] = before; });
    if (threadIdx.x == 0 && total) total[blockIdx.x] = sum;
}

__global__ __launch_bounds__(JD_MARK_THREADS) void k_jd_compact(const uint8_t *seg, long long n, const unsigned int *keepoff,
                                                                const unsigned int *markoff, unsigned int nint, uint8_t *compact,
                                                                jd_u64 *cbyte, JdCtl *ctl)
{
    __shared__ unsigned int wk[JD_MARK_THREADS / 64], wm[JD_MARK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long i = (long long)blockIdx.x * JD_MARK_THREADS + tid;
    const int c = i < n ? jd_classify(seg, n, i) : 0;
    const jd_u64 bk = __ballot(c & 1), bm = __ballot(c & 2);
    if (lane == 0) {
        wk[wv] = (unsigned int)__popcll(bk);
        wm[wv] = (unsigned int)__popcll(bm);
    }
    __syncthreads();
    unsigned int pk = keepoff[blockIdx.x], pm = markoff[blockIdx.x];
    for (int v = 0; v < wv; ++v) {
        pk += wk[v];
        pm += wm[v];
    }
    const jd_u64 below = (1ull << lane) - 1;
    pk += (unsigned int)__popcll(bk & below);
    pm += (unsigned int)__popcll(bm & below);
    if (c & 1) compact[pk] = seg[i];                      // pk < kept bytes <= n
    if (c & 2) {
        if (seg[i + 1] != 0xD0 + (pm & 7)) atomicOr(&ctl->bad_marker, 1u);   // c & 2 implies i + 1 < n
        if (pm + 1 < nint) cbyte[pm + 1] = pk;            // the interval after marker pm starts at the next kept byte
    }
}

__global__ void k_jd_intervals(jd_u64 *cbyte, unsigned int nint, unsigned int sbits, unsigned int *nsubs, JdCtl *ctl)
{
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (ctl->mark_total != nint - 1 || ctl->bad_marker) {
        if (i == 0) jd_fail(ctl, LARS_JPGD_RESTART, (int)min(ctl->mark_total, 0x7FFFFFFFu));
        if (i < nint) nsubs[i] = 0;
        return;
    }
    if (i >= nint) return;
    const jd_u64 a = i == 0 ? 0ull : cbyte[i], b = i + 1 == nint ? (jd_u64)ctl->kept_total : cbyte[i + 1];
    if (i == 0) {
        cbyte[0] = 0;
        cbyte[nint] = ctl->kept_total;
    }
    const jd_u64 bits = (b - a) * 8;
    nsubs[i] = (unsigned int)max((bits + sbits - 1) / sbits, 1ull);
}

__global__ void k_jd_subs(const jd_u64 *cbyte, const unsigned int *suboff, unsigned int nint, unsigned int sbits, unsigned int cap,
                          JdSub *subs, JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned int total = ctl->nsub_total;
    if (total > cap) {
        if (j == 0) jd_fail(ctl, LARS_JPGD_INTERNAL, 1);
        return;
    }
    if (j >= total) return;
    unsigned int lo = 0, hi = nint - 1;                   // the last interval whose first subsequence is <= j
    while (lo < hi) {
        const unsigned int mid = (lo + hi + 1) >> 1;
        if (suboff[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const jd_u64 ibeg = cbyte[lo] * 8, iend = cbyte[lo + 1] * 8;
    const unsigned int local = j - suboff[lo];
    JdSub s;
    s.start = min(ibeg + (jd_u64)local * sbits, iend);
    s.end = min(s.start + sbits, iend);
    s.iend = iend;
    s.interval = lo;
    s.first = local == 0;
    subs[j] = s;
}

// ------------------------------------------------------------------------------------------------- entropy decode
__device__ inline unsigned int jd_peek32(const unsigned int *words, jd_u64 pos)
{
    const jd_u64 i = pos >> 5;
    const unsigned int a = __builtin_bswap32(words[i]), b = __builtin_bswap32(words[i + 1]);
    const unsigned int sh = (unsigned int)pos & 31u;
    return sh ? (a << sh) | (b >> (32 - sh)) : a;
}

__device__ inline jd_u64 jd_pack(jd_u64 pos, int b, int k) { return pos << 10 | (jd_u64)b << 6 | (jd_u64)k; }

// Decodes from (pos, block b of the MCU, coefficient k) until pos >= end; symbols that would cross iend are not taken
// (the padding of the interval's last byte).  Returns the packed exit state or JD_INVALID_*; cnt = blocks completed.
// WRITE: coefficients go to coef[blk][...] while blk < nblocks.  At most end - pos iterations: every symbol has a bit.
template <bool WRITE>
__device__ jd_u64 jd_run(const JdTables *T, const unsigned int *words, jd_u64 st, jd_u64 end, jd_u64 iend, int bpm, int ny,
                         unsigned int *cnt_out, short *coef, unsigned int blk, unsigned int nblocks)
{
    jd_u64 pos = st >> 10;
    int b = (int)(st >> 6) & 15, k = (int)st & 63;
    unsigned int cnt = 0;
    while (pos < end) {
        const int comp = b < ny ? 0 : b - ny + 1;
        const JdHuff *H = &T->huff[k == 0 ? comp : 3 + comp];
        const unsigned int w = jd_peek32(words, pos);
        int len, sym;
        const unsigned int e = H->look[w >> (32 - JD_LOOK)];
        if (e) {
            len = (int)(e >> 8);
            sym = (int)(e & 255);
        } else {
            len = JD_LOOK + 1;
            while ((int)(w >> (32 - len)) > H->maxcode[len]) ++len;   // maxcode[17] stops it
            if (len > 16) {
                if (pos + 16 > iend) { pos = iend; break; }          // padding at the end of the interval
                *cnt_out = cnt;
                return JD_INVALID_CODE;
            }
            sym = H->val[((int)(w >> (32 - len)) + H->valoff[len]) & 255];
        }
        const int s = sym & 15;
        if (pos + len + s > iend) { pos = iend; break; }
        int v = 0;
        if (s) {
            v = (int)((w << len) >> (32 - s));
            if (v < (1 << (s - 1))) v -= (1 << s) - 1;
        }
        pos += len + s;
        bool done = false;
        if (k == 0) {
            if (WRITE && blk < nblocks) coef[(size_t)blk * 64] = (short)v;
            k = 1;
        } else {
            const int r = sym >> 4;
            if (s == 0) {
                if (r == 15) { k += 16; done = k > 63; }
                else done = true;
            } else {
                k += r;
                if (k > 63) {
                    *cnt_out = cnt;
                    return JD_INVALID_COEF;
                }
                if (WRITE && blk < nblocks) coef[(size_t)blk * 64 + T->zigzag[k]] = (short)v;
                ++k;
                done = k > 63;
            }
        }
        if (done) {
            ++cnt;
            ++blk;
            k = 0;
            b = b + 1 == bpm ? 0 : b + 1;
        }
    }
    *cnt_out = cnt;
    return jd_pack(pos, b, k);
}

__device__ inline void jd_load_tables(JdTables *dst, const JdTables *src)
{
    const unsigned int *s = reinterpret_cast<const unsigned int *>(src);
    unsigned int *d = reinterpret_cast<unsigned int *>(dst);
    for (unsigned int i = threadIdx.x; i < sizeof(JdTables) / 4; i += blockDim.x) d[i] = s[i];
    __syncthreads();
}
static_assert(sizeof(JdTables) % 4 == 0, "JdTables is copied by words");

__global__ __launch_bounds__(256) void k_jd_pass(const JdTables *Tg, const unsigned int *words, const JdSub *subs, jd_u64 *in, jd_u64 *out,
                                                 unsigned int *cnt, int round, int bpm, int ny, JdCtl *ctl)
{
    __shared__ JdTables T;
    if (ctl->status[0]) return;
    if (round > 1 && ctl->changed[round - 1] == 0) return;
    const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = j < ctl->nsub_total;
    JdSub s{};
    jd_u64 my_in = 0;
    bool loaded = false, did = false;
    if (live) s = subs[j];
    if (round == 0) {
        jd_load_tables(&T, Tg);
        loaded = true;
        if (live) {
            unsigned int n = 0;
            my_in = jd_pack(s.start, 0, 0);
            const jd_u64 o = jd_run<false>(&T, words, my_in, s.end, s.iend, bpm, ny, &n, nullptr, 0, 0);
            in[j] = my_in;
            cnt[j] = n;
            __atomic_store_n(&out[j], o, __ATOMIC_RELAXED);
        }
    } else if (live) {
        my_in = in[j];
    }
    // The borders inside the workgroup, until none of them moves: at most one iteration per lane.  The border to the
    // workgroup before is looked at from round 1 on, when that workgroup has written it.
    for (int it = 0; it < 256; ++it) {
        __syncthreads();
        bool need = false;
        jd_u64 st = 0;
        if (live && !s.first && (threadIdx.x > 0 || round > 0)) {
            st = __atomic_load_n(&out[j - 1], __ATOMIC_RELAXED);
            need = !JD_IS_INVALID(st) && st != my_in;
        }
        if (!__syncthreads_or(need)) break;
        if (!loaded) {
            jd_load_tables(&T, Tg);
            loaded = true;
        }
        if (need) {
            unsigned int n = 0;
            const jd_u64 o = jd_run<false>(&T, words, st, s.end, s.iend, bpm, ny, &n, nullptr, 0, 0);
            my_in = st;
            in[j] = st;
            cnt[j] = n;
            __atomic_store_n(&out[j], o, __ATOMIC_RELAXED);
            did = true;
        }
    }
    if (did && round > 0) atomicAdd(&ctl->changed[round], 1u);
}

// what the rounds left: the borders in order, one wave, each lane owning one subsequence of a group of 64
__global__ __launch_bounds__(64) void k_jd_finish(const JdTables *Tg, const unsigned int *words, const JdSub *subs, jd_u64 *in, jd_u64 *out,
                                                  unsigned int *cnt, int bpm, int ny, JdCtl *ctl)
{
    __shared__ JdTables T;
    if (ctl->status[0] || ctl->changed[JD_ROUNDS] == 0) return;
    jd_load_tables(&T, Tg);
    const unsigned int total = ctl->nsub_total;
    const int lane = threadIdx.x;
    jd_u64 carry = JD_INVALID_CODE;                       // exit of the subsequence before the group
    for (unsigned int base = 0; base < total; base += 64) {
        const unsigned int j = base + lane;
        const bool live = j < total;
        JdSub s{};
        jd_u64 my_in = 0, my_out = 0;
        if (live) {
            s = subs[j];
            my_in = in[j];
            my_out = out[j];
        }
        const jd_u64 before = __shfl_up(my_out, 1);
        const jd_u64 prev = lane == 0 ? carry : before;
        const bool differs = live && !s.first && !JD_IS_INVALID(prev) && prev != my_in;
        if (__ballot(differs) != 0) {
            for (int l = 0; l < 64 && base + l < total; ++l) {
                const jd_u64 p = l == 0 ? carry : __shfl(my_out, l - 1);
                if (lane == l && !s.first && !JD_IS_INVALID(p) && p != my_in) {
                    unsigned int n = 0;
                    my_out = jd_run<false>(&T, words, p, s.end, s.iend, bpm, ny, &n, nullptr, 0, 0);
                    in[j] = p;
                    cnt[j] = n;
                    out[j] = my_out;
                }
            }
        }
        carry = __shfl(my_out, 63);                       // a group that is not full is the last one
    }
}

__global__ void k_jd_check(const jd_u64 *out, JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ctl->nsub_total) return;
    const jd_u64 o = out[j];
    if (JD_IS_INVALID(o)) atomicMin(&ctl->errkey, (jd_u64)j << 2 | (o == JD_INVALID_CODE ? 1u : 2u));
}

// pre = exclusive scan of cnt: every interval must start at the block the frame says, and the total must be the frame's
__global__ void k_jd_verify(const unsigned int *pre, const unsigned int *suboff, JdGeo g, JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (ctl->errkey != ~0ull) {
        if (i == 0) jd_fail(ctl, (ctl->errkey & 3) == 1 ? LARS_JPGD_CODE : LARS_JPGD_COEF, (int)min(ctl->errkey >> 2, (jd_u64)0x7FFFFFFF));
        return;
    }
    if (i >= g.nint) return;
    const unsigned int want = i * g.ri * (unsigned int)g.bpm;
    bool bad = pre[suboff[i]] != want;
    if (i == 0) bad = bad || ctl->block_total != g.nblocks;
    if (bad) jd_fail(ctl, LARS_JPGD_BLOCKS, (int)min(ctl->block_total, 0x7FFFFFFFu));
}

__global__ __launch_bounds__(256) void k_jd_write(const JdTables *Tg, const unsigned int *words, const JdSub *subs, const jd_u64 *in,
                                                  const unsigned int *pre, int bpm, int ny, unsigned int nblocks, short *coef, JdCtl *ctl)
{
    __shared__ JdTables T;
    if (ctl->status[0]) return;
    jd_load_tables(&T, Tg);
    const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ctl->nsub_total) return;
    const JdSub s = subs[j];
    unsigned int n = 0;
    jd_run<true>(&T, words, in[j], s.end, s.iend, bpm, ny, &n, coef, pre[j], nblocks);
}

// ------------------------------------------------------------------------------------------------- DC, IDCT, colour
__global__ void k_jd_mcu_sums(const short *coef, JdGeo g, unsigned int *sums, const JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const unsigned int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= g.nmcu) return;
    const short *c = coef + (size_t)m * g.bpm * 64;
    unsigned int y = 0;
    for (int b = 0; b < g.ny; ++b) y += (unsigned int)(int)c[b * 64];
    sums[m] = y;
    for (int k = 1; k < g.ncomp; ++k) sums[(size_t)k * g.nmcu + m] = (unsigned int)(int)c[(g.ny + k - 1) * 64];
}

#define JD_F_0_298631336 2446
#define JD_F_0_390180644 3196
#define JD_F_0_541196100 4433
#define JD_F_0_765366865 6270
#define JD_F_0_899976223 7373
#define JD_F_1_175875602 9633
#define JD_F_1_501321110 12299
#define JD_F_1_847759065 15137
#define JD_F_1_961570560 16069
#define JD_F_2_053119869 16819
#define JD_F_2_562915447 20995
#define JD_F_3_072711026 25172

__device__ inline int jd_wrap16(int v) { return (int)(short)v; }
__device__ inline int jd_sat16(int v) { return min(32767, max(-32768, v)); }

// One 8-point pass of the slow-integer IDCT, x in, x out, in the arithmetic of libjpeg-turbo's SIMD jsimd_idct_islow
// (what Pillow runs; SSE2 and AVX2 give the same).  Inside the 10-bit window around the sample centre this is
// jidctint.c's jpeg_idct_islow bit for bit; outside it the SIMD code is its own rule: the inputs are 16-bit lanes, so
// the sums formed before a multiplication (x0 +- x4, x7 + x3, x5 + x1) wrap at 16 bits; every rotation is one
// multiply-add with the constants folded; 32-bit sums wrap (unsigned here); the descaled result saturates to 16 bits.
template <int SH>
__device__ inline void jd_idct8(int x[8])
{
    typedef unsigned int u;
    const u t2 = (u)(x[2] * JD_F_0_541196100) + (u)(x[6] * (JD_F_0_541196100 - JD_F_1_847759065));
    const u t3 = (u)(x[2] * (JD_F_0_541196100 + JD_F_0_765366865)) + (u)(x[6] * JD_F_0_541196100);
    const u t0 = (u)jd_wrap16(x[0] + x[4]) << 13, t1 = (u)jd_wrap16(x[0] - x[4]) << 13;
    const u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int s3 = jd_wrap16(x[7] + x[3]), s4 = jd_wrap16(x[5] + x[1]);
    const u z3 = (u)(s3 * (JD_F_1_175875602 - JD_F_1_961570560)) + (u)(s4 * JD_F_1_175875602);
    const u z4 = (u)(s3 * JD_F_1_175875602) + (u)(s4 * (JD_F_1_175875602 - JD_F_0_390180644));
    const u a0 = (u)(x[7] * (JD_F_0_298631336 - JD_F_0_899976223)) + (u)(x[1] * -JD_F_0_899976223) + z3;
    const u a1 = (u)(x[5] * (JD_F_2_053119869 - JD_F_2_562915447)) + (u)(x[3] * -JD_F_2_562915447) + z4;
    const u a2 = (u)(x[5] * -JD_F_2_562915447) + (u)(x[3] * (JD_F_3_072711026 - JD_F_2_562915447)) + z3;
    const u a3 = (u)(x[7] * -JD_F_0_899976223) + (u)(x[1] * (JD_F_1_501321110 - JD_F_0_899976223)) + z4;
    const u half = 1u << (SH - 1);
    x[0] = jd_sat16((int)(t10 + a3 + half) >> SH);
    x[7] = jd_sat16((int)(t10 - a3 + half) >> SH);
    x[1] = jd_sat16((int)(t11 + a2 + half) >> SH);
    x[6] = jd_sat16((int)(t11 - a2 + half) >> SH);
    x[2] = jd_sat16((int)(t12 + a1 + half) >> SH);
    x[5] = jd_sat16((int)(t12 - a1 + half) >> SH);
    x[3] = jd_sat16((int)(t13 + a0 + half) >> SH);
    x[4] = jd_sat16((int)(t13 - a0 + half) >> SH);
}

#define JD_WS_STRIDE 72                   // words per block in LDS: 64 + 8, so that the blocks of a wave start on different banks

__global__ __launch_bounds__(256) void k_jd_idct(const short *coef, const unsigned int *dcpre, const JdTables *Tg, JdGeo g, unsigned int first,
                                                 uint8_t *planes, const JdCtl *ctl)
{
    __shared__ int ws[32 * JD_WS_STRIDE];
    __shared__ int qt[3][64];
    if (ctl->status[0]) return;
    for (int i = threadIdx.x; i < 192; i += 256) qt[i / 64][i % 64] = Tg->qt[i / 64][i % 64];
    __syncthreads();
    const unsigned int pb = first + blockIdx.x * 32 + (threadIdx.x >> 3);   // block in plane order; first: 0, or where the chroma planes start
    const int r = threadIdx.x & 7;
    const bool live = pb < g.pblocks[3];
    int comp = 0, bx = 0, by = 0;
    int *w = ws + (threadIdx.x >> 3) * JD_WS_STRIDE;
    int x[8];
    bool ac_row = false;
    if (live) {
        comp = pb >= g.pblocks[2] ? 2 : pb >= g.pblocks[1] ? 1 : 0;
        const unsigned int local = pb - g.pblocks[comp];
        const int hs = comp == 0 ? g.hs : 1, vs = comp == 0 ? g.vs : 1;
        const int bw = g.mcux * hs;
        by = (int)(local / bw);
        bx = (int)(local % bw);
        const unsigned int m = (unsigned int)(by / vs) * g.mcux + (unsigned int)(bx / hs);
        const int inner = comp == 0 ? (by % vs) * hs + (bx % hs) : g.ny + comp - 1;
        const size_t blk = (size_t)m * g.bpm + inner;
        const uint4 raw = *reinterpret_cast<const uint4 *>(coef + blk * 64 + r * 8);   // row r: 8 coefficients
        const unsigned int rw[4] = {raw.x, raw.y, raw.z, raw.w};
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = (int)(short)(rw[i] & 0xFFFF);
            x[2 * i + 1] = (int)(short)(rw[i] >> 16);
        }
        if (r == 0) {                                     // the DC: differences summed from the start of the restart interval
            const unsigned int m0 = m / g.ri * g.ri;
            const unsigned int *P = dcpre + (size_t)comp * g.nmcu;
            unsigned int dc = P[m] - P[m0];
            const short *mc = coef + (size_t)m * g.bpm * 64;
            if (comp == 0) for (int b = 0; b <= inner; ++b) dc += (unsigned int)(int)mc[b * 64];
            else dc += (unsigned int)(int)mc[inner * 64];
            x[0] = (int)(short)dc;
        }
        for (int i = 0; i < 8; ++i) {
            ac_row = ac_row || (r > 0 && x[i] != 0);
            w[r * 8 + i] = jd_wrap16(x[i] * qt[comp][r * 8 + i]);   // the product keeps its low 16 bits
        }
    }
    // a block whose rows 1-7 are all zero takes the SIMD code's short cut in the column pass: DC * 4, wrapping at 16 bits
    const bool dc_only = ((__ballot(ac_row) >> (threadIdx.x & 56)) & 0xFFull) == 0;
    __syncthreads();
    if (live) {
        for (int i = 0; i < 8; ++i) x[i] = w[i * 8 + r];  // column r
        if (dc_only) {
            const int v = jd_wrap16((int)((unsigned int)x[0] << 2));
            for (int i = 0; i < 8; ++i) x[i] = v;
        } else {
            jd_idct8<11>(x);
        }
    }
    __syncthreads();
    if (live) for (int i = 0; i < 8; ++i) w[i * 8 + r] = x[i];
    __syncthreads();
    if (live) {
        for (int i = 0; i < 8; ++i) x[i] = w[r * 8 + i];  // row r
        jd_idct8<18>(x);
        unsigned int lo = 0, hi = 0;
        for (int i = 0; i < 8; ++i) {
            const int v = min(127, max(-128, x[i])) + 128;  // packed with signed saturation to 8 bits, then centred
            if (i < 4) lo |= (unsigned int)v << (8 * i); else hi |= (unsigned int)v << (8 * (i - 4));
        }
        uint8_t *dst = planes + g.poff[comp] + (size_t)(by * 8 + r) * g.pw[comp] + bx * 8;   // plane widths are multiples of 8
        *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
    }
}

__device__ inline int jd_chroma(const uint8_t *P, int pw, int cw, int chh, int hs, int vs, int x, int y)
{
    if (hs == 1) return P[(size_t)y * pw + x];
    const int cx = x >> 1;
    if (cw <= 2) return P[(size_t)(vs == 2 ? y >> 1 : y) * pw + cx];        // libjpeg replicates narrow planes
    if (vs == 1) {
        const int a = P[(size_t)y * pw + cx];
        if (x & 1) return cx == cw - 1 ? a : (3 * a + P[(size_t)y * pw + cx + 1] + 2) >> 2;
        return cx == 0 ? a : (3 * a + P[(size_t)y * pw + cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const int fy = (y & 1) ? min(cy + 1, chh - 1) : max(cy - 1, 0);
    const uint8_t *n = P + (size_t)cy * pw, *f = P + (size_t)fy * pw;
    const int t = 3 * n[cx] + f[cx];
    if (x & 1) return cx == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * n[cx + 1] + f[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * n[cx - 1] + f[cx - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void k_jd_color(const uint8_t *planes, JdGeo g, uint8_t *out, const JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const long long n = (long long)g.w * g.h;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / g.w), x = (int)(p % g.w);
        const int Y = planes[g.poff[0] + (size_t)y * g.pw[0] + x];
        if (g.ncomp == 1) {
            out[p] = (uint8_t)Y;
            continue;
        }
        const int cw = (g.w + g.hs - 1) / g.hs, chh = (g.h + g.vs - 1) / g.vs;
        const int cb = jd_chroma(planes + g.poff[1], g.pw[1], cw, chh, g.hs, g.vs, x, y) - 128;
        const int cr = jd_chroma(planes + g.poff[2], g.pw[2], cw, chh, g.hs, g.vs, x, y) - 128;
        const int R = Y + ((91881 * cr + 32768) >> 16);
        const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        const int B = Y + ((116130 * cb + 32768) >> 16);
        out[p * 3] = (uint8_t)min(255, max(0, R));
        out[p * 3 + 1] = (uint8_t)min(255, max(0, G));
        out[p * 3 + 2] = (uint8_t)min(255, max(0, B));
    }
}

// ------------------------------------------------------------------------------------------------- scaled decoding
// libjpeg's reduced-size IDCTs (jidctred.c), restated in the arithmetic of libjpeg-turbo's SIMD code for 4 x 4 and 2 x 2 and
// of its C code for 1 x 1 -- what Pillow runs after draft().  tests/jpeg_scaled_model.py is the same in NumPy.
#define JD_R_1_847759065 15137
#define JD_R_0_765366865 6270
#define JD_R_0_211164243 1730
#define JD_R_1_451774981 11893
#define JD_R_2_172734803 17799
#define JD_R_1_061594337 8697
#define JD_R_0_509795579 4176
#define JD_R_0_601344887 4926
#define JD_R_0_899976223 7373
#define JD_R_2_562915447 20995
#define JD_R_0_720959822 5906
#define JD_R_0_850430095 6967
#define JD_R_1_272758580 10426
#define JD_R_3_624509785 29692

struct JdBlockAt {
    int comp, bx, by, inner;              // component, block position in its plane, block inside the MCU
    unsigned int m;                       // MCU
    size_t blk;                           // block in scan order
};

// where block pb (plane order) lies, as k_jd_idct works it out
__device__ inline JdBlockAt jd_block_at(const JdGeo &g, unsigned int pb)
{
    JdBlockAt a;
    a.comp = pb >= g.pblocks[2] ? 2 : pb >= g.pblocks[1] ? 1 : 0;
    const unsigned int local = pb - g.pblocks[a.comp];
    const int hs = a.comp == 0 ? g.hs : 1, vs = a.comp == 0 ? g.vs : 1;
    const int bw = g.mcux * hs;
    a.by = (int)(local / bw);
    a.bx = (int)(local % bw);
    a.m = (unsigned int)(a.by / vs) * g.mcux + (unsigned int)(a.bx / hs);
    a.inner = a.comp == 0 ? (a.by % vs) * hs + (a.bx % hs) : g.ny + a.comp - 1;
    a.blk = (size_t)a.m * g.bpm + a.inner;
    return a;
}

// the DC of that block: differences summed from the start of the restart interval, in 16 bits
__device__ inline int jd_block_dc(const short *coef, const unsigned int *dcpre, const JdGeo &g, const JdBlockAt &a)
{
    const unsigned int m0 = a.m / g.ri * g.ri;
    const unsigned int *P = dcpre + (size_t)a.comp * g.nmcu;
    unsigned int dc = P[a.m] - P[m0];
    const short *mc = coef + (size_t)a.m * g.bpm * 64;
    if (a.comp == 0) for (int b = 0; b <= a.inner; ++b) dc += (unsigned int)(int)mc[b * 64];
    else dc += (unsigned int)(int)mc[a.inner * 64];
    return (int)(short)dc;
}

// The 4-point pass: x[4] is not read.  Every product is exact (16-bit input, 15-bit constant), the 32-bit sums wrap,
// the descaled result saturates to 16 bits (the SIMD code packs it).
template <int SH>
__device__ inline void jd_idct4(const int x[8], int y[4])
{
    typedef unsigned int u;
    const u t0 = (u)x[0] << 14;
    const u t2 = (u)(x[2] * JD_R_1_847759065) + (u)(x[6] * -JD_R_0_765366865);
    const u a0 = (u)(x[7] * -JD_R_0_211164243) + (u)(x[5] * JD_R_1_451774981) + (u)(x[3] * -JD_R_2_172734803) + (u)(x[1] * JD_R_1_061594337);
    const u a2 = (u)(x[7] * -JD_R_0_509795579) + (u)(x[5] * -JD_R_0_601344887) + (u)(x[3] * JD_R_0_899976223) + (u)(x[1] * JD_R_2_562915447);
    const u half = 1u << (SH - 1);
    y[0] = jd_sat16((int)(t0 + t2 + a2 + half) >> SH);
    y[3] = jd_sat16((int)(t0 + t2 - a2 + half) >> SH);
    y[1] = jd_sat16((int)(t0 - t2 + a0 + half) >> SH);
    y[2] = jd_sat16((int)(t0 - t2 - a0 + half) >> SH);
}

// The 2-point pass over entries 0, 1, 3, 5, 7 (x1 .. x7: 16-bit values; t10: entry 0 shifted up by 15, which in the row pass
// wraps at 32 bits).  The results are 32-bit numbers.
template <int SH>
__device__ inline void jd_idct2(unsigned int t10, int x1, int x3, int x5, int x7, int y[2])
{
    typedef unsigned int u;
    const u t0 = (u)(x7 * -JD_R_0_720959822) + (u)(x5 * JD_R_0_850430095) + (u)(x3 * -JD_R_1_272758580) + (u)(x1 * JD_R_3_624509785);
    const u half = 1u << (SH - 1);
    y[0] = (int)(t10 + t0 + half) >> SH;
    y[1] = (int)(t10 - t0 + half) >> SH;
}

#define JD_RS_BLOCKS 64                   // blocks per workgroup, four lanes each: 16 blocks per wave
#define JD_RS_IN 68                       // words per block of dequantised coefficients in LDS: 64 + 4.  The lanes of a wave read
                                          // column c of their blocks at word 68 b + 8 i + c (+ lane): banks 4 b + lane, all 32 twice
#define JD_RS_MID 36                      // words per block of column results, rows 9 words apart: a lane reads its row at
                                          // 36 b + 9 lane + c, banks 4 b + 9 lane: all 32 twice again

// Blocks first .. last - 1 (plane order) of components whose blocks become S x S samples, S = 4 or 2.  Lane l of a block
// loads the coefficient rows a size reads (4 x 4: 0-3 and 5-7, lane 0 one row, the others two; 2 x 2: 0, 1, 3, 5, 7),
// dequantises them into LDS, runs the column pass of one or two columns and the row pass of one row, and stores S bytes.
// Planes are pw = (blocks across) * S bytes wide and start at multiples of 16 bytes (jd_plan), so the stores are aligned.
template <int S>
__global__ __launch_bounds__(256) void k_jd_idct_reduced(const short *coef, const unsigned int *dcpre, const JdTables *Tg, JdGeo g,
                                                         unsigned int first, unsigned int last, uint8_t *planes, const JdCtl *ctl)
{
    static_assert(S == 4 || S == 2, "4 x 4 and 2 x 2; 8 x 8 is k_jd_idct, 1 x 1 k_jd_idct_dc");
    __shared__ int win[JD_RS_BLOCKS * JD_RS_IN];
    __shared__ int mid[JD_RS_BLOCKS * JD_RS_MID];
    __shared__ int qt[3][64];
    if (ctl->status[0]) return;
    for (int i = threadIdx.x; i < 192; i += 256) qt[i / 64][i % 64] = Tg->qt[i / 64][i % 64];
    __syncthreads();
    const unsigned int pb = first + blockIdx.x * JD_RS_BLOCKS + (threadIdx.x >> 2);
    const int l = threadIdx.x & 3;
    const bool live = pb < last;
    int *wi = win + (threadIdx.x >> 2) * JD_RS_IN, *wm = mid + (threadIdx.x >> 2) * JD_RS_MID;
    JdBlockAt a{};
    bool ac = false;
    if (live) {
        a = jd_block_at(g, pb);
        // 4 x 4: rows l and, but for lane 0, l + 4.  2 x 2: rows 0 | 1, 5 | 3 | 7.
        const int r0 = S == 4 ? l : (l == 0 ? 0 : l == 1 ? 1 : l == 2 ? 3 : 7);
        const int r1 = S == 4 ? (l ? l + 4 : -1) : (l == 1 ? 5 : -1);
        for (int k = 0; k < 2; ++k) {
            const int r = k ? r1 : r0;
            if (r < 0) continue;
            const uint4 raw = *reinterpret_cast<const uint4 *>(coef + a.blk * 64 + r * 8);
            const unsigned int rw[4] = {raw.x, raw.y, raw.z, raw.w};
            int x[8];
            for (int i = 0; i < 4; ++i) {
                x[2 * i] = (int)(short)(rw[i] & 0xFFFF);
                x[2 * i + 1] = (int)(short)(rw[i] >> 16);
            }
            if (r == 0) x[0] = jd_block_dc(coef, dcpre, g, a);
            for (int i = 0; i < 8; ++i) {
                ac = ac || (r > 0 && x[i] != 0);
                wi[r * 8 + i] = jd_wrap16(x[i] * qt[a.comp][r * 8 + i]);   // the product keeps its low 16 bits
            }
        }
    }
    // 4 x 4: a block whose rows 1-3 and 5-7 are all zero takes the SIMD code's short cut in the column pass: row 0 * 4, wrapping at 16 bits
    const bool cut = S == 4 && ((__ballot(ac) >> (threadIdx.x & 60)) & 0xFull) == 0;
    __syncthreads();
    if (live) {
        if (S == 4) {
            for (int c = l; c < 8; c += 4) {
                if (c == 4) continue;                     // column 4 is never read by the row pass
                int x[8], y[4];
                for (int i = 0; i < 8; ++i) x[i] = i == 4 ? 0 : wi[i * 8 + c];
                if (cut) y[0] = y[1] = y[2] = y[3] = jd_wrap16((int)((unsigned int)x[0] << 2));
                else jd_idct4<12>(x, y);
                for (int i = 0; i < 4; ++i) wm[i * 9 + c] = y[i];
            }
        } else {
            for (int k = 0; k < 2; ++k) {                 // columns 0 | 1 | 3 | 5, 7
                const int c = k ? 7 : (l == 0 ? 0 : 2 * l - 1);
                if (k && l != 3) continue;
                int y[2];
                jd_idct2<13>((unsigned int)wi[c] << 15, wi[8 + c], wi[24 + c], wi[40 + c], wi[56 + c], y);
                wm[c] = y[0];
                wm[9 + c] = y[1];
            }
        }
    }
    __syncthreads();
    if (live && l < S) {                                  // row l of the block
        const int *row = wm + l * 9;
        uint8_t *dst = planes + g.poff[a.comp] + (size_t)(a.by * S + l) * g.pw[a.comp] + a.bx * S;
        if (S == 4) {
            int x[8], y[4];
            for (int i = 0; i < 8; ++i) x[i] = i == 4 ? 0 : row[i];
            jd_idct4<19>(x, y);
            unsigned int v = 0;
            for (int i = 0; i < 4; ++i) v |= (unsigned int)(min(127, max(-128, y[i])) + 128) << (8 * i);   // signed saturation to 8 bits, then centred
            *reinterpret_cast<unsigned int *>(dst) = v;
        } else {
            int y[2];                                     // column 0 stays a 32-bit number, the others were packed to 16 bits with saturation
            jd_idct2<20>((unsigned int)row[0] << 15, jd_sat16(row[1]), jd_sat16(row[3]), jd_sat16(row[5]), jd_sat16(row[7]), y);
            const unsigned int v = (unsigned int)(min(127, max(-128, y[0])) + 128) | (unsigned int)(min(127, max(-128, y[1])) + 128) << 8;
            *reinterpret_cast<unsigned short *>(dst) = (unsigned short)v;
        }
    }
}

// 1 x 1: libjpeg's C code.  The quantiser is a signed 16-bit number there, the product is exact, and the result goes
// through the range-limit table, which takes its index modulo 1024: 0-127 -> 128-255, 128-511 -> 255, 512-895 -> 0, 896-1023 -> 0-127.
__global__ __launch_bounds__(256) void k_jd_idct_dc(const short *coef, const unsigned int *dcpre, const JdTables *Tg, JdGeo g, unsigned int first,
                                                    unsigned int last, uint8_t *planes, const JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const unsigned int pb = first + blockIdx.x * 256 + threadIdx.x;
    if (pb >= last) return;
    const JdBlockAt a = jd_block_at(g, pb);
    const int v = (jd_block_dc(coef, dcpre, g, a) * (int)(short)Tg->qt[a.comp][0] + 4) >> 3;
    const int i = v & 1023;
    planes[g.poff[a.comp] + (size_t)a.by * g.pw[a.comp] + a.bx] = (uint8_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

// One thread per pixel of the scaled picture (g.w x g.h, planes as jd_plan lays them out for the scale).  hf: how many
// pixels a chroma sample covers horizontally (2 for 4:2:2, 1 else; vertically it is always 1: the chroma blocks of 4:2:0
// are twice the luma's size).  fancy: libjpeg's h2v1 triangle filter (jd_chroma), which libjpeg-turbo leaves out at 1/8.
__global__ __launch_bounds__(256) void k_jd_color_scaled(const uint8_t *planes, JdGeo g, int hf, int fancy, uint8_t *out, const JdCtl *ctl)
{
    if (ctl->status[0]) return;
    const long long n = (long long)g.w * g.h;
    const int cw = (g.w + hf - 1) / hf;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
        const int y = (int)(p / g.w), x = (int)(p % g.w);
        const int Y = planes[g.poff[0] + (size_t)y * g.pw[0] + x];
        if (g.ncomp == 1) {
            out[p] = (uint8_t)Y;
            continue;
        }
        int c[2];
        for (int k = 0; k < 2; ++k) {
            const uint8_t *P = planes + g.poff[1 + k];
            const int pw = g.pw[1 + k];
            c[k] = (hf == 1 ? P[(size_t)y * pw + x] : fancy ? jd_chroma(P, pw, cw, g.h, 2, 1, x, y) : P[(size_t)y * pw + (x >> 1)]) - 128;
        }
        const int cb = c[0], cr = c[1];
        const int R = Y + ((91881 * cr + 32768) >> 16);
        const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        const int B = Y + ((116130 * cb + 32768) >> 16);
        out[p * 3] = (uint8_t)min(255, max(0, R));
        out[p * 3 + 1] = (uint8_t)min(255, max(0, G));
        out[p * 3 + 2] = (uint8_t)min(255, max(0, B));
    }
}

// ------------------------------------------------------------------------------------------------- host side
// lars_jpeg_info's info[] by name (sampling: component 0's, the others are checked to be 1 x 1)
struct JpegInfo {
    int64_t w, h, ncomp, hs0, vs0, ri, eoff, elen, supported, reason;
    explicit JpegInfo(const int64_t *i)
        : w(i[LARS_JPEG_INFO_WIDTH]), h(i[LARS_JPEG_INFO_HEIGHT]), ncomp(i[LARS_JPEG_INFO_COMPONENTS]), hs0(i[LARS_JPEG_INFO_H0]),
          vs0(i[LARS_JPEG_INFO_V0]), ri(i[LARS_JPEG_INFO_RESTART_INTERVAL]), eoff(i[LARS_JPEG_INFO_ENTROPY_OFFSET]),
          elen(i[LARS_JPEG_INFO_ENTROPY_BYTES]), supported(i[LARS_JPEG_INFO_SUPPORTED]), reason(i[LARS_JPEG_INFO_REASON])
    {
    }
};

// geometry and the device scratch of one file: what lars_jpeg_decode_scratch_bytes counts and lars_d_decode_jpeg_u8 points into
// At scale 2, 4 or 8 (m = 8 / scale) gs is g with the picture and the planes of that scale: the picture is ceil(w / scale) x
// ceil(h / scale); a block of component c becomes bs[c] samples wide and high -- m, doubled while it is below 8 and both
// hmax * m and vmax * m stay multiples of h_c * bs * 2 and v_c * bs * 2 (libjpeg's rule: m for luma and for the chroma of
// 4:2:2, 2 m for the chroma of 4:2:0) -- so plane c is (blocks across) * bs[c] bytes wide, (blocks down) * bs[c] rows high,
// and every plane starts at a multiple of 16 bytes.  hf = 2 where the chroma planes are half as wide as the picture.
struct JdPlan {
    JdGeo g, gs;
    int scale, bs[3], hf;
    jd_u64 elen, nwg, nsub_cap;
    unsigned int sbits;
    JdCtl *ctl;
    JdTables *tables;
    unsigned int *keepcnt, *markcnt, *nsubs, *suboff, *cnt, *pre, *sums;
    uint8_t *compact, *planes;
    jd_u64 *cbyte, *in, *out;
    JdSub *subs;
    short *coef;
};

// false for what the decoder does not take
static bool jd_plan(const JpegInfo &I, int sbits, int scale, Carver &cv, JdPlan *Lp)
{
    JdPlan L{};
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return false;
    const int64_t w = I.w, h = I.h, nc = I.ncomp;
    if (!I.supported || w < 1 || h < 1 || w > 65535 || h > 65535 || (nc != 1 && nc != 3) || h * w * nc >= (1ll << 31)) return false;
    if (I.eoff < 0 || I.elen < 0 || I.elen > (1ll << 40) || I.ri < 0 || I.ri > 65535) return false;
    const int hs = nc == 1 ? 1 : (int)I.hs0, vs = nc == 1 ? 1 : (int)I.vs0;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    JdGeo &g = L.g;
    g.w = (int)w; g.h = (int)h; g.ncomp = (int)nc; g.hs = hs; g.vs = vs;
    g.ny = hs * vs;
    g.bpm = g.ny + (int)nc - 1;
    g.mcux = (int)((w + 8 * hs - 1) / (8 * hs));
    g.mcuy = (int)((h + 8 * vs - 1) / (8 * vs));
    g.nmcu = (unsigned int)g.mcux * g.mcuy;
    g.nblocks = g.nmcu * g.bpm;
    g.ri = I.ri > 0 && (unsigned int)I.ri < g.nmcu ? (unsigned int)I.ri : g.nmcu;
    g.nint = (g.nmcu + g.ri - 1) / g.ri;
    unsigned int off = 0, blocks = 0;
    for (int c = 0; c < 3; ++c) {
        g.pblocks[c] = blocks;
        if (c >= nc) { g.pw[c] = g.ph[c] = 0; g.poff[c] = off; continue; }
        g.pw[c] = g.mcux * (c == 0 ? hs : 1) * 8;
        g.ph[c] = g.mcuy * (c == 0 ? vs : 1) * 8;
        g.poff[c] = off;
        off += (unsigned int)g.pw[c] * g.ph[c];           // < 2^32: each plane is at most 65536^2 / 1, checked by h * w * nc above
        blocks += (unsigned int)(g.pw[c] / 8) * (g.ph[c] / 8);
    }
    g.pblocks[3] = blocks;
    L.scale = scale;
    L.gs = g;
    L.hf = 1;
    for (int c = 0; c < 3; ++c) L.bs[c] = 8;
    if (scale > 1) {
        const int m = 8 / scale;
        JdGeo &gs = L.gs;
        gs.w = (int)((w + scale - 1) / scale);
        gs.h = (int)((h + scale - 1) / scale);
        off = 0;
        for (int c = 0; c < nc; ++c) {
            const int hc = c == 0 ? hs : 1, vc = c == 0 ? vs : 1;
            int s = m;
            while (s < 8 && (hs * m) % (hc * s * 2) == 0 && (vs * m) % (vc * s * 2) == 0) s *= 2;
            L.bs[c] = s;
            gs.pw[c] = g.mcux * hc * s;
            gs.ph[c] = g.mcuy * vc * s;
            gs.poff[c] = off;
            off += ((unsigned int)gs.pw[c] * gs.ph[c] + 15u) & ~15u;    // no larger than at full scale
        }
        for (int c = (int)nc; c < 3; ++c) gs.poff[c] = off;
        if (nc == 3) L.hf = hs * m / L.bs[1];
    }
    L.elen = (jd_u64)I.elen;
    L.sbits = (unsigned int)sbits;
    L.nwg = (L.elen + JD_MARK_THREADS - 1) / JD_MARK_THREADS;
    L.nsub_cap = L.elen * 8 / L.sbits + g.nint + 1;
    if (L.nsub_cap >= (1ull << 31) || L.nwg >= (1ull << 31)) return false;
    L.ctl = cv.take<JdCtl>(1);
    L.tables = cv.take<JdTables>(1);
    L.keepcnt = cv.take<unsigned int>(L.nwg + 1);
    L.markcnt = cv.take<unsigned int>(L.nwg + 1);
    L.compact = cv.take<uint8_t>(L.elen + 16);
    L.cbyte = cv.take<jd_u64>((size_t)g.nint + 1);
    L.nsubs = cv.take<unsigned int>((size_t)g.nint + 1);
    L.suboff = cv.take<unsigned int>((size_t)g.nint + 1);
    L.subs = cv.take<JdSub>(L.nsub_cap);
    L.in = cv.take<jd_u64>(L.nsub_cap);
    L.out = cv.take<jd_u64>(L.nsub_cap);
    L.cnt = cv.take<unsigned int>(L.nsub_cap);
    L.pre = cv.take<unsigned int>(L.nsub_cap);
    L.coef = cv.take<short>((size_t)g.nblocks * 64);
    L.sums = cv.take<unsigned int>((size_t)g.nmcu * 3);
    L.planes = cv.take<uint8_t>((size_t)off);
    *Lp = L;
    return true;
}

static int jd_status_fail(const char *who, const int st[2])
{
    switch (st[0]) {
    case LARS_JPGD_RESTART: return fail(LARS_ERR_INVALID, "%s: a restart marker is missing or out of sequence (%d found)", who, st[1]);
    case LARS_JPGD_CODE: return fail(LARS_ERR_INVALID, "%s: entropy data holds a bit pattern that is no Huffman code of its table (subsequence %d)", who, st[1]);
    case LARS_JPGD_COEF: return fail(LARS_ERR_INVALID, "%s: entropy data runs past coefficient 63 of a block (subsequence %d)", who, st[1]);
    case LARS_JPGD_BLOCKS: return fail(LARS_ERR_INVALID, "%s: entropy data does not hold the frame's blocks (it ends early or is damaged; %d blocks found)", who, st[1]);
    default: return fail(LARS_ERR_HIP, "%s: internal decoder status %d (%d)", who, st[0], st[1]);
    }
}

static const char *jd_reason(int64_t r)
{
    switch (r) {
    case LARS_JPEG_REASON_PROGRESSIVE: return "progressive";
    case LARS_JPEG_REASON_FRAME: return "lossless, arithmetic-coded or hierarchical";
    case LARS_JPEG_REASON_PRECISION: return "not 8-bit";
    case LARS_JPEG_REASON_SCANS: return "multi-scan";
    case LARS_JPEG_REASON_COMPONENTS: return "2- or 4-component (CMYK / YCCK)";
    case LARS_JPEG_REASON_COLORSPACE: return "RGB-stored";
    case LARS_JPEG_REASON_SAMPLING: return "unusually sampled";
    case LARS_JPEG_REASON_DNL: return "DNL";
    case LARS_JPEG_REASON_SIZE: return "too large";
    default: return "these";
    }
}

// the JPEG side of the host entry points (codec_host.h)
struct JdFile : HostFile {
    int64_t info[LARS_JPEG_INFO_N];
    JdCtl ctl;
    int scale = 1;                        // 2, 4, 8: h and w are the scaled picture's

    int parse(const char *who_, const uint8_t *file_, int64_t len_)
    {
        who = who_; file = file_; len = len_;
        if (!file || len <= 0) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
        LARS_TRY(lars_jpeg_info(file, len, info));
        const JpegInfo I(info);
        if (!I.supported) return fail(LARS_ERR_UNSUPPORTED, "%s: %s JPEG files are not supported", who, jd_reason(I.reason));
        if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return fail(LARS_ERR_INVALID, "%s: scale 1, 2, 4 or 8, got %d", who, scale);
        h = (I.h + scale - 1) / scale; w = (I.w + scale - 1) / scale; channels = (int)I.ncomp;
        extra_bytes = 0;
        scratch_bytes = lars_jpeg_decode_scaled_scratch_bytes(info, scale);
        return LARS_OK;
    }
    int enqueue(hipStream_t s)
    {
        LARS_TRY(lars_d_decode_jpeg_scaled_u8(d_file, file, info, scale, d_img, d_status, d_scratch, s));
        // the control block opens the scratch: the rounds that decoded anything
        LARS_HIP_TRY(hipMemcpyAsync(&ctl, d_scratch, sizeof ctl, hipMemcpyDeviceToHost, s));
        return LARS_OK;
    }
    int finish(const int st[2])
    {
        if (st[0]) return jd_status_fail(who, st);
        int rounds = 1;
        for (int r = 1; r <= JD_ROUNDS; ++r) rounds += ctl.changed[r] != 0;
        tuning().jpeg_last_rounds = rounds + (ctl.changed[JD_ROUNDS] != 0 ? 100 : 0);
        return LARS_OK;
    }
};

}  // namespace lars

using namespace lars;

extern "C" {

size_t lars_jpeg_decode_scratch_bytes(const int64_t info[LARS_JPEG_INFO_N]) { return lars_jpeg_decode_scaled_scratch_bytes(info, 1); }

size_t lars_jpeg_decode_scaled_scratch_bytes(const int64_t info[LARS_JPEG_INFO_N], int scale)
{
    JdPlan L;
    Carver size(nullptr);
    if (!info || !jd_plan(JpegInfo(info), tuning().jpeg_subseq_bits, scale, size, &L)) return 0;
    return size.bytes();
}

}  // extern "C"

// lars_d_decode_jpeg_u8 (scale 1) and lars_d_decode_jpeg_scaled_u8
static int jd_enqueue(const char *who, const uint8_t *file_dev, const uint8_t *head, const int64_t info[LARS_JPEG_INFO_N], int scale, uint8_t *out,
                      int32_t *status_dev, void *scratch, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!file_dev || !head || !info || !out || !status_dev || !scratch) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    const JpegInfo I(info);
    JdPlan L;
    Carver cv(scratch);
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return fail(LARS_ERR_INVALID, "%s: scale 1, 2, 4 or 8, got %d", who, scale);
    if (!jd_plan(I, tuning().jpeg_subseq_bits, scale, cv, &L)) return fail(LARS_ERR_INVALID, "%s: info describes no file this decoder takes", who);
    JpegHeader H;
    LARS_TRY(jpeg_parse(head, I.eoff, &H, false));
    if (!H.supported || H.w != I.w || H.h != I.h || H.ncomp != I.ncomp || H.eoff != I.eoff || H.ri != I.ri ||
        (H.ncomp == 3 && (H.hs[0] != I.hs0 || H.vs[0] != I.vs0)))
        return fail(LARS_ERR_INVALID, "%s: head and info do not describe the same file", who);
    JdTablesArg A;
    memset(&A, 0, sizeof A);
    for (int k = 0; k < H.ncomp; ++k) {
        memcpy(A.qt[k], H.qt[H.tq[k]], sizeof A.qt[k]);
        memcpy(A.hcount[k], H.hcount[H.td[k]], 16);
        memcpy(A.hval[k], H.hval[H.td[k]], 256);
        memcpy(A.hcount[3 + k], H.hcount[4 + H.ta[k]], 16);
        memcpy(A.hval[3 + k], H.hval[4 + H.ta[k]], 256);
    }
    const JdGeo &g = L.g;
    JdCtl *ctl = L.ctl;
    const unsigned int *words = reinterpret_cast<const unsigned int *>(L.compact);
    const uint8_t *seg = file_dev + I.eoff;
    const long long elen = (long long)L.elen;
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(JdCtl), s));
    LARS_HIP_TRY(hipMemsetAsync(&ctl->errkey, 0xFF, sizeof(jd_u64), s));
    LARS_HIP_TRY(hipMemsetAsync(L.coef, 0, (size_t)g.nblocks * 128, s));
    LARS_HIP_TRY(hipMemsetAsync(L.cnt, 0, (size_t)L.nsub_cap * 4, s));       // the scan of the counts runs over the whole capacity
    hipLaunchKernelGGL(k_jd_setup, dim3(1), dim3(64), 0, s, A, L.tables);
    if (L.nwg) {
        hipLaunchKernelGGL(k_jd_mark, dim3((unsigned)L.nwg), dim3(JD_MARK_THREADS), 0, s, seg, elen, L.keepcnt, L.markcnt);
        hipLaunchKernelGGL(k_jd_exscan, dim3(1), dim3(1024), 0, s, L.keepcnt, L.keepcnt, (long long)L.nwg, 0ll, &ctl->kept_total);
        hipLaunchKernelGGL(k_jd_exscan, dim3(1), dim3(1024), 0, s, L.markcnt, L.markcnt, (long long)L.nwg, 0ll, &ctl->mark_total);
        hipLaunchKernelGGL(k_jd_compact, dim3((unsigned)L.nwg), dim3(JD_MARK_THREADS), 0, s, seg, elen, L.keepcnt, L.markcnt, g.nint, L.compact, L.cbyte, ctl);
    }
    hipLaunchKernelGGL(k_jd_intervals, dim3((g.nint + 255) / 256), dim3(256), 0, s, L.cbyte, g.nint, L.sbits, L.nsubs, ctl);
    hipLaunchKernelGGL(k_jd_exscan, dim3(1), dim3(1024), 0, s, L.nsubs, L.suboff, (long long)g.nint, 0ll, &ctl->nsub_total);
    const unsigned int sgrid = (unsigned int)((L.nsub_cap + 255) / 256);
    hipLaunchKernelGGL(k_jd_subs, dim3(sgrid), dim3(256), 0, s, L.cbyte, L.suboff, g.nint, L.sbits, (unsigned int)L.nsub_cap, L.subs, ctl);
    for (int r = 0; r <= JD_ROUNDS; ++r)
        hipLaunchKernelGGL(k_jd_pass, dim3(sgrid), dim3(256), 0, s, L.tables, words, L.subs, L.in, L.out, L.cnt, r, g.bpm, g.ny, ctl);
    hipLaunchKernelGGL(k_jd_finish, dim3(1), dim3(64), 0, s, L.tables, words, L.subs, L.in, L.out, L.cnt, g.bpm, g.ny, ctl);
    hipLaunchKernelGGL(k_jd_check, dim3(sgrid), dim3(256), 0, s, L.out, ctl);
    hipLaunchKernelGGL(k_jd_exscan, dim3(1), dim3(1024), 0, s, L.cnt, L.pre, (long long)L.nsub_cap, 0ll, &ctl->block_total);
    hipLaunchKernelGGL(k_jd_verify, dim3((g.nint + 255) / 256), dim3(256), 0, s, L.pre, L.suboff, g, ctl);
    hipLaunchKernelGGL(k_jd_write, dim3(sgrid), dim3(256), 0, s, L.tables, words, L.subs, L.in, L.pre, g.bpm, g.ny, g.nblocks, L.coef, ctl);
    hipLaunchKernelGGL(k_jd_mcu_sums, dim3((g.nmcu + 255) / 256), dim3(256), 0, s, L.coef, g, L.sums, ctl);
    hipLaunchKernelGGL(k_jd_exscan, dim3((unsigned)g.ncomp), dim3(1024), 0, s, L.sums, L.sums, (long long)g.nmcu, (long long)g.nmcu, (unsigned int *)nullptr);
    if (scale == 1) {
        hipLaunchKernelGGL(k_jd_idct, dim3((g.pblocks[3] + 31) / 32), dim3(256), 0, s, L.coef, L.sums, L.tables, g, 0u, L.planes, ctl);
        const long long npix = (long long)g.w * g.h;
        hipLaunchKernelGGL(k_jd_color, dim3((unsigned)std::min<long long>((npix + 255) / 256, 16384)), dim3(256), 0, s, L.planes, g, out, ctl);
    } else {
        // luma, then both chroma planes (their blocks have one size): each group with the kernel of its block size
        const JdGeo &gs = L.gs;
        for (int grp = 0; grp < (g.ncomp == 3 ? 2 : 1); ++grp) {
            const unsigned int first = g.pblocks[grp], last = grp ? g.pblocks[3] : g.pblocks[1], n = last - first;
            switch (L.bs[grp]) {
            case 8: hipLaunchKernelGGL(k_jd_idct, dim3((n + 31) / 32), dim3(256), 0, s, L.coef, L.sums, L.tables, gs, first, L.planes, ctl); break;
            case 4: hipLaunchKernelGGL(k_jd_idct_reduced<4>, dim3((n + JD_RS_BLOCKS - 1) / JD_RS_BLOCKS), dim3(256), 0, s, L.coef, L.sums, L.tables, gs, first, last, L.planes, ctl); break;
            case 2: hipLaunchKernelGGL(k_jd_idct_reduced<2>, dim3((n + JD_RS_BLOCKS - 1) / JD_RS_BLOCKS), dim3(256), 0, s, L.coef, L.sums, L.tables, gs, first, last, L.planes, ctl); break;
            default: hipLaunchKernelGGL(k_jd_idct_dc, dim3((n + 255) / 256), dim3(256), 0, s, L.coef, L.sums, L.tables, gs, first, last, L.planes, ctl); break;
            }
        }
        const long long npix = (long long)gs.w * gs.h;
        hipLaunchKernelGGL(k_jd_color_scaled, dim3((unsigned)std::min<long long>((npix + 255) / 256, 16384)), dim3(256), 0, s, L.planes, gs, L.hf,
                           scale < 8 ? 1 : 0, out, ctl);
    }
    LARS_HIP_TRY(hipMemcpyAsync(status_dev, ctl->status, 8, hipMemcpyDeviceToDevice, s));
    return launch_check(who);
}

extern "C" {

int lars_d_decode_jpeg_u8(const uint8_t *file_dev, const uint8_t *head, const int64_t info[LARS_JPEG_INFO_N], uint8_t *out,
                          int32_t *status_dev, void *scratch, void *stream)
{
    return jd_enqueue("lars_d_decode_jpeg_u8", file_dev, head, info, 1, out, status_dev, scratch, stream);
}

int lars_d_decode_jpeg_scaled_u8(const uint8_t *file_dev, const uint8_t *head, const int64_t info[LARS_JPEG_INFO_N], int scale, uint8_t *out,
                                 int32_t *status_dev, void *scratch, void *stream)
{
    return jd_enqueue("lars_d_decode_jpeg_scaled_u8", file_dev, head, info, scale, out, status_dev, scratch, stream);
}

// host file in, host pixels out: one upload, the status, one download
int lars_h_decode_jpeg_u8(const uint8_t *file, int64_t len, uint8_t *out, size_t out_cap)
{
    static const char *who = "lars_h_decode_jpeg_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    JdFile F;
    LARS_TRY(F.parse(who, file, len));
    return decode_file_to_host(c, F, out, out_cap);
}

// ... at 1/scale: out holds ceil(h / scale) * ceil(w / scale) * components bytes
int lars_h_decode_jpeg_scaled_u8(const uint8_t *file, int64_t len, int scale, uint8_t *out, size_t out_cap)
{
    static const char *who = "lars_h_decode_jpeg_scaled_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    JdFile F;
    F.scale = scale;
    LARS_TRY(F.parse(who, file, len));
    return decode_file_to_host(c, F, out, out_cap);
}

// host file in, thumbnail out: the decoded pixels go straight into the thumbnail kernels (resize.hip)
int lars_h_thumbnail_jpeg_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                             int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    static const char *who = "lars_h_thumbnail_jpeg_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out || !reduce_box || !box) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    JdFile F;
    LARS_TRY(F.parse(who, file, len));
    return thumbnail_file(c, F, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

// ... from the picture decoded at 1/scale: the plan's numbers are for that picture
int lars_h_thumbnail_jpeg_scaled_u8(const uint8_t *file, int64_t len, int scale, int fx, int fy, const int reduce_box[4], const float box[4],
                                    int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    static const char *who = "lars_h_thumbnail_jpeg_scaled_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out || !reduce_box || !box) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    JdFile F;
    F.scale = scale;
    LARS_TRY(F.parse(who, file, len));
    return thumbnail_file(c, F, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

}  // extern "C"
