// TIFF files built on the device (lars_h_encode_tiff, lars_d_encode_tiff, and their _f32 siblings for float32 samples, whose
// predictor is the floating-point one; everything but te_byte and three directory values is shared): every strip is LZW-coded by one wave into its own
// buffer, one workgroup scans the strip lengths and writes the header and the directory, and one pass moves the strips to their
// places, so that only the finished file crosses PCIe.
//
// The stream of a strip is specified before the kernel: it is the greedy encoder's (tests/lzw_writer.py, encode(data,
// clear_at=4094)), which is libtiff's.  A leading Clear; at every step the longest string the table holds; after each code the
// string plus the next byte becomes entry 258, 259, ...; once the table holds 4094 codes (3836 entries added) a Clear goes
// out and the table starts again; the last string's code, a Clear too where that code is the 3836th of its segment (libtiff
// counts it as an entry although none is added), then EndOfInformation.  Code i of a segment (the codes between two
// Clears, the Clear that ends it included) is 9 bits wide for i <= 253, 10 for i <= 765, 11 for i <= 1789, 12 after that;
// codes are packed MSB first.
//
// The string table is an open-addressed hash in LDS: 8192 slots of 32 bits, key (prefix code << 8 | byte, 20 bits) << 12 |
// code (12 bits); 0 is an empty slot (no entry has code 0).  At most 3836 slots are taken, so a probe sequence meets an
// empty slot; the 64 lanes look at 64 consecutive slots per step, so it ends after at most 8192 / 64 steps.
// tests/tiff_encode_model.py restates the phases below in NumPy and checks every index they form.
//
// Deflate (lars_*_encode_tiff_deflate*, Compression 8) replaces k_te_lzw by kernels that code a strip in parallel; the directory, the
// strip rule, the status codes and the placement of the strips are the LZW path's.  The stream of a strip, specified before the
// kernels (tests/tiff_deflate_encode_model.py builds it byte for byte): the strip has n stored bytes (after the predictor,
// little-endian) and p = ceil(n / 32768) parts.  The stream opens with 78 01.  Part i covers bytes [32768 i, min(n, 32768 (i + 1)))
// and is the block deflate_segment (deflate_device.h) writes for them -- a dynamic literal-only Huffman block, or a stored block
// where the dynamic one would not be shorter.  A dynamic block of a part that is not the last is followed by three zero bits, the
// padding to a byte and 00 00 FF FF (an empty stored block), so that every part ends on a byte boundary (a stored block does
// anyway); the last part carries BFINAL and is padded to a byte; a strip of one part is first and last at once.  The Adler-32 of
// the n bytes, big-endian, ends the stream.  The stream is a function of the strip's bytes alone.
#include <algorithm>

#include "checksum_device.h"
#include "codec_host.h"
#include "common.h"
#include "deflate_device.h"
#include "deflate_lz_device.h"

namespace lars {

namespace {

constexpr int TE_SLOTS = 8192;
constexpr int TE_CLEAR = 256, TE_EOI = 257, TE_FIRST = 258, TE_CLEAR_AT = 4094;
constexpr int TE_SEG_CODES = TE_CLEAR_AT - TE_FIRST;      // 3836 codes of a segment add the entries that fill the table
constexpr int TE_FRAME_THREADS = 1024;
constexpr int TE_PACK_THREADS = 256;
constexpr int TE_MAX_ENTRIES = 13;                        // directory entries: 11 always, Predictor, ExtraSamples

struct TeGeom {
    long long nstrips, pitch;      // pitch: bytes of one strip's buffer = te_strip_cap of a whole strip, rounded up to 4
    long long rowb;                // bytes of a row of the picture
    int width, height, spp, bps;   // bps: bytes per sample; 4: float32 (SampleFormat 3)
    int rps, predictor;            // predictor: 0 none, else horizontal differencing (2) or, for float32, the floating-point one (3)
};

// Upper bound of a strip's stream for n input bytes, its pad byte included.  Every code but the leading Clear, the Clears that
// end a segment and EndOfInformation takes at least one input byte, so there are at most n of them; a Clear follows 3836 of
// them, so there are at most n / 3836; every code is at most 12 bits wide; the last byte is filled up, and one more byte brings
// the next strip to an even offset.
__host__ __device__ inline long long te_strip_cap(long long n)
{
    const long long bytes = (12 * (n + n / TE_SEG_CODES + 2) + 7) / 8;
    return bytes + (bytes & 1);
}

__device__ inline unsigned int te_hash(unsigned int key) { return (key * 2654435761u) >> 19; }      // 13 bits

// byte B of the picture as the file stores it: the sample's byte, or with the predictor the byte of the sample minus the
// sample of the pixel to its left (the first pixel of a row as it is), little-endian.  float32 with the predictor (libtiff's
// fpDiff): the row is stored as four planes of width * spp bytes, plane 0 the most significant byte of every sample, and
// byte q of that row is its plane byte minus the plane byte spp positions earlier, which may lie in the plane before
__device__ inline unsigned int te_byte(const uint8_t *__restrict__ img, const TeGeom &g, long long B)
{
    if (!g.predictor) return img[B];
    const long long q = B % g.rowb;                       // the byte within its row
    if (g.bps == 4) {
        const uint8_t *row = img + (B - q);
        const long long wc = g.rowb >> 2;                 // samples of a row; q / wc <= 3
        const long long pl = q / wc, e = q - pl * wc;
        unsigned int v = row[4 * e + 3 - pl];
        if (q >= g.spp) {
            const long long q1 = q - g.spp, pl1 = q1 / wc, e1 = q1 - pl1 * wc;
            v -= row[4 * e1 + 3 - pl1];
        }
        return v & 255u;
    }
    if (g.bps == 1) return (unsigned int)(img[B] - (q >= g.spp ? img[B - g.spp] : 0)) & 255u;
    const uint16_t *s = reinterpret_cast<const uint16_t *>(img) + (B >> 1);       // rowb is even: B and q have the same parity
    const unsigned int v = (unsigned int)(s[0] - ((q >> 1) >= g.spp ? s[-g.spp] : 0)) & 0xFFFFu;
    return (q & 1) ? v >> 8 : v & 255u;
}

// One wave per strip.  Everything but the table probe is wave-uniform: 64 bytes are read at once (one per lane), the match
// then goes through them in order; lane 0 writes the table and the stream.
__global__ __launch_bounds__(64) void k_te_lzw(const uint8_t *__restrict__ img, TeGeom g, uint8_t *__restrict__ zbuf,
                                               unsigned int *__restrict__ zlen, int *status)
{
    __shared__ unsigned int tab[TE_SLOTS];
    const int lane = threadIdx.x;
    const long long k = blockIdx.x;
    if (k >= g.nstrips) return;
    const long long left = (long long)g.height - k * g.rps;
    const long long n = (left < g.rps ? left : (long long)g.rps) * g.rowb;        // 1 <= n <= 2^30: the host checked
    const long long base = k * g.rps * g.rowb;
    uint8_t *dst = zbuf + k * g.pitch;
    const unsigned int cap = (unsigned int)g.pitch;
    for (int q = lane; q < TE_SLOTS; q += 64) tab[q] = 0;
    __syncthreads();
    unsigned int acc = 0, op = 0;        // bits not yet written (fewer than 8 between codes), bytes written
    int nbits = 0, i = 0, nxt = TE_FIRST, w = -1;
    bool over = false;
    auto emit = [&](int code) {
        const int width = tiff_lzw_width(i);
        acc = (acc << width) | (unsigned int)code;
        nbits += width;                                   // <= 7 + 12; 7 + 12 + 9 for EndOfInformation behind the last Clear
        while (nbits >= 8) {
            nbits -= 8;
            if (op < cap) { if (lane == 0) dst[op] = (uint8_t)(acc >> nbits); }
            else over = true;
            ++op;
        }
        acc &= (1u << nbits) - 1u;
        i = code == TE_CLEAR ? 0 : i + 1;
    };
    emit(TE_CLEAR);
    for (long long t0 = 0; t0 < n; t0 += 64) {
        const long long t = t0 + lane;
        const unsigned int mine = t < n ? te_byte(img, g, base + t) : 0u;
        const int cnt = (int)(n - t0 < 64 ? n - t0 : 64);
#pragma unroll 1
        for (int u = 0; u < cnt; ++u) {
            const int byte = (int)__builtin_amdgcn_readlane(mine, u);
            if (w < 0) { w = byte; continue; }
            const unsigned int key = ((unsigned int)w << 8) | (unsigned int)byte;
            const unsigned int h0 = te_hash(key);
            int found = -1, slot_at = -1;
#pragma unroll 1
            for (int step = 0; step < TE_SLOTS / 64; ++step) {
                const unsigned int v = tab[(h0 + step * 64 + lane) & (TE_SLOTS - 1)];
                const unsigned long long m = __ballot(v == 0u || (v >> 12) == key);
                if (m) {
                    const int first = __ffsll((long long)m) - 1;
                    const unsigned int vv = __builtin_amdgcn_readlane(v, first);
                    if (vv) found = (int)(vv & 4095u);
                    else slot_at = (int)((h0 + step * 64 + first) & (TE_SLOTS - 1));
                    break;
                }
            }
            if (found >= 0) { w = found; continue; }
            emit(w);
            if (slot_at < 0) over = true;                 // no empty slot: the table never holds more than 3836 entries
            else if (lane == 0) tab[slot_at] = (key << 12) | (unsigned int)nxt;
            ++nxt;
            if (nxt >= TE_CLEAR_AT) {
                emit(TE_CLEAR);
                __syncthreads();
                for (int q = lane; q < TE_SLOTS; q += 64) tab[q] = 0;
                nxt = TE_FIRST;
            }
            __syncthreads();
            w = byte;
        }
    }
    if (w >= 0) emit(w);
    // libtiff's LZWPostEncode counts the last code as an entry: a table that is full by that count is cleared before
    // EndOfInformation.  The Clear is code 3837 of its segment, 12 bits, and goes into the accumulator in front of
    // EndOfInformation, which then has 9 bits: at most 7 + 12 + 9 bits, written by the one emit below.
    if (nxt + 1 >= TE_CLEAR_AT) {
        acc = (acc << 12) | (unsigned int)TE_CLEAR;
        nbits += 12;
        i = 0;
    }
    emit(TE_EOI);
    if (nbits) {
        if (op < cap) { if (lane == 0) dst[op] = (uint8_t)(acc << (8 - nbits)); }
        else over = true;
        ++op;
    }
    if (lane == 0) {
        if ((op & 1) && op < cap) dst[op] = 0;            // the pad byte travels with the strip
        zlen[k] = over ? 0u : op;
        if (over && atomicCAS(&status[0], LARS_TIFE_OK, LARS_TIFE_OVERFLOW) == LARS_TIFE_OK) status[1] = (int)k;
    }
}

__device__ inline void te_put16(uint8_t *p, unsigned int v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
__device__ inline void te_put32(uint8_t *p, unsigned int v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// one directory entry at p; n values of `value` (SHORT: typ 3, LONG: typ 4) inline where they fit in four bytes, else the
// offset `where` of the array; returns the entry's size
__device__ inline int te_entry(uint8_t *p, int tag, int typ, unsigned int n, unsigned int value, bool inline_ok, unsigned int where)
{
    te_put16(p, (unsigned int)tag);
    te_put16(p + 2, (unsigned int)typ);
    te_put32(p + 4, n);
    te_put32(p + 8, 0);
    if (!inline_ok) te_put32(p + 8, where);
    else if (typ == 4) te_put32(p + 8, value);
    else for (unsigned int j = 0; j < n; ++j) te_put16(p + 8 + 2 * j, value);
    return 12;
}

// The scan of the strip lengths (each rounded up to even) and everything of the file that is not strip data: the header, the
// directory (Compression: 5 or 8) in tiffio.write_tiff's order (tags ascending; arrays of more than four bytes after the directory, in the order of
// their tags), the strip offsets and byte counts, the file's length.  One workgroup.
__global__ __launch_bounds__(TE_FRAME_THREADS) void k_te_frame(TeGeom g, int compression, const unsigned int *__restrict__ zlen,
                                                              unsigned long long *__restrict__ off, uint8_t *__restrict__ out,
                                                              unsigned long long out_cap, long long *out_len, int *status)
{
    __shared__ unsigned long long s_w[TE_FRAME_THREADS / 64];
    const int tid = threadIdx.x;
    if (status[0]) {                                      // uniform: nothing has written status since k_te_lzw ended
        if (tid == 0) *out_len = 0;
        return;
    }
    const long long per = (g.nstrips + TE_FRAME_THREADS - 1) / TE_FRAME_THREADS;
    const long long lo = min(g.nstrips, tid * per), hi = min(g.nstrips, lo + per);
    unsigned long long s = 0;
    for (long long k = lo; k < hi; ++k) s += (unsigned long long)zlen[k] + (zlen[k] & 1u);
    unsigned long long strips;                            // the bytes of all strips
    const unsigned long long before = wg_exscan<TE_FRAME_THREADS>(s, s_w, &strips);
    const unsigned long long n = (unsigned long long)g.nstrips;
    const int c = g.spp;
    const int extra = c > 3 ? c - 3 : (c == 2 ? 1 : 0);
    const int nent = 11 + (g.predictor ? 1 : 0) + (extra ? 1 : 0);
    const unsigned long long ifd_at = 8ull + strips;
    const unsigned long long over_at = ifd_at + 2ull + 12ull * nent + 4ull;
    const unsigned long long bits_at = over_at;                                   // BitsPerSample, c >= 3
    const unsigned long long offs_at = bits_at + (c >= 3 ? 2ull * c : 0ull);      // StripOffsets, n > 1
    const unsigned long long cnts_at = offs_at + (n > 1 ? 4ull * n : 0ull);       // StripByteCounts, n > 1
    const unsigned long long fmt_at = cnts_at + (n > 1 ? 4ull * n : 0ull);        // SampleFormat, c >= 3
    const unsigned long long file = fmt_at + (c >= 3 ? 2ull * c : 0ull);
    const bool too_large = file >= (1ull << 32), no_space = !too_large && file > out_cap;
    unsigned long long o = 8ull + before;
    for (long long k = lo; k < hi; ++k) {
        off[k] = o;
        if (!too_large && !no_space && n > 1) {
            te_put32(out + offs_at + 4ull * k, (unsigned int)o);
            te_put32(out + cnts_at + 4ull * k, zlen[k]);
        }
        o += (unsigned long long)zlen[k] + (zlen[k] & 1u);
    }
    if (tid != 0) return;
    *out_len = too_large ? 0 : (long long)file;
    if (too_large || no_space) {
        status[0] = too_large ? LARS_TIFE_TOO_LARGE : LARS_TIFE_NOSPACE;
        status[1] = 0;
        return;
    }
    out[0] = 'I'; out[1] = 'I';
    te_put16(out + 2, 42);
    te_put32(out + 4, (unsigned int)ifd_at);
    uint8_t *p = out + ifd_at;
    te_put16(p, (unsigned int)nent);
    p += 2;
    const unsigned int bits = 8u * g.bps;
    p += te_entry(p, 256, 4, 1, (unsigned int)g.width, true, 0);
    p += te_entry(p, 257, 4, 1, (unsigned int)g.height, true, 0);
    p += te_entry(p, 258, 3, (unsigned int)c, bits, c < 3, (unsigned int)bits_at);
    p += te_entry(p, 259, 3, 1, (unsigned int)compression, true, 0);
    p += te_entry(p, 262, 3, 1, c >= 3 ? 2 : 1, true, 0);
    p += te_entry(p, 273, 4, (unsigned int)n, 8u, n == 1, (unsigned int)offs_at);
    p += te_entry(p, 277, 3, 1, (unsigned int)c, true, 0);
    p += te_entry(p, 278, 4, 1, (unsigned int)g.rps, true, 0);
    p += te_entry(p, 279, 4, (unsigned int)n, zlen[0], n == 1, (unsigned int)cnts_at);
    p += te_entry(p, 284, 3, 1, 1, true, 0);
    if (g.predictor) p += te_entry(p, 317, 3, 1, g.bps == 4 ? 3 : 2, true, 0);
    if (extra) p += te_entry(p, 338, 3, (unsigned int)extra, 0, true, 0);
    const unsigned int format = g.bps == 4 ? 3 : 1;       // IEEE float : unsigned integer
    p += te_entry(p, 339, 3, (unsigned int)c, format, c < 3, (unsigned int)fmt_at);
    te_put32(p, 0);                                       // no further directory
    if (c >= 3)
        for (int j = 0; j < c; ++j) {
            te_put16(out + bits_at + 2 * j, bits);
            te_put16(out + fmt_at + 2 * j, format);
        }
}

// one workgroup per strip: its bytes and its pad byte to off[k]; both ends are on even addresses
__global__ __launch_bounds__(TE_PACK_THREADS) void k_te_pack(TeGeom g, const uint8_t *__restrict__ zbuf, const unsigned int *__restrict__ zlen,
                                                            const unsigned long long *__restrict__ off, uint8_t *__restrict__ out,
                                                            unsigned long long out_cap, const int *__restrict__ status)
{
    if (status[0]) return;
    const long long k = blockIdx.x;
    if (k >= g.nstrips) return;
    const unsigned int m = zlen[k] + (zlen[k] & 1u);
    const unsigned long long o = off[k];
    if (m > (unsigned long long)g.pitch || o + m > out_cap) return;              // k_te_frame refused such a file
    const uint16_t *src = reinterpret_cast<const uint16_t *>(zbuf + k * g.pitch);
    uint16_t *dst = reinterpret_cast<uint16_t *>(out + o);
    for (unsigned int j = threadIdx.x; j < m / 2; j += TE_PACK_THREADS) dst[j] = src[j];
}

// ---- Deflate ---------------------------------------------------------------------------------------------------------------------
constexpr int TZ_STAGE_THREADS = 256, TZ_STAGE_BYTES = 4 * TZ_STAGE_THREADS;     // k_tz_stage: four stored bytes per thread
constexpr int TZ_JOIN_THREADS = 256;

// Upper bound of a strip's stream for n input bytes, its pad byte included: the header 78 01; per part its bytes and five more
// (a stored block is BFINAL/BTYPE, LEN, NLEN and the bytes; the dynamic block, with its three flush bits, padding and 00 00 FF FF
// where the part is not the last, is chosen only where it is no longer than that); the Adler-32; one byte more brings the next
// strip to an even offset.
__host__ __device__ inline long long tz_parts(long long n) { return (n + DEFLATE_SEG - 1) / DEFLATE_SEG; }
__host__ __device__ inline long long tz_strip_cap(long long n)
{
    const long long bytes = 2 + n + 5 * tz_parts(n) + 4;
    return bytes + (bytes & 1);
}

__device__ inline long long tz_strip_bytes(const TeGeom &g, long long k)
{
    const long long left = (long long)g.height - k * g.rps;
    return (left < g.rps ? left : (long long)g.rps) * g.rowb;
}

// The picture as the file stores it (te_byte), for the predictors; without one the picture's own bytes are the stored bytes and
// nothing is staged.  Strips are consecutive rows, so strip k's stored bytes are stage[k * rps * rowb ...), contiguous.  One
// workgroup per TZ_STAGE_BYTES bytes of a row: blockIdx.x = row * chunks + chunk.
__global__ __launch_bounds__(TZ_STAGE_THREADS) void k_tz_stage(const uint8_t *__restrict__ img, TeGeom g, long long chunks,
                                                              uint8_t *__restrict__ stage)
{
    const long long y = blockIdx.x / chunks, q0 = (blockIdx.x - y * chunks) * TZ_STAGE_BYTES + 4 * threadIdx.x;
    if (y >= g.height) return;
    const long long B = y * g.rowb + q0;
    for (int j = 0; j < 4 && q0 + j < g.rowb; ++j) stage[B + j] = (uint8_t)te_byte(img, g, B + j);
}

// One workgroup per (strip, part): slot = strip * pf + part, pf the parts of a whole strip (the last strip may have fewer: its
// other slots stay unused).  The part's block goes to Z + slot * DEFLATE_ZCAP.
__global__ __launch_bounds__(DEFLATE_THREADS) void k_tz_deflate(const uint8_t *__restrict__ stored, TeGeom g, long long pf,
                                                               uint8_t *__restrict__ Z, unsigned int *__restrict__ seglen,
                                                               unsigned int *__restrict__ adl)
{
    const long long slot = blockIdx.x, k = slot / pf, i = slot - k * pf;
    if (k >= g.nstrips) return;
    const long long n = tz_strip_bytes(g, k), at = i * DEFLATE_SEG;
    if (at >= n) return;                                  // uniform: the whole workgroup leaves
    const int m = (int)(n - at < DEFLATE_SEG ? n - at : DEFLATE_SEG);
    deflate_segment(stored + k * g.rps * g.rowb + at, m, i == 0, at + m == n, Z + slot * DEFLATE_ZCAP, seglen + slot, adl + 2 * slot);
}

// the same with string matching (deflate_lz_device.h), where the tuning knob deflate_matching is 1
__global__ __launch_bounds__(DLZ_THREADS) void k_tz_deflate_lz(const uint8_t *__restrict__ stored, TeGeom g, long long pf,
                                                              uint8_t *__restrict__ Z, unsigned int *__restrict__ seglen,
                                                              unsigned int *__restrict__ adl)
{
    const long long slot = blockIdx.x, k = slot / pf, i = slot - k * pf;
    if (k >= g.nstrips) return;
    const long long n = tz_strip_bytes(g, k), at = i * DEFLATE_SEG;
    if (at >= n) return;                                  // uniform: the whole workgroup leaves
    const int m = (int)(n - at < DEFLATE_SEG ? n - at : DEFLATE_SEG);
    deflate_lz_segment(stored + k * g.rps * g.rowb + at, m, i == 0, at + m == n, Z + slot * DEFLATE_ZCAP, seglen + slot, adl + 2 * slot);
}

// One workgroup per strip: where each part starts within the strip's stream (an exclusive scan of the parts' lengths, 256 parts
// per round, the sum carried on), the strip's length, and the Adler-32 of the strip behind its last part.  With a_i = sum of part
// i's bytes and b_i = sum of (n_i - j) * byte_j, both mod ADLER_MOD, and r_i bytes of the strip behind part i, the checksum's halves
// are 1 + sum a_i and n + sum (b_i + r_i a_i) (adler_append, adler_value: checksum_device.h).
__global__ __launch_bounds__(TZ_JOIN_THREADS) void k_tz_join(TeGeom g, long long pf, uint8_t *__restrict__ Z,
                                                            const unsigned int *__restrict__ seglen, const unsigned int *__restrict__ adl,
                                                            unsigned int *__restrict__ partoff, unsigned int *__restrict__ zlen)
{
    __shared__ unsigned int s_scan[TZ_JOIN_THREADS / 64];
    __shared__ unsigned long long s_red[2 * TZ_JOIN_THREADS / 64];
    const int tid = threadIdx.x;
    const long long k = blockIdx.x;
    if (k >= g.nstrips) return;
    const long long n = tz_strip_bytes(g, k), p = tz_parts(n), slot0 = k * pf;
    unsigned int carry = 0;                               // a strip's stream has at most tz_strip_cap(2^30) < 2^32 bytes
    unsigned long long A = 0, B = 0;
    for (long long i0 = 0; i0 < p; i0 += TZ_JOIN_THREADS) {
        const long long i = i0 + tid;
        const unsigned int len = i < p ? seglen[slot0 + i] : 0u;
        unsigned int round;
        const unsigned int before = wg_exscan<TZ_JOIN_THREADS>(len, s_scan, &round);
        if (i < p) {
            partoff[slot0 + i] = carry + before;
            const long long at = i * DEFLATE_SEG, ni = n - at < DEFLATE_SEG ? n - at : DEFLATE_SEG;
            adler_append(A, B, adl[2 * (slot0 + i)], adl[2 * (slot0 + i) + 1], (unsigned long long)(n - at - ni));
        }
        carry += round;
    }
    adler_wg<TZ_JOIN_THREADS>(A, B, s_red);
    if (tid == 0) {
        const unsigned int sum = adler_value(A, B, (unsigned long long)n);
        uint8_t *zl = Z + (slot0 + p - 1) * DEFLATE_ZCAP + seglen[slot0 + p - 1] - 4;      // the last part's length counts these four
        zl[0] = (uint8_t)(sum >> 24); zl[1] = (uint8_t)(sum >> 16); zl[2] = (uint8_t)(sum >> 8); zl[3] = (uint8_t)sum;
        zlen[k] = carry;
    }
}

// one workgroup per (strip, part): the part's bytes to their place in the strip at off[strip]; the last part adds the pad byte
__global__ __launch_bounds__(TE_PACK_THREADS) void k_tz_pack(TeGeom g, long long pf, const uint8_t *__restrict__ Z,
                                                            const unsigned int *__restrict__ seglen, const unsigned int *__restrict__ partoff,
                                                            const unsigned int *__restrict__ zlen, const unsigned long long *__restrict__ off,
                                                            uint8_t *__restrict__ out, unsigned long long out_cap, const int *__restrict__ status)
{
    if (status[0]) return;
    const long long slot = blockIdx.x, k = slot / pf, i = slot - k * pf;
    if (k >= g.nstrips) return;
    const long long n = tz_strip_bytes(g, k), p = tz_parts(n);
    if (i >= p) return;
    const unsigned int m = seglen[slot];
    const unsigned long long o = off[k] + partoff[slot];
    const bool pad = i == p - 1 && (zlen[k] & 1u);
    if (m > (unsigned int)DEFLATE_ZCAP || o + m + (pad ? 1ull : 0ull) > out_cap) return;   // k_te_frame refused such a file
    const uint8_t *src = Z + slot * DEFLATE_ZCAP;
    uint8_t *dst = out + o;
    for (unsigned int j = threadIdx.x; j < m; j += TE_PACK_THREADS) dst[j] = src[j];
    if (pad && threadIdx.x == 0) dst[m] = 0;
}

// the strips of a picture, or false for a shape that is not encoded; itemsize 1 or 2: unsigned integers; 4, which only the
// _f32 entry points hand in (f32): float32
bool te_geometry(int64_t h, int64_t w, int channels, int itemsize, bool f32, int64_t rows_per_strip, int predictor, TeGeom *g)
{
    if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24) || channels < 1 || channels > 5 || rows_per_strip < 0 ||
        !(f32 ? itemsize == 4 : (itemsize == 1 || itemsize == 2)))
        return false;
    g->rowb = (long long)w * channels * itemsize;
    long long rps = rows_per_strip ? rows_per_strip : std::max<long long>(1, tuning().tiff_strip_bytes / g->rowb);
    rps = std::min<long long>(rps, h);
    if (rps * g->rowb > (1ll << 30)) return false;
    g->nstrips = (h + rps - 1) / rps;
    g->pitch = (te_strip_cap(rps * g->rowb) + 3) & ~3ll;
    g->width = (int)w; g->height = (int)h; g->spp = channels; g->bps = itemsize;
    g->rps = (int)rps; g->predictor = predictor ? 1 : 0;
    return true;
}

struct TePlan {
    uint8_t *zbuf;
    unsigned int *zlen;
    unsigned long long *off;
};

TePlan te_plan(const TeGeom &g, Carver &cv)
{
    TePlan P;
    P.zbuf = cv.take<uint8_t>((size_t)(g.nstrips * g.pitch));
    P.zlen = cv.take<unsigned int>((size_t)g.nstrips);
    P.off = cv.take<unsigned long long>((size_t)g.nstrips);
    return P;
}

size_t te_bound(const TeGeom &g)
{
    const long long last = ((long long)g.height - (g.nstrips - 1) * g.rps) * g.rowb;
    return 8 + (size_t)((g.nstrips - 1) * te_strip_cap((long long)g.rps * g.rowb) + te_strip_cap(last)) + 2 + 12 * TE_MAX_ENTRIES + 4 +
           4 * (size_t)g.spp + 8 * (size_t)g.nstrips;
}

int te_check(const char *who, bool pointers, int64_t h, int64_t w, int channels, int itemsize, bool f32, int64_t rows_per_strip, int predictor,
             TeGeom *g)
{
    if (!pointers) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    if (!te_geometry(h, w, channels, itemsize, f32, rows_per_strip, predictor, g))
        return fail(LARS_ERR_INVALID, "%s: %lld x %lld x %d samples of %d bytes in strips of %lld rows (1 to 2^24 on each side, 1 to 5 samples of %s, "
                    "strips of at most 2^30 bytes)", who, (long long)h, (long long)w, channels, itemsize, (long long)rows_per_strip,
                    f32 ? "4 bytes" : "1 or 2 bytes");
    if (g->nstrips >= (1ll << 31)) return fail(LARS_ERR_UNSUPPORTED, "%s: %lld strips", who, g->nstrips);
    return LARS_OK;
}

// Deflate: the slots of the parts (pf per strip), the staged picture, and what the join step leaves
struct TzPlan {
    long long pf, slots, chunks;   // chunks: workgroups of k_tz_stage per row
    uint8_t *stage, *z;
    unsigned int *seglen, *adl, *partoff, *zlen;
    unsigned long long *off;
};

TzPlan tz_plan(const TeGeom &g, Carver &cv)
{
    TzPlan P;
    P.pf = tz_parts((long long)g.rps * g.rowb);
    P.slots = g.nstrips * P.pf;
    P.chunks = (g.rowb + TZ_STAGE_BYTES - 1) / TZ_STAGE_BYTES;
    P.stage = cv.take<uint8_t>((size_t)g.height * (size_t)g.rowb);      // used with a predictor only; the size does not ask
    P.z = cv.take<uint8_t>((size_t)P.slots * DEFLATE_ZCAP);
    P.seglen = cv.take<unsigned int>((size_t)P.slots);
    P.adl = cv.take<unsigned int>((size_t)P.slots * 2);
    P.partoff = cv.take<unsigned int>((size_t)P.slots);
    P.zlen = cv.take<unsigned int>((size_t)g.nstrips);
    P.off = cv.take<unsigned long long>((size_t)g.nstrips);
    return P;
}

// te_bound with the Deflate strips: tz_strip_cap per strip (the last one may be shorter), the header, the directory at its
// largest, BitsPerSample and SampleFormat arrays, StripOffsets and StripByteCounts
size_t tz_bound(const TeGeom &g)
{
    const long long last = ((long long)g.height - (g.nstrips - 1) * g.rps) * g.rowb;
    return 8 + (size_t)((g.nstrips - 1) * tz_strip_cap((long long)g.rps * g.rowb) + tz_strip_cap(last)) + 2 + 12 * TE_MAX_ENTRIES + 4 +
           4 * (size_t)g.spp + 8 * (size_t)g.nstrips;
}

}  // namespace

}  // namespace lars

using namespace lars;

// compression: TIFF's own codes, 5 (LZW) or 8 (Deflate)
static size_t bound_of(int64_t h, int64_t w, int channels, int itemsize, bool f32, int64_t rows_per_strip, int compression = 5)
{
    TeGeom g;
    if (!te_geometry(h, w, channels, itemsize, f32, rows_per_strip, 0, &g)) return 0;
    return compression == 8 ? tz_bound(g) : te_bound(g);
}

static size_t scratch_of(int64_t h, int64_t w, int channels, int itemsize, bool f32, int64_t rows_per_strip, int compression = 5)
{
    TeGeom g;
    if (!te_geometry(h, w, channels, itemsize, f32, rows_per_strip, 0, &g)) return 0;
    Carver size(nullptr);
    if (compression == 8) tz_plan(g, size);
    else te_plan(g, size);
    return size.bytes();
}

static int encode_on_device(const char *who, const void *img, int64_t h, int64_t w, int channels, int itemsize, bool f32, int64_t rows_per_strip,
                            int predictor, uint8_t *out, size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream,
                            int compression = 5)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    TeGeom g;
    LARS_TRY(te_check(who, img && out && out_len_dev && status_dev && scratch, h, w, channels, itemsize, f32, rows_per_strip, predictor, &g));
    if (((uintptr_t)img | (uintptr_t)out) & 1) return fail(LARS_ERR_INVALID, "%s: img and out must be on even addresses", who);
    Carver cv(scratch);
    if (compression == 8) {
        const TzPlan P = tz_plan(g, cv);
        if (P.slots >= (1ll << 31) || (long long)g.height * P.chunks >= (1ll << 31))
            return fail(LARS_ERR_UNSUPPORTED, "%s: %lld parts of strips, %lld rows of %lld bytes", who, P.slots, (long long)g.height, g.rowb);
        hipStream_t s = pick_stream(c, stream);
        LARS_HIP_TRY(hipMemsetAsync(status_dev, 0, 2 * sizeof(int32_t), s));
        LARS_HIP_TRY(hipMemsetAsync(out_len_dev, 0, sizeof(int64_t), s));
        const uint8_t *stored = static_cast<const uint8_t *>(img);      // little-endian host: without a predictor the samples are the stored bytes
        if (g.predictor) {
            hipLaunchKernelGGL(k_tz_stage, dim3((unsigned)(g.height * P.chunks)), dim3(TZ_STAGE_THREADS), 0, s, stored, g, P.chunks, P.stage);
            stored = P.stage;
        }
        if (tuning().deflate_matching)
            hipLaunchKernelGGL(k_tz_deflate_lz, dim3((unsigned)P.slots), dim3(DLZ_THREADS), 0, s, stored, g, P.pf, P.z, P.seglen, P.adl);
        else
            hipLaunchKernelGGL(k_tz_deflate, dim3((unsigned)P.slots), dim3(DEFLATE_THREADS), 0, s, stored, g, P.pf, P.z, P.seglen, P.adl);
        hipLaunchKernelGGL(k_tz_join, dim3((unsigned)g.nstrips), dim3(TZ_JOIN_THREADS), 0, s, g, P.pf, P.z, P.seglen, P.adl, P.partoff, P.zlen);
        hipLaunchKernelGGL(k_te_frame, dim3(1), dim3(TE_FRAME_THREADS), 0, s, g, 8, P.zlen, P.off, out, (unsigned long long)out_cap,
                           reinterpret_cast<long long *>(out_len_dev), status_dev);
        hipLaunchKernelGGL(k_tz_pack, dim3((unsigned)P.slots), dim3(TE_PACK_THREADS), 0, s, g, P.pf, P.z, P.seglen, P.partoff, P.zlen, P.off, out,
                           (unsigned long long)out_cap, status_dev);
        return launch_check(who);
    }
    const TePlan P = te_plan(g, cv);
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(status_dev, 0, 2 * sizeof(int32_t), s));
    LARS_HIP_TRY(hipMemsetAsync(out_len_dev, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL(k_te_lzw, dim3((unsigned)g.nstrips), dim3(64), 0, s, static_cast<const uint8_t *>(img), g, P.zbuf, P.zlen, status_dev);
    hipLaunchKernelGGL(k_te_frame, dim3(1), dim3(TE_FRAME_THREADS), 0, s, g, 5, P.zlen, P.off, out, (unsigned long long)out_cap,
                       reinterpret_cast<long long *>(out_len_dev), status_dev);
    hipLaunchKernelGGL(k_te_pack, dim3((unsigned)g.nstrips), dim3(TE_PACK_THREADS), 0, s, g, P.zbuf, P.zlen, P.off, out,
                       (unsigned long long)out_cap, status_dev);
    return launch_check(who);
}

// host picture in, file out: one upload, then the status and the length (one small read), then the file's bytes
static int encode_to_host_tiff(const char *who, const void *img, int64_t h, int64_t w, int channels, int itemsize, bool f32,
                               int64_t rows_per_strip, int predictor, uint8_t *out, size_t out_cap, int64_t *out_len, int compression = 5)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    TeGeom g;
    LARS_TRY(te_check(who, img && out && out_len, h, w, channels, itemsize, f32, rows_per_strip, predictor, &g));
    const size_t in_bytes = (size_t)h * g.rowb, dev_cap = std::min(compression == 8 ? tz_bound(g) : te_bound(g), out_cap);
    Carver size(nullptr);
    if (compression == 8) tz_plan(g, size);
    else te_plan(g, size);
    struct Answer { int64_t len; int32_t status[2]; } a = {0, {0, 0}}, *d_a;
    uint8_t *d_in, *d_out;
    char *d_scr;
    LARS_TRY(ws_plan(c, [&](Carver &cv) {
        d_in = cv.take<uint8_t>(in_bytes);
        d_out = cv.take<uint8_t>(dev_cap);
        d_scr = cv.take<char>(size.bytes());
        d_a = cv.take<Answer>(1);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(d_in, img, in_bytes, hipMemcpyHostToDevice, s));
    LARS_TRY(encode_on_device(who, d_in, h, w, channels, itemsize, f32, g.rps, predictor, d_out, dev_cap, &d_a->len, d_a->status, d_scr, s,
                              compression));
    LARS_HIP_TRY(hipMemcpyAsync(&a, d_a, sizeof a, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    switch (a.status[0]) {
    case LARS_TIFE_OK: break;
    case LARS_TIFE_NOSPACE:
        return fail(LARS_ERR_INVALID, "%s: the file needs %lld bytes, out_cap is %zu (device status %d)", who, (long long)a.len, out_cap, a.status[0]);
    case LARS_TIFE_TOO_LARGE: return fail(LARS_ERR_UNSUPPORTED, "%s: image too large for a classic TIFF (4 GiB)", who);
    default: return fail(LARS_ERR_HIP, "%s: internal encoder status %d (%d)", who, a.status[0], a.status[1]);
    }
    if (a.len <= 0 || (size_t)a.len > dev_cap) return fail(LARS_ERR_HIP, "%s: the device did not finish the file", who);
    LARS_HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)a.len, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    *out_len = a.len;
    return LARS_OK;
}

extern "C" {

size_t lars_tiff_bound(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip)
{
    return bound_of(h, w, channels, itemsize, false, rows_per_strip);
}

size_t lars_tiff_encode_scratch_bytes(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip)
{
    return scratch_of(h, w, channels, itemsize, false, rows_per_strip);
}

int lars_d_encode_tiff(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                       uint8_t *out, size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream)
{
    return encode_on_device("lars_d_encode_tiff", img, h, w, channels, itemsize, false, rows_per_strip, predictor, out, out_cap,
                            out_len_dev, status_dev, scratch, stream);
}

int lars_h_encode_tiff(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                       uint8_t *out, size_t out_cap, int64_t *out_len)
{
    return encode_to_host_tiff("lars_h_encode_tiff", img, h, w, channels, itemsize, false, rows_per_strip, predictor, out, out_cap, out_len);
}

// the float32 siblings: the same strips, bound and kernels with four bytes per sample
size_t lars_tiff_f32_bound(int64_t h, int64_t w, int channels, int64_t rows_per_strip) { return bound_of(h, w, channels, 4, true, rows_per_strip); }

size_t lars_tiff_f32_encode_scratch_bytes(int64_t h, int64_t w, int channels, int64_t rows_per_strip)
{
    return scratch_of(h, w, channels, 4, true, rows_per_strip);
}

int lars_d_encode_tiff_f32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                           size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream)
{
    return encode_on_device("lars_d_encode_tiff_f32", img, h, w, channels, 4, true, rows_per_strip, predictor, out, out_cap, out_len_dev, status_dev,
                            scratch, stream);
}

int lars_h_encode_tiff_f32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                           size_t out_cap, int64_t *out_len)
{
    return encode_to_host_tiff("lars_h_encode_tiff_f32", img, h, w, channels, 4, true, rows_per_strip, predictor, out, out_cap, out_len);
}

// Deflate (Compression 8): the same arguments, strips, knob, status codes and 4 GiB refusal; only the strips' streams differ
size_t lars_tiff_deflate_bound(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip)
{
    return bound_of(h, w, channels, itemsize, false, rows_per_strip, 8);
}

size_t lars_tiff_deflate_encode_scratch_bytes(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip)
{
    return scratch_of(h, w, channels, itemsize, false, rows_per_strip, 8);
}

int lars_d_encode_tiff_deflate(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                               uint8_t *out, size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream)
{
    return encode_on_device("lars_d_encode_tiff_deflate", img, h, w, channels, itemsize, false, rows_per_strip, predictor, out, out_cap,
                            out_len_dev, status_dev, scratch, stream, 8);
}

int lars_h_encode_tiff_deflate(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                               uint8_t *out, size_t out_cap, int64_t *out_len)
{
    return encode_to_host_tiff("lars_h_encode_tiff_deflate", img, h, w, channels, itemsize, false, rows_per_strip, predictor, out, out_cap,
                               out_len, 8);
}

size_t lars_tiff_float32_deflate_bound(int64_t h, int64_t w, int channels, int64_t rows_per_strip)
{
    return bound_of(h, w, channels, 4, true, rows_per_strip, 8);
}

size_t lars_tiff_float32_deflate_encode_scratch_bytes(int64_t h, int64_t w, int channels, int64_t rows_per_strip)
{
    return scratch_of(h, w, channels, 4, true, rows_per_strip, 8);
}

int lars_d_encode_tiff_deflate_float32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                                   size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream)
{
    return encode_on_device("lars_d_encode_tiff_deflate_float32", img, h, w, channels, 4, true, rows_per_strip, predictor, out, out_cap, out_len_dev,
                            status_dev, scratch, stream, 8);
}

int lars_h_encode_tiff_deflate_float32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                                   size_t out_cap, int64_t *out_len)
{
    return encode_to_host_tiff("lars_h_encode_tiff_deflate_float32", img, h, w, channels, 4, true, rows_per_strip, predictor, out, out_cap, out_len, 8);
}

}  // extern "C"
