// The Deflate segment coder the PNG encoder (png.hip, k_png_deflate) and the TIFF encoder (tiff_encode.hip, k_te_deflate) share: one
// workgroup of DEFLATE_THREADS threads codes at most DEFLATE_SEG contiguous bytes as one block of a zlib stream.  Symbol histogram in
// LDS, length-limited (15 bit) Huffman code lengths (Moffat-Katajainen + the max-code-length fix-up, on one lane), the dynamic
// block header with its code-length alphabet (16/17/18 runs), then every thread packs the codes of its sub-range at the bit
// offset a workgroup prefix sum gives it.  Literal-only coding (zlib's Z_HUFFMAN_ONLY strategy).  A segment that is not the last of
// its stream ends in an empty stored block (sync flush) so that it ends on a byte boundary; a segment whose dynamic block would be
// larger is stored instead.  Each segment also leaves its Adler-32 partial sums.  tests/png_encode_model.py restates lane 0's work.
#pragma once

#include "checksum_device.h"
#include "common.h"

namespace lars {

#define DEFLATE_SEG 32768                               // input bytes per deflate block (one workgroup)
#define DEFLATE_THREADS 256
#define DEFLATE_ZCAP (DEFLATE_SEG + 256)                // per-segment output capacity: zlib header + stored header + Adler-32 fit
#define DEFLATE_OUT_WORDS ((DEFLATE_SEG + 64) / 4)      // LDS bit buffer of one dynamic block (never larger than the stored form)

static_assert(DEFLATE_SEG <= 65535, "one stored block per segment");

// ---- Huffman code lengths (one lane) ----------------------------------------------------------------------------------
// key[0..n) ascending (frequency, symbol); on return key[i] = code length of the i-th sorted symbol, at most maxbits,
// lengths of the most frequent symbols shortest.  Moffat & Katajainen's in-place minimum-redundancy lengths, then the
// Kraft fix-up that moves overlong codes to maxbits (the method of miniz's tdefl_optimize_huffman_table).
__device__ void huff_lengths(unsigned int *key, int n, int maxbits)
{
    if (n == 1) { key[0] = 1; return; }
    key[0] += key[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || key[root] < key[leaf]) { key[next] = key[root]; key[root++] = next; }
        else key[next] = key[leaf++];
        if (leaf >= n || (root < next && key[root] < key[leaf])) { key[next] += key[root]; key[root++] = next; }
        else key[next] += key[leaf++];
    }
    key[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) key[next] = key[key[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    int next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)key[root] == dpth) { ++used; --root; }
        while (avbl > used) { key[next--] = dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
    unsigned int count[33];
    for (int i = 0; i < 33; ++i) count[i] = 0;
    for (int i = 0; i < n; ++i) ++count[key[i] > 32u ? 32u : key[i]];
    for (int i = maxbits + 1; i <= 32; ++i) { count[maxbits] += count[i]; count[i] = 0; }
    unsigned int total = 0;
    for (int i = maxbits; i > 0; --i) total += count[i] << (maxbits - i);
    while (total != (1u << maxbits)) {
        --count[maxbits];
        for (int i = maxbits - 1; i > 0; --i)
            if (count[i]) { --count[i]; count[i + 1] += 2; break; }
        --total;
    }
    int j = n;
    for (int len = 1; len <= maxbits; ++len)
        for (unsigned int k = count[len]; k > 0; --k) key[--j] = len;
}

// canonical deflate codes, bit-reversed for LSB-first packing: out[s] = (len << 16) | code
__device__ void huff_codes(const uint8_t *len, int nsym, unsigned int *out)
{
    unsigned int bl[16], next[16];
    for (int i = 0; i < 16; ++i) bl[i] = 0;
    for (int s = 0; s < nsym; ++s) ++bl[len[s]];
    bl[0] = 0;
    unsigned int code = 0;
    for (int b = 1; b < 16; ++b) { code = (code + bl[b - 1]) << 1; next[b] = code; }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        unsigned int rev = 0;
        if (l) {
            const unsigned int c = next[l]++;
            for (int i = 0; i < l; ++i) rev |= ((c >> i) & 1u) << (l - 1 - i);
        }
        out[s] = ((unsigned int)l << 16) | rev;
    }
}

// plain (non-atomic) LSB-first bit writer into a zeroed word buffer; n <= 16
__device__ inline void put_bits(unsigned int *buf, unsigned int &pos, unsigned int v, int n)
{
    const unsigned int sh = pos & 31u;
    buf[pos >> 5] |= v << sh;
    if (sh + n > 32u) buf[(pos >> 5) + 1] |= v >> (32u - sh);
    pos += n;
}

// One segment, by a whole workgroup of DEFLATE_THREADS threads (every thread calls it, with the same arguments): in[0 .. n), 1 <= n <=
// DEFLATE_SEG, becomes one block at z (DEFLATE_ZCAP bytes).  first: the segment opens its zlib stream and writes the header 78 01.
// last: the block carries BFINAL, no empty stored block follows it, and *seglen counts four more bytes, which the caller fills
// with the stream's Adler-32 behind the block.  *seglen = bytes at z; adl[0] = sum of the bytes, adl[1] = sum of (n - j) * byte_j,
// both mod ADLER_MOD.  LDS: 38.0 KiB of static arrays.
__device__ __forceinline__ void deflate_segment(const uint8_t *__restrict__ in, const int n, const bool first, const bool last,
                                                uint8_t *__restrict__ z, unsigned int *__restrict__ seglen, unsigned int *__restrict__ adl)
{
    __shared__ unsigned int hist[288];
    __shared__ unsigned int table[288];         // (length << 16) | reversed code of each literal / end-of-block symbol
    __shared__ unsigned int key[288];
    __shared__ unsigned short sym[288];
    __shared__ unsigned int obuf[DEFLATE_OUT_WORDS];
    __shared__ unsigned long long s_red[2 * DEFLATE_THREADS / 64];
    __shared__ unsigned int s_scan[DEFLATE_THREADS / 64];
    __shared__ uint8_t lens[260], rsym[260], rext[260];   // lane 0's work arrays
    __shared__ unsigned int s_nused, s_hdr_bits, s_data_bits, s_huff, s_body;
    const int tid = threadIdx.x;
    const int pre = first ? 2 : 0;               // zlib header 78 01 (deflate, 32 KiB window, fastest level)

    for (int i = tid; i < 288; i += DEFLATE_THREADS) hist[i] = 0;
    for (int i = tid; i < DEFLATE_OUT_WORDS; i += DEFLATE_THREADS) obuf[i] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    for (int j = tid; j < n; j += DEFLATE_THREADS) {
        const unsigned int b = in[j];
        atomicAdd(&hist[b], 1u);
        s1 += b;
        s2 += (unsigned long long)(n - j) * b;
    }
    adler_wg<DEFLATE_THREADS>(s1, s2, s_red);
    if (tid == 0) {
        hist[256] = 1;                           // end of block
        adl[0] = (unsigned int)s1;
        adl[1] = (unsigned int)s2;
    }
    __syncthreads();
    // rank sort of the used symbols by (frequency, symbol)
    for (int s = tid; s < 257; s += DEFLATE_THREADS) {
        const unsigned int f = hist[s];
        if (!f) continue;
        const unsigned long long mine = ((unsigned long long)f << 9) | (unsigned)s;
        unsigned int r = 0;
        for (int t = 0; t < 257; ++t) {
            const unsigned int g = hist[t];
            r += (g && ((((unsigned long long)g << 9) | (unsigned)t) < mine)) ? 1u : 0u;
        }
        key[r] = f;
        sym[r] = (unsigned short)s;
    }
    if (tid == 0) {
        unsigned int u = 0;
        for (int s = 0; s < 257; ++s) u += hist[s] ? 1u : 0u;
        s_nused = u;
    }
    __syncthreads();
    if (tid == 0) {
        const int nused = (int)s_nused;
        huff_lengths(key, nused, 15);
        for (int s = 0; s < 257; ++s) lens[s] = 0;
        for (int i = 0; i < nused; ++i) lens[sym[i]] = (uint8_t)key[i];
        huff_codes(lens, 257, table);
        lens[257] = 1;                           // two distance codes of length 1 (a complete, unused distance tree)
        lens[258] = 1;
        // run-length coded code lengths (HLIT = 257, HDIST = 2): 16 repeats the previous length 3-6 times, 17 / 18 are
        // 3-10 / 11-138 zeros
        int nr = 0;
        for (int i = 0; i < 259;) {
            const int v = lens[i];
            int run = 1;
            while (i + run < 259 && lens[i + run] == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = run < 138 ? run : 138; rsym[nr] = 18; rext[nr++] = (uint8_t)(r - 11); run -= r; }
                if (run >= 3) { rsym[nr] = 17; rext[nr++] = (uint8_t)(run - 3); run = 0; }
                while (run-- > 0) { rsym[nr] = 0; rext[nr++] = 0; }
            } else {
                rsym[nr] = (uint8_t)v; rext[nr++] = 0; --run;
                while (run >= 3) { const int r = run < 6 ? run : 6; rsym[nr] = 16; rext[nr++] = (uint8_t)(r - 3); run -= r; }
                while (run-- > 0) { rsym[nr] = (uint8_t)v; rext[nr++] = 0; }
            }
        }
        unsigned int cfreq[19];
        for (int i = 0; i < 19; ++i) cfreq[i] = 0;
        for (int i = 0; i < nr; ++i) ++cfreq[rsym[i]];
        unsigned int ckey[19];
        unsigned short csym[19];
        int nc = 0;
        for (int s = 0; s < 19; ++s) {           // insertion sort by (frequency, symbol)
            if (!cfreq[s]) continue;
            int p = nc++;
            while (p > 0 && ckey[p - 1] > cfreq[s]) { ckey[p] = ckey[p - 1]; csym[p] = csym[p - 1]; --p; }
            ckey[p] = cfreq[s];
            csym[p] = (unsigned short)s;
        }
        huff_lengths(ckey, nc, 7);
        uint8_t clen[19];
        for (int s = 0; s < 19; ++s) clen[s] = 0;
        for (int i = 0; i < nc; ++i) clen[csym[i]] = (uint8_t)ckey[i];
        unsigned int ccode[19];
        huff_codes(clen, 19, ccode);
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && clen[order[hclen - 1]] == 0) --hclen;
        unsigned int pos = 0;
        put_bits(obuf, pos, last ? 1u : 0u, 1);
        put_bits(obuf, pos, 2u, 2);              // BTYPE 2: dynamic Huffman
        put_bits(obuf, pos, 257u - 257u, 5);
        put_bits(obuf, pos, 2u - 1u, 5);
        put_bits(obuf, pos, (unsigned)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) put_bits(obuf, pos, clen[order[i]], 3);
        for (int i = 0; i < nr; ++i) {
            const unsigned int e = ccode[rsym[i]];
            put_bits(obuf, pos, e & 0xFFFFu, (int)(e >> 16));
            if (rsym[i] == 16) put_bits(obuf, pos, rext[i], 2);
            else if (rsym[i] == 17) put_bits(obuf, pos, rext[i], 3);
            else if (rsym[i] == 18) put_bits(obuf, pos, rext[i], 7);
        }
        unsigned long long data = 0;
        for (int s = 0; s < 256; ++s) data += (unsigned long long)hist[s] * (table[s] >> 16);
        s_hdr_bits = pos;
        s_data_bits = (unsigned int)data;
        const unsigned long long bits = pos + data + (table[256] >> 16);
        const unsigned long long huff_bytes = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
        s_huff = huff_bytes <= (unsigned long long)n + 5ull ? 1u : 0u;
    }
    __syncthreads();
    unsigned int body;
    if (s_huff) {
        // each thread packs a contiguous sub-range at the offset the prefix sum of the sub-ranges' bit counts gives it
        const int chunk = (n + DEFLATE_THREADS - 1) / DEFLATE_THREADS;
        const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
        unsigned int bits = 0;
        for (int j = lo; j < hi; ++j) bits += table[in[j]] >> 16;
        unsigned int pos = s_hdr_bits + wg_exscan<DEFLATE_THREADS>(bits, s_scan);
        unsigned long long acc = 0;
        unsigned int nacc = pos & 31u, w = pos >> 5;
        for (int j = lo; j < hi; ++j) {
            const unsigned int e = table[in[j]];
            acc |= (unsigned long long)(e & 0xFFFFu) << nacc;
            nacc += e >> 16;
            if (nacc >= 32) {
                atomicOr(&obuf[w++], (unsigned int)acc);   // OR of disjoint bits: the result does not depend on order
                acc >>= 32;
                nacc -= 32;
            }
        }
        if (nacc) atomicOr(&obuf[w], (unsigned int)acc);
        __syncthreads();
        if (tid == 0) {
            unsigned int p = s_hdr_bits + s_data_bits;
            put_bits(obuf, p, table[256] & 0xFFFFu, (int)(table[256] >> 16));
            if (!last) {                         // empty stored block: 3 zero bits, align, LEN 0000, NLEN FFFF
                const unsigned int q = (p + 3 + 7) / 8;
                reinterpret_cast<uint8_t *>(obuf)[q + 2] = 0xFF;
                reinterpret_cast<uint8_t *>(obuf)[q + 3] = 0xFF;
                body = q + 4;
            } else {
                body = (p + 7) / 8;
            }
            s_body = body;
        }
        __syncthreads();
        body = s_body;
        const uint8_t *ob = reinterpret_cast<const uint8_t *>(obuf);
        for (unsigned int j = tid; j < body; j += DEFLATE_THREADS) z[pre + j] = ob[j];
    } else {
        // stored block: BFINAL / BTYPE 0 byte, LEN, NLEN, the bytes
        body = (unsigned int)n + 5u;
        if (tid == 0) {
            z[pre] = last ? 1 : 0;
            z[pre + 1] = (uint8_t)(n & 255);
            z[pre + 2] = (uint8_t)(n >> 8);
            z[pre + 3] = (uint8_t)(~n & 255);
            z[pre + 4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int j = tid; j < n; j += DEFLATE_THREADS) z[pre + 5 + j] = in[j];
    }
    if (tid == 0) {
        if (pre) { z[0] = 0x78; z[1] = 0x01; }
        *seglen = (unsigned int)pre + body + (last ? 4u : 0u);    // the last 4: Adler-32, written by the caller's frame or join step
    }
}

}  // namespace lars
