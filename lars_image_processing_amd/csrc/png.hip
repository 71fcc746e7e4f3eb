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

#include "codec_host.h"

namespace lars {

#define PNG_SEG 32768                           // bytes of filtered stream per deflate block (one workgroup)
#define PNG_THREADS 256
#define PNG_ZCAP (PNG_SEG + 256)                // per-segment output capacity: zlib header + stored header + Adler-32 fit
#define PNG_OUT_WORDS ((PNG_SEG + 64) / 4)      // LDS bit buffer of one dynamic block (never larger than the stored form)
#define PNG_CRC_POLY 0xEDB88320u

static_assert(PNG_SEG <= 65535, "one stored block per segment");

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

// one workgroup per segment of the filtered stream -> Z + seg * PNG_ZCAP, seglen[seg] bytes; adl[2 seg] = sum of the bytes,
// adl[2 seg + 1] = sum of (n - j) * byte_j, both mod 65521
__global__ __launch_bounds__(PNG_THREADS) void k_png_deflate(const uint8_t *__restrict__ filt, long long total, long long nseg,
                                                            uint8_t *__restrict__ Z, unsigned int *__restrict__ seglen,
                                                            unsigned int *__restrict__ adl)
{
    __shared__ unsigned int hist[288];
    __shared__ unsigned int table[288];         // (length << 16) | reversed code of each literal / end-of-block symbol
    __shared__ unsigned int key[288];
    __shared__ unsigned short sym[288];
    __shared__ unsigned int obuf[PNG_OUT_WORDS];
    __shared__ unsigned long long red[2][PNG_THREADS];
    __shared__ unsigned int scan[PNG_THREADS];
    __shared__ uint8_t lens[260], rsym[260], rext[260];   // lane 0's work arrays
    __shared__ unsigned int s_nused, s_hdr_bits, s_data_bits, s_huff, s_body;
    const int tid = threadIdx.x;
    const long long seg = blockIdx.x;
    const long long base = seg * PNG_SEG;
    const int n = (int)(total - base < PNG_SEG ? total - base : PNG_SEG);
    const bool last = seg == nseg - 1;
    const uint8_t *in = filt + base;
    uint8_t *z = Z + seg * PNG_ZCAP;
    const int pre = seg == 0 ? 2 : 0;            // zlib header 78 01 (deflate, 32 KiB window, fastest level)

    for (int i = tid; i < 288; i += PNG_THREADS) hist[i] = 0;
    for (int i = tid; i < PNG_OUT_WORDS; i += PNG_THREADS) obuf[i] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    for (int j = tid; j < n; j += PNG_THREADS) {
        const unsigned int b = in[j];
        atomicAdd(&hist[b], 1u);
        s1 += b;
        s2 += (unsigned long long)(n - j) * b;
    }
    red[0][tid] = s1;
    red[1][tid] = s2;
    __syncthreads();
    for (int half = PNG_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) { red[0][tid] += red[0][tid + half]; red[1][tid] += red[1][tid + half]; }
        __syncthreads();
    }
    if (tid == 0) {
        hist[256] = 1;                           // end of block
        adl[2 * seg] = (unsigned int)(red[0][0] % 65521ull);
        adl[2 * seg + 1] = (unsigned int)(red[1][0] % 65521ull);
    }
    __syncthreads();
    // rank sort of the used symbols by (frequency, symbol)
    for (int s = tid; s < 257; s += PNG_THREADS) {
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
        const int chunk = (n + PNG_THREADS - 1) / PNG_THREADS;
        const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
        unsigned int bits = 0;
        for (int j = lo; j < hi; ++j) bits += table[in[j]] >> 16;
        scan[tid] = bits;
        __syncthreads();
        for (int off = 1; off < PNG_THREADS; off <<= 1) {
            const unsigned int v = tid >= off ? scan[tid - off] : 0u;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        unsigned int pos = s_hdr_bits + scan[tid] - bits;
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
        for (unsigned int j = tid; j < body; j += PNG_THREADS) z[pre + j] = ob[j];
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
        for (int j = tid; j < n; j += PNG_THREADS) z[pre + 5 + j] = in[j];
    }
    if (tid == 0) {
        if (pre) { z[0] = 0x78; z[1] = 0x01; }
        seglen[seg] = (unsigned int)pre + body + (last ? 4u : 0u);    // the last 4: Adler-32, written by k_png_frame
    }
}

// ---- CRC-32 -----------------------------------------------------------------------------------------------------------
__device__ void crc_table_fill(unsigned int *tab, int tid, int nthreads)
{
    for (int i = tid; i < 256; i += nthreads) {
        unsigned int c = (unsigned int)i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ PNG_CRC_POLY : c >> 1;
        tab[i] = c;
    }
}

__device__ inline unsigned int crc_update(const unsigned int *tab, unsigned int crc, unsigned int byte)
{
    return tab[(crc ^ byte) & 255u] ^ (crc >> 8);
}

// a * b mod P (reflected)
__device__ unsigned int crc_multmodp(unsigned int a, unsigned int b)
{
    unsigned int m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
    }
    return p;
}

// x^(n * 2^k) mod P from x2n[i] = x^(2^i) mod P
__device__ unsigned int crc_x2nmodp(const unsigned int *x2n, unsigned long long n, unsigned int k)
{
    unsigned int p = 1u << 31;
    while (n) {
        if (n & 1) p = crc_multmodp(x2n[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
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
    __shared__ unsigned long long sums[PNG_FRAME_THREADS];
    __shared__ unsigned long long a1[PNG_FRAME_THREADS], a2[PNG_FRAME_THREADS];
    __shared__ unsigned int tab[256];
    const int tid = threadIdx.x;
    crc_table_fill(tab, tid, PNG_FRAME_THREADS);
    const long long per = (nseg + PNG_FRAME_THREADS - 1) / PNG_FRAME_THREADS;
    const long long lo = min(nseg, tid * per), hi = min(nseg, lo + per);
    unsigned long long s = 0, A = 0, B = 0;
    for (long long k = lo; k < hi; ++k) {
        s += 12ull + seglen[k];
        const long long o = k * PNG_SEG, nk = min((long long)PNG_SEG, total - o);
        const unsigned long long after = (unsigned long long)(total - o - nk) % 65521ull;
        A = (A + adl[2 * k]) % 65521ull;
        B = (B + adl[2 * k + 1] + after * adl[2 * k]) % 65521ull;
    }
    sums[tid] = s;
    a1[tid] = A;
    a2[tid] = B;
    __syncthreads();
    for (int d = 1; d < PNG_FRAME_THREADS; d <<= 1) {       // inclusive scan of the chunk bytes
        const unsigned long long v = tid >= d ? sums[tid - d] : 0ull;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    unsigned long long o = head + sums[tid] - s;
    for (long long k = lo; k < hi; ++k) {
        off[k] = o;
        o += 12ull + seglen[k];
    }
    for (int half = PNG_FRAME_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) { a1[tid] = (a1[tid] + a1[tid + half]) % 65521ull; a2[tid] = (a2[tid] + a2[tid + half]) % 65521ull; }
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned int s1 = (unsigned int)((1ull + a1[0]) % 65521ull);
        const unsigned int s2 = (unsigned int)(((unsigned long long)total % 65521ull + a2[0]) % 65521ull);
        uint8_t *zl = Z + (nseg - 1) * PNG_ZCAP + seglen[nseg - 1] - 4;
        put_be32(zl, (s2 << 16) | s1);
        const unsigned long long file = head + sums[PNG_FRAME_THREADS - 1] + 12ull;
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
    __shared__ unsigned int part[PNG_THREADS];
    const int tid = threadIdx.x;
    const long long seg = blockIdx.x;
    const unsigned int m = seglen[seg];
    const unsigned long long o = off[seg];
    if (o + 12ull + m > out_cap) return;         // k_png_frame refused the file (cannot happen within lars_png_bound)
    crc_table_fill(tab, tid, PNG_THREADS);
    if (tid == 0) {
        unsigned int p = 1u << 30;               // x^1
        x2n[0] = p;
        for (int i = 1; i < 32; ++i) x2n[i] = p = crc_multmodp(p, p);
    }
    const uint8_t *z = Z + seg * PNG_ZCAP;
    uint8_t *dst = out + o;
    for (unsigned int j = tid; j < m; j += PNG_THREADS) dst[8 + j] = z[j];
    if (tid == 0) {
        put_be32(dst, m);
        dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
    }
    __syncthreads();
    // CRC-32 of "IDAT" + data: crc(A B) = crc(A) x^(8 |B|) ^ crc(B) for finished CRCs, so each thread's piece is shifted by
    // the bytes after it and the pieces XOR together
    const unsigned int len = m + 4u;
    const unsigned int chunk = (len + PNG_THREADS - 1) / PNG_THREADS;
    const unsigned int lo = min(len, tid * chunk), hi = min(len, lo + chunk);
    const char idat[4] = {'I', 'D', 'A', 'T'};
    unsigned int crc = 0xFFFFFFFFu;
    for (unsigned int j = lo; j < hi; ++j) crc = crc_update(tab, crc, j < 4 ? (unsigned int)(uint8_t)idat[j] : z[j - 4]);
    crc = hi > lo ? ~crc : 0u;
    part[tid] = crc ? crc_multmodp(crc_x2nmodp(x2n, len - hi, 3), crc) : 0u;
    __syncthreads();
    for (int half = PNG_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half) part[tid] ^= part[tid + half];
        __syncthreads();
    }
    if (tid == 0) put_be32(dst + 8 + m, part[0]);
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
