// The Deflate segment coder with string matching (tuning knob deflate_matching = 1): k_png_deflate_lz (png.hip) and k_tz_deflate_lz
// (tiff_encode.hip) call deflate_lz_segment where k_png_deflate / k_tz_deflate call deflate_segment.  Same framing, same arguments,
// same outputs (deflate_device.h); one workgroup of DLZ_THREADS threads per segment, one workgroup per CU (the LDS map is in
// DESIGN.md).  tests/deflate_lz_model.py states the stream; the kernel writes it byte for byte:
//   hash(j) = top 12 bits of (the 4 bytes at j, little-endian) * 2654435761, for j <= n - 4
//   head[h] of a tile of 256 positions = the largest position before the tile with hash h (one round per tile: read, barrier,
//     atomicMax of the tile's own positions, barrier -- no lane order enters)
//   candidates at j <= n - 3 by rising distance: j-1 .. j-4, then head[hash(j)]; length = common prefix up to min(258, n - j);
//     the longest wins, the nearer on a tie; taken from 3 bytes on
//   greedy parse from 0; a block of HLIT 286 / HDIST 30 with both trees limited to 15 bits; written only where it is shorter than
//     both the literal-only dynamic block and the stored block, which otherwise are written exactly as deflate_segment writes them
// Matches never leave the segment.  The blocks go to global memory by atomicOr of disjoint bits into words this workgroup zeroed.
#pragma once

#include "deflate_device.h"

namespace lars {

#define DLZ_THREADS 1024
#define DLZ_TILE 256                                    // positions per hash round
#define DLZ_HASH_BITS 12
#define DLZ_MIN_MATCH 3
#define DLZ_MAX_MATCH 258
#define DLZ_PARSE_BLOCK 64                              // positions one lane resolves in the parse
#define DLZ_PARSE_ROUND 8192                            // positions per parse round (their exits fit the 16 KiB pool)
#define DLZ_NLL 286
#define DLZ_ND 30
#define DLZ_HDR_WORDS 144                               // 74 bits + 316 runs of at most 14 bits
#define DLZ_POOL_WORDS 4096                             // 16 KiB: head[4096] | exits of a parse round | forms and scan

static_assert(DLZ_PARSE_ROUND / DLZ_PARSE_BLOCK <= DLZ_THREADS && DLZ_PARSE_BLOCK == 64, "one lane per parse block, a 64-bit mask per block");
static_assert(DLZ_PARSE_ROUND * 2 <= DLZ_POOL_WORDS * 4 && (1 << DLZ_HASH_BITS) <= DLZ_POOL_WORDS, "the pool holds the exits and the heads");
static_assert(DLZ_TILE <= DLZ_THREADS, "one lane per position of a hash round");
static_assert(DEFLATE_ZCAP % 4 == 0, "every segment's output starts on a word");

// lane-0 work arrays of one block form (matched, or literal-only)
struct DlzForm {
    unsigned int key[288];
    unsigned int table[320];                            // (length << 16) | reversed code: literal/length symbols, then the distance symbols
    unsigned int hdr[DLZ_HDR_WORDS];
    unsigned int dkey[32];
    unsigned int ckey[20], ccode[20], cfreq[20];
    unsigned int count[36], bl[16], nx[16];             // work arrays of dlz_huff_lengths / dlz_huff_codes
    unsigned short sym[288], dsym[32], csym[20];
    uint8_t lens[320], rsym[320], rext[320], clen[20];
    unsigned int hdr_bits, data_bits, bytes;
};
static_assert(2 * sizeof(DlzForm) + DLZ_THREADS / 64 * 4 <= DLZ_POOL_WORDS * 4, "two forms and the scan's words share the pool");

__device__ inline void dlz_length_symbol(unsigned int length, unsigned int &s, unsigned int &eb, unsigned int &ev)
{
    if (length == 258u) { s = 285u; eb = 0; ev = 0; return; }
    const unsigned int v = length - 3u;
    if (v < 8u) { s = 257u + v; eb = 0; ev = 0; return; }
    eb = (31u - (unsigned)__builtin_clz(v)) - 2u;
    s = 261u + 4u * eb + ((v >> eb) & 3u);
    ev = v & ((1u << eb) - 1u);
}
__device__ inline void dlz_distance_symbol(unsigned int dist, unsigned int &s, unsigned int &eb, unsigned int &ev)
{
    const unsigned int v = dist - 1u;
    if (v < 4u) { s = v; eb = 0; ev = 0; return; }
    const unsigned int k = 31u - (unsigned)__builtin_clz(v);
    eb = k - 1u;
    s = 2u * k + ((v >> eb) & 1u);
    ev = v & ((1u << eb) - 1u);
}
__device__ inline unsigned int dlz_length_extra(int s) { return (s < 265 || s == 285) ? 0u : (unsigned)(s - 261) >> 2; }
__device__ inline unsigned int dlz_distance_extra(int s) { return s < 4 ? 0u : (unsigned)(s >> 1) - 1u; }

// huff_lengths and huff_codes of deflate_device.h with their small work arrays in LDS (the caller's) instead of private memory:
// beside 150 KiB of LDS the compiler finds no other place for an indexed private array than scratch memory
__device__ __forceinline__ void dlz_huff_lengths(unsigned int *key, int n, int maxbits, unsigned int *count /* 33 */)
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
__device__ __forceinline__ void dlz_huff_codes(const uint8_t *len, int nsym, unsigned int *out, unsigned int *bl /* 16 */, unsigned int *next /* 16 */)
{
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

// rank sort of the used symbols of hist[0 .. nsym) by (frequency, symbol), by all threads
__device__ inline void dlz_rank(const unsigned int *hist, int nsym, unsigned int *key, unsigned short *sym, int tid)
{
    for (int s = tid; s < nsym; s += DLZ_THREADS) {
        const unsigned int f = hist[s];
        if (!f) continue;
        const unsigned long long mine = ((unsigned long long)f << 9) | (unsigned)s;
        unsigned int r = 0;
        for (int t = 0; t < nsym; ++t) {
            const unsigned int g = hist[t];
            r += (g && ((((unsigned long long)g << 9) | (unsigned)t) < mine)) ? 1u : 0u;
        }
        key[r] = f;
        sym[r] = (unsigned short)s;
    }
}

// One lane: the trees, the codes and the header of one form from its sorted symbols (F.key / F.sym, F.dkey / F.dsym).  nll literal /
// length symbols; nd distance code lengths in the header (dhist: the matched form's 30, nullptr: the literal-only form's two codes
// of length 1).  The literal-only form's header is deflate_segment's, bit for bit.
__device__ __forceinline__ void dlz_build(DlzForm &F, const unsigned int *hist, int nll, const unsigned int *dhist, int nd, bool last)
{
    int nused = 0;
    for (int s = 0; s < nll; ++s) nused += hist[s] ? 1 : 0;
    dlz_huff_lengths(F.key, nused, 15, F.count);
    for (int s = 0; s < nll + nd; ++s) F.lens[s] = 0;
    for (int i = 0; i < nused; ++i) F.lens[F.sym[i]] = (uint8_t)F.key[i];
    dlz_huff_codes(F.lens, nll, F.table, F.bl, F.nx);
    uint8_t *dl = F.lens + nll;
    if (dhist) {
        int ndused = 0;
        for (int s = 0; s < nd; ++s) ndused += dhist[s] ? 1 : 0;
        if (ndused == 0) { dl[0] = 1; dl[1] = 1; }
        else if (ndused == 1) { dl[F.dsym[0]] = 1; dl[F.dsym[0] == 0 ? 1 : 0] = 1; }
        else {
            dlz_huff_lengths(F.dkey, ndused, 15, F.count);
            for (int i = 0; i < ndused; ++i) dl[F.dsym[i]] = (uint8_t)F.dkey[i];
        }
        dlz_huff_codes(dl, nd, F.table + nll, F.bl, F.nx);
    } else {
        dl[0] = 1;
        dl[1] = 1;
    }
    const int ntot = nll + nd;
    int nr = 0;
    for (int i = 0; i < ntot;) {
        const int v = F.lens[i];
        int run = 1;
        while (i + run < ntot && F.lens[i + run] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; F.rsym[nr] = 18; F.rext[nr++] = (uint8_t)(r - 11); run -= r; }
            if (run >= 3) { F.rsym[nr] = 17; F.rext[nr++] = (uint8_t)(run - 3); run = 0; }
            while (run-- > 0) { F.rsym[nr] = 0; F.rext[nr++] = 0; }
        } else {
            F.rsym[nr] = (uint8_t)v; F.rext[nr++] = 0; --run;
            while (run >= 3) { const int r = run < 6 ? run : 6; F.rsym[nr] = 16; F.rext[nr++] = (uint8_t)(r - 3); run -= r; }
            while (run-- > 0) { F.rsym[nr] = (uint8_t)v; F.rext[nr++] = 0; }
        }
    }
    for (int i = 0; i < 19; ++i) F.cfreq[i] = 0;
    for (int i = 0; i < nr; ++i) ++F.cfreq[F.rsym[i]];
    int nc = 0;
    for (int s = 0; s < 19; ++s) {                   // insertion sort by (frequency, symbol)
        if (!F.cfreq[s]) continue;
        int p = nc++;
        while (p > 0 && F.ckey[p - 1] > F.cfreq[s]) { F.ckey[p] = F.ckey[p - 1]; F.csym[p] = F.csym[p - 1]; --p; }
        F.ckey[p] = F.cfreq[s];
        F.csym[p] = (unsigned short)s;
    }
    dlz_huff_lengths(F.ckey, nc, 7, F.count);
    for (int s = 0; s < 19; ++s) F.clen[s] = 0;
    for (int i = 0; i < nc; ++i) F.clen[F.csym[i]] = (uint8_t)F.ckey[i];
    dlz_huff_codes(F.clen, 19, F.ccode, F.bl, F.nx);
    int hclen = 19;
    while (hclen > 4) {
        const int o = hclen - 1;                     // the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, computed
        const int s = o < 3 ? 16 + o : o == 3 ? 0 : (o & 1) ? 8 - ((o - 3) >> 1) : 8 + ((o - 4) >> 1);
        if (F.clen[s]) break;
        --hclen;
    }
    for (int i = 0; i < DLZ_HDR_WORDS; ++i) F.hdr[i] = 0;
    unsigned int pos = 0;
    put_bits(F.hdr, pos, last ? 1u : 0u, 1);
    put_bits(F.hdr, pos, 2u, 2);
    put_bits(F.hdr, pos, (unsigned)(nll - 257), 5);
    put_bits(F.hdr, pos, (unsigned)(nd - 1), 5);
    put_bits(F.hdr, pos, (unsigned)(hclen - 4), 4);
    for (int o = 0; o < hclen; ++o) {
        const int s = o < 3 ? 16 + o : o == 3 ? 0 : (o & 1) ? 8 - ((o - 3) >> 1) : 8 + ((o - 4) >> 1);
        put_bits(F.hdr, pos, F.clen[s], 3);
    }
    for (int i = 0; i < nr; ++i) {
        const unsigned int e = F.ccode[F.rsym[i]];
        put_bits(F.hdr, pos, e & 0xFFFFu, (int)(e >> 16));
        if (F.rsym[i] == 16) put_bits(F.hdr, pos, F.rext[i], 2);
        else if (F.rsym[i] == 17) put_bits(F.hdr, pos, F.rext[i], 3);
        else if (F.rsym[i] == 18) put_bits(F.hdr, pos, F.rext[i], 7);
    }
    unsigned long long data = 0;
    for (int s = 0; s < nll; ++s)
        if (s != 256) data += (unsigned long long)hist[s] * ((F.table[s] >> 16) + (s > 256 ? dlz_length_extra(s) : 0u));
    if (dhist)
        for (int s = 0; s < nd; ++s) data += (unsigned long long)dhist[s] * ((F.table[nll + s] >> 16) + dlz_distance_extra(s));
    F.hdr_bits = pos;
    F.data_bits = (unsigned int)data;
    const unsigned long long bits = pos + data + (F.table[256] >> 16);
    F.bytes = (unsigned int)(last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4);
}

// up to 32 bits at a bit position of the zeroed global word buffer
__device__ inline void dlz_or_bits(unsigned int *zw, unsigned int bitpos, unsigned int v, unsigned int nbits)
{
    const unsigned int sh = bitpos & 31u;
    atomicOr(&zw[bitpos >> 5], v << sh);
    if (sh + nbits > 32u) atomicOr(&zw[(bitpos >> 5) + 1], v >> (32u - sh));
}

// a lane's run of codes: a 64-bit accumulator flushed word by word; every add is at most 28 bits on fewer than 32 held
struct DlzSink {
    unsigned int *zw;
    unsigned long long acc;
    unsigned int nacc, w;
    __device__ inline void open(unsigned int *buf, unsigned int bitpos) { zw = buf; acc = 0; nacc = bitpos & 31u; w = bitpos >> 5; }
    __device__ inline void add(unsigned int v, unsigned int nbits)
    {
        acc |= (unsigned long long)v << nacc;
        nacc += nbits;
        if (nacc >= 32u) {
            atomicOr(&zw[w++], (unsigned int)acc);      // OR of disjoint bits: the result does not depend on order
            acc >>= 32;
            nacc -= 32u;
        }
    }
    __device__ inline void close() { if (nacc) atomicOr(&zw[w], (unsigned int)acc); }
};

// Arguments and results as deflate_segment's; every thread of the workgroup calls it with the same arguments.  z is 4-byte aligned
// and DEFLATE_ZCAP bytes long.
__device__ __forceinline__ void deflate_lz_segment(const uint8_t *__restrict__ in, const int n, const bool first, const bool last,
                                                   uint8_t *__restrict__ z, unsigned int *__restrict__ seglen, unsigned int *__restrict__ adl)
{
    __shared__ __attribute__((aligned(16))) unsigned int s_segw[DEFLATE_SEG / 4 + 2];   // the segment, and 8 bytes a word read may touch
    __shared__ uint8_t s_len[DEFLATE_SEG];                 // match length - 3 of a position's taken match
    __shared__ unsigned short s_dist[DEFLATE_SEG];         // its distance, 0 = no match taken (the hash rounds keep head + 1 here)
    __shared__ __attribute__((aligned(8))) unsigned int s_onpath[DEFLATE_SEG / 32];   // bit j: the greedy parse visits j (before step 4: the Adler sums' words)
    __shared__ __attribute__((aligned(16))) unsigned int s_pool[DLZ_POOL_WORDS];
    __shared__ unsigned int s_hm[288], s_hl[288], s_hd[32];   // histograms: matched literal/length, literal-only, distance
    __shared__ unsigned short s_entry[DLZ_PARSE_ROUND / DLZ_PARSE_BLOCK];
    static_assert(sizeof(s_onpath) >= 2 * (DLZ_THREADS / 64) * sizeof(unsigned long long), "adler_wg's words fit");
    __shared__ unsigned int s_pos;
    const int tid = threadIdx.x;
    const int pre = first ? 2 : 0;
    uint8_t *seg = reinterpret_cast<uint8_t *>(s_segw);

    // 1. stage, Adler sums
    if (tid == 0) s_pos = 0;
    {
        unsigned long long s1 = 0, s2 = 0;
        for (int j = tid; j < n; j += DLZ_THREADS) {
            const unsigned int b = in[j];
            seg[j] = (uint8_t)b;
            s1 += b;
            s2 += (unsigned long long)(n - j) * b;
        }
        adler_wg<DLZ_THREADS>(s1, s2, reinterpret_cast<unsigned long long *>(s_onpath));
        if (tid == 0) {
            adl[0] = (unsigned int)s1;
            adl[1] = (unsigned int)s2;
        }
    }
    auto word_at = [&](int p) -> unsigned int {          // the 4 bytes at p, little-endian (p + 3 may pass n: callers cap)
        const unsigned long long both = ((unsigned long long)s_segw[(p >> 2) + 1] << 32) | s_segw[p >> 2];
        return (unsigned int)(both >> ((p & 3) * 8));
    };
    auto match_len = [&](int a, int b, int cap) -> int { // common prefix of seg[a ..) and seg[b ..), a < b, b + cap <= n
        int k = 0;
        while (k < cap) {
            const unsigned int x = word_at(a + k) ^ word_at(b + k);
            if (x) { k += __builtin_ctz(x) >> 3; break; }
            k += 4;
        }
        return k < cap ? k : cap;
    };

    // 2. hash rounds
    unsigned int *head = s_pool;                          // position + 1, 0 = none
    for (int i = tid; i < (1 << DLZ_HASH_BITS); i += DLZ_THREADS) head[i] = 0;
    __syncthreads();
    const int nh = n - 3;                                 // positions below nh have a hash
    for (int t0 = 0; t0 < nh; t0 += DLZ_TILE) {
        const int j = t0 + tid;
        const bool act = tid < DLZ_TILE && j < nh;
        unsigned int h = 0;
        if (act) {
            h = (word_at(j) * 2654435761u) >> (32 - DLZ_HASH_BITS);
            s_dist[j] = (unsigned short)head[h];
        }
        __syncthreads();
        if (act) atomicMax(&head[h], (unsigned int)j + 1u);
        __syncthreads();
    }

    // 3. every position's best candidate
    for (int j = tid; j < n; j += DLZ_THREADS) {
        int blen = 0, bdist = 0;
        if (j <= n - DLZ_MIN_MATCH) {
            const int cap = n - j < DLZ_MAX_MATCH ? n - j : DLZ_MAX_MATCH;
            for (int d = 1; d <= 4; ++d) {
                if (j - d < 0 || blen == cap) break;
                const int l = match_len(j - d, j, cap);
                if (l > blen) { blen = l; bdist = d; }
            }
            if (j < nh && blen < cap) {
                const int c = (int)s_dist[j] - 1;
                if (c >= 0) {
                    const int l = match_len(c, j, cap);
                    if (l > blen) { blen = l; bdist = j - c; }
                }
            }
        }
        const bool take = blen >= DLZ_MIN_MATCH;
        s_len[j] = (uint8_t)(take ? blen - 3 : 0);
        s_dist[j] = (unsigned short)(take ? bdist : 0);
    }

    // 4. greedy parse: per round of 8192 positions, a lane per block of 64 resolves backwards where a walk entering at each
    // position leaves the block; one lane chains the blocks; each block marks its path
    unsigned short *ex = reinterpret_cast<unsigned short *>(s_pool);
    for (int base = 0; base < n; base += DLZ_PARSE_ROUND) {
        __syncthreads();
        const int bs = base + tid * DLZ_PARSE_BLOCK;
        const int be = bs + DLZ_PARSE_BLOCK < n ? bs + DLZ_PARSE_BLOCK : n;
        const bool mine = tid < DLZ_PARSE_ROUND / DLZ_PARSE_BLOCK;
        if (mine)
            for (int j = be - 1; j >= bs; --j) {
                const int nx = j + (s_dist[j] ? (int)s_len[j] + 3 : 1);
                ex[j - base] = (unsigned short)(nx >= be ? nx : ex[nx - base]);
            }
        __syncthreads();
        if (tid == 0) {
            int pos = (int)s_pos;
            for (int bk = 0; bk < DLZ_PARSE_ROUND / DLZ_PARSE_BLOCK; ++bk) {
                const int s = base + bk * DLZ_PARSE_BLOCK;
                const int e = s + DLZ_PARSE_BLOCK < n ? s + DLZ_PARSE_BLOCK : n;
                unsigned short entry = 0xFFFFu;
                if (pos >= s && pos < e) { entry = (unsigned short)pos; pos = ex[pos - base]; }
                s_entry[bk] = entry;
            }
            s_pos = (unsigned int)pos;
        }
        __syncthreads();
        if (mine) {
            unsigned long long mask = 0;
            int p = s_entry[tid];
            if (p != 0xFFFF)
                while (p < be) {
                    mask |= 1ull << (p - bs);
                    p += s_dist[p] ? (int)s_len[p] + 3 : 1;
                }
            s_onpath[bs >> 5] = (unsigned int)mask;
            s_onpath[(bs >> 5) + 1] = (unsigned int)(mask >> 32);
        }
    }
    __syncthreads();

    // 5. histograms
    for (int i = tid; i < 288; i += DLZ_THREADS) { s_hm[i] = 0; s_hl[i] = 0; }
    if (tid < 32) s_hd[tid] = 0;
    __syncthreads();
    for (int j = tid; j < n; j += DLZ_THREADS) {
        const unsigned int b = seg[j];
        atomicAdd(&s_hl[b], 1u);
        if (!((s_onpath[j >> 5] >> (j & 31)) & 1u)) continue;
        const unsigned int d = s_dist[j];
        if (d) {
            unsigned int s, eb, ev;
            dlz_length_symbol((unsigned)s_len[j] + 3u, s, eb, ev);
            atomicAdd(&s_hm[s], 1u);
            dlz_distance_symbol(d, s, eb, ev);
            atomicAdd(&s_hd[s], 1u);
        } else {
            atomicAdd(&s_hm[b], 1u);
        }
    }
    if (tid == 0) { s_hm[256] = 1; s_hl[256] = 1; }      // end of block (no other lane touches 256)
    __syncthreads();

    // 6. both forms' trees and headers: lane 0 the matched form, lane 64 (another wave) the literal-only form
    DlzForm &FM = *reinterpret_cast<DlzForm *>(s_pool);
    DlzForm &FL = *reinterpret_cast<DlzForm *>(reinterpret_cast<uint8_t *>(s_pool) + sizeof(DlzForm));
    unsigned int *scan = s_pool + (2 * sizeof(DlzForm) + 3) / 4;
    dlz_rank(s_hm, DLZ_NLL, FM.key, FM.sym, tid);
    dlz_rank(s_hd, DLZ_ND, FM.dkey, FM.dsym, tid);
    dlz_rank(s_hl, 257, FL.key, FL.sym, tid);
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const bool lz = tid == 0;
        dlz_build(lz ? FM : FL, lz ? s_hm : s_hl, lz ? DLZ_NLL : 257, lz ? s_hd : nullptr, lz ? DLZ_ND : 2, last);
    }
    __syncthreads();

    // 7. the shortest form; today's choice on a tie
    const unsigned int stored_bytes = (unsigned int)n + 5u;
    const bool matched = FM.bytes < FL.bytes && FM.bytes < stored_bytes;
    const bool huff = matched || FL.bytes <= stored_bytes;
    unsigned int body;
    if (huff) {
        const DlzForm &F = matched ? FM : FL;
        body = F.bytes;
        unsigned int *zw = reinterpret_cast<unsigned int *>(z);
        const unsigned int zwords = ((unsigned int)pre + body + 3u) / 4u;
        for (unsigned int i = tid; i < zwords; i += DLZ_THREADS) zw[i] = 0;
        const int chunk = (n + DLZ_THREADS - 1) / DLZ_THREADS;
        const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
        unsigned int bits = 0;
        for (int j = lo; j < hi; ++j) {
            if (!matched) { bits += F.table[seg[j]] >> 16; continue; }
            if (!((s_onpath[j >> 5] >> (j & 31)) & 1u)) continue;
            const unsigned int d = s_dist[j];
            if (d) {
                unsigned int s, eb, ev;
                dlz_length_symbol((unsigned)s_len[j] + 3u, s, eb, ev);
                bits += (F.table[s] >> 16) + eb;
                dlz_distance_symbol(d, s, eb, ev);
                bits += (F.table[DLZ_NLL + s] >> 16) + eb;
            } else {
                bits += F.table[seg[j]] >> 16;
            }
        }
        const unsigned int before = wg_exscan<DLZ_THREADS>(bits, scan);   // its barriers also make the zeroed words visible to the whole workgroup
        const unsigned int bit0 = 8u * (unsigned int)pre;
        DlzSink sink;
        sink.open(zw, bit0 + F.hdr_bits + before);
        for (int j = lo; j < hi; ++j) {
            if (!matched) { const unsigned int e = F.table[seg[j]]; sink.add(e & 0xFFFFu, e >> 16); continue; }
            if (!((s_onpath[j >> 5] >> (j & 31)) & 1u)) continue;
            const unsigned int d = s_dist[j];
            if (d) {
                unsigned int s, eb, ev;
                dlz_length_symbol((unsigned)s_len[j] + 3u, s, eb, ev);
                unsigned int e = F.table[s];
                sink.add((e & 0xFFFFu) | (ev << (e >> 16)), (e >> 16) + eb);
                dlz_distance_symbol(d, s, eb, ev);
                e = F.table[DLZ_NLL + s];
                sink.add((e & 0xFFFFu) | (ev << (e >> 16)), (e >> 16) + eb);
            } else {
                const unsigned int e = F.table[seg[j]];
                sink.add(e & 0xFFFFu, e >> 16);
            }
        }
        sink.close();
        const int hw = (int)((F.hdr_bits + 31u) / 32u);
        for (int i = tid; i < hw; i += DLZ_THREADS) dlz_or_bits(zw, bit0 + 32u * (unsigned int)i, F.hdr[i], 32u);
        if (tid == 0) {
            if (pre) atomicOr(&zw[0], 0x0178u);           // 78 01
            const unsigned int p = F.hdr_bits + F.data_bits;
            const unsigned int e = F.table[256];
            dlz_or_bits(zw, bit0 + p, e & 0xFFFFu, e >> 16);
            if (!last) {                                  // empty stored block: 3 zero bits, align, LEN 0000, NLEN FFFF
                const unsigned int q = (p + (e >> 16) + 3u + 7u) / 8u;
                dlz_or_bits(zw, bit0 + 8u * (q + 2u), 0xFFFFu, 16u);
            }
        }
    } else {
        // stored block: BFINAL / BTYPE 0 byte, LEN, NLEN, the bytes
        body = stored_bytes;
        if (tid == 0) {
            if (pre) { z[0] = 0x78; z[1] = 0x01; }
            z[pre] = last ? 1 : 0;
            z[pre + 1] = (uint8_t)(n & 255);
            z[pre + 2] = (uint8_t)(n >> 8);
            z[pre + 3] = (uint8_t)(~n & 255);
            z[pre + 4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int j = tid; j < n; j += DLZ_THREADS) z[pre + 5 + j] = seg[j];
    }
    if (tid == 0) *seglen = (unsigned int)pre + body + (last ? 4u : 0u);   // the last 4: Adler-32, written by the caller's frame or join step
}

}  // namespace lars
