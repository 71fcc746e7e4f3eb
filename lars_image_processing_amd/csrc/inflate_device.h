// Deflate pieces the PNG decoder (png_decode.hip) and the TIFF decoder (tiff_decode.hip) share: the bit reader, the constant
// tables, zlib's acceptance rules for code-length sets, the block-header parser and the Huffman tables of one block in LDS.
// Device code only; every function here is used by one lane (pd_header) or by a whole wave (pd_fast_tables) as it says.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lars {

#define PD_FB 10                       // bits of the first-level Huffman lookup (longer codes: canonical bit-by-bit decode)

// ---- bit reader (LSB first) ------------------------------------------------------------------------------------------
// ALIGNED: over a stream of nw 32-bit words on a 16-byte boundary that is padded with zero words (the gathered PNG stream).
// !ALIGNED: over nw BYTES that start at any address (a strip inside a TIFF file); w points at the first byte and is never
// dereferenced as a word.  No byte at or past nw is loaded; the reader gives zero bits there.  It keeps two words ahead in
// scalars (a0, a1) instead of the quads, so the whole reader stays in registers.
template <bool ALIGNED>
struct BitReaderT {
    const unsigned int *w;
    unsigned long long nw, wt, buf;      // wt: the next word to take
    uint4 cur, nxt;                      // ALIGNED: the aligned quad holding word wt and the one after it (loaded ahead)
    unsigned int a0, a1;                 // !ALIGNED: words wt and wt + 1 (loaded ahead)
    int cnt;
    __device__ __forceinline__ unsigned int word_at(unsigned long long at) const      // !ALIGNED: bytes at .. at + 3, zero from nw on
    {
        const uint8_t *b = reinterpret_cast<const uint8_t *>(w);
        unsigned int x = 0;
        if (at + 4 <= nw) {
            __builtin_memcpy(&x, b + at, 4);
        } else {
            if (at < nw) x = b[at];
            if (at + 1 < nw) x |= (unsigned int)b[at + 1] << 8;
            if (at + 2 < nw) x |= (unsigned int)b[at + 2] << 16;
        }
        return x;
    }
    __device__ __forceinline__ uint4 quad(unsigned long long q) const
    {
        return q + 4 <= nw ? *reinterpret_cast<const uint4 *>(w + q) : make_uint4(0u, 0u, 0u, 0u);
    }
    __device__ __forceinline__ unsigned int take()
    {
        if (!ALIGNED) {
            const unsigned int v = a0;
            ++wt;
            a0 = a1;
            a1 = word_at((wt + 1) * 4);
            return v;
        }
        const unsigned int v = (wt & 2) ? ((wt & 1) ? cur.w : cur.z) : ((wt & 1) ? cur.y : cur.x);
        ++wt;
        if ((wt & 3) == 0) { cur = nxt; nxt = quad(wt + 4); }
        return v;
    }
    __device__ __forceinline__ void init(const unsigned int *words, unsigned long long nwords, unsigned long long pos)
    {
        w = words; nw = nwords; wt = pos >> 5;
        if (ALIGNED) {
            cur = quad(wt & ~3ull);
            nxt = quad((wt & ~3ull) + 4);
        } else {
            a0 = word_at(wt * 4);
            a1 = word_at(wt * 4 + 4);
        }
        const int sh = (int)(pos & 31);
        buf = (unsigned long long)take() >> sh;
        cnt = 32 - sh;
        refill();
    }
    __device__ __forceinline__ void refill()
    {
        if (cnt <= 32) {
            buf |= (unsigned long long)take() << cnt;
            cnt += 32;
        }
    }
    __device__ __forceinline__ unsigned int bits(int n)                 // n <= 32 - with at least n bits in buf
    {
        const unsigned int v = (unsigned int)(buf & ((1ull << n) - 1));
        buf >>= n; cnt -= n;
        return v;
    }
    __device__ __forceinline__ unsigned int need(int n) { if (cnt < n) refill(); return bits(n); }
    __device__ __forceinline__ unsigned long long pos() const { return wt * 32 - (unsigned long long)cnt; }
};
typedef BitReaderT<true> BitReader;

static __constant__ unsigned short c_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                                                  131, 163, 195, 227, 258};
static __constant__ unsigned char c_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static __constant__ unsigned short c_dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                                  2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static __constant__ unsigned char c_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static __constant__ unsigned char c_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// canonical decode, one bit at a time (puff's algorithm); count[1..maxlen], symbols sorted by (length, value); -1: no code
__device__ __forceinline__ int pd_slow_decode(unsigned long long b, const unsigned short *count, const unsigned short *sym, int maxlen, int *used)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= maxlen; ++len) {
        code |= (int)(b & 1); b >>= 1;
        const int c = count[len];
        if (code - c < first) { *used = len; return sym[index + (code - first)]; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}

// zlib's inflate_table acceptance: 0 ok, 1 over-subscribed or incomplete (except a single code of length 1 for lengths and
// distances; an empty distance code is accepted and fails when used)
__device__ inline int pd_code_check(const unsigned short *count, bool codes)
{
    int max = 15;
    while (max >= 1 && count[max] == 0) --max;
    if (max == 0) return codes ? 1 : 0;
    int left = 1;
    for (int len = 1; len <= 15; ++len) {
        left <<= 1;
        left -= count[len];
        if (left < 0) return 1;
    }
    if (left > 0 && (codes || max != 1)) return 1;
    return 0;
}

// ---- the header and the Huffman tables of one block, in LDS ----------------------------------------------------------
struct PdCodes {
    unsigned short lfast[1 << PD_FB], dfast[1 << PD_FB];
    unsigned short lcnt[16], dcnt[16], lsym[288], dsym[32], clcnt[16], clsym[19];
    unsigned char lens[320];
    // the header, written by one lane
    int kind, err, final_;
    unsigned long long data_pos;
    unsigned int stored_len;
};

// one lane: the block header at pos into L (kind 0 stored, 1 fixed, 2 dynamic; err 0, 1 block type, 2 LEN / NLEN, 3 code
// lengths, 5 the input ends first).  STOP_FIRST: a value is judged only when all its bits lie in front of nbits, as zlib
// judges it -- where a value is both cut off and wrong the answer is 5, not 1 .. 3 -- and a stored block whose bytes are
// cut off still leaves data_pos (non-zero) and stored_len.  Without it the order is the PNG decoder's, for which either
// answer fails the file.
template <bool ALIGNED, bool STOP_FIRST>
__device__ void pd_header_t(PdCodes &L, const unsigned int *words, unsigned long long nw, unsigned long long nbits, unsigned long long pos)
{
    L.err = 0;
    if (STOP_FIRST) L.data_pos = 0;
    if (pos + 3 > nbits) { L.err = 5; return; }
    BitReaderT<ALIGNED> br;
    br.init(words, nw, pos);
    L.final_ = (int)br.bits(1);
    const int type = (int)br.bits(2);
    L.kind = type;
    if (type == 3) { L.err = 1; return; }
    if (type == 0) {
        const unsigned long long p = (br.pos() + 7) & ~7ull;
        if (p + 32 > nbits) { L.err = 5; return; }
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words);
        const unsigned int len = bytes[p / 8] | (unsigned int)bytes[p / 8 + 1] << 8;
        const unsigned int nlen = bytes[p / 8 + 2] | (unsigned int)bytes[p / 8 + 3] << 8;
        if (len != (~nlen & 0xFFFFu)) { L.err = 2; return; }
        L.data_pos = p + 32;
        L.stored_len = len;
        if (L.data_pos + 8ull * len > nbits) { L.err = 5; return; }
        return;
    }
    int nlen = 288, ndist = 32;
    if (type == 1) {
        for (int i = 0; i < 288; ++i) L.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        for (int i = 0; i < 32; ++i) L.lens[288 + i] = 5;
    } else {
        nlen = (int)br.bits(5) + 257;
        ndist = (int)br.bits(5) + 1;
        const int ncode = (int)br.bits(4) + 4;
        if (STOP_FIRST && br.pos() > nbits) { L.err = 5; return; }
        if (nlen > 286 || ndist > 30) { L.err = 3; return; }
        unsigned char cl[19];
        for (int i = 0; i < 19; ++i) cl[i] = 0;
        for (int i = 0; i < ncode; ++i) cl[c_clorder[i]] = (unsigned char)br.need(3);
        if (STOP_FIRST && br.pos() > nbits) { L.err = 5; return; }
        for (int i = 0; i < 16; ++i) L.clcnt[i] = 0;
        for (int i = 0; i < 19; ++i) L.clcnt[cl[i]]++;
        L.clcnt[0] = 0;
        if (pd_code_check(L.clcnt, true)) { L.err = 3; return; }
        unsigned short offs[16];
        offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + L.clcnt[l];
        for (int s = 0; s < 19; ++s) if (cl[s]) L.clsym[offs[cl[s]]++] = (unsigned short)s;
        unsigned char tmp[316];
        int idx = 0;
        const int n = nlen + ndist;
        while (idx < n) {
            br.refill();
            int used = 0;
            const int s = pd_slow_decode(br.buf, L.clcnt, L.clsym, 7, &used);
            if (s < 0) { L.err = 3; return; }
            br.bits(used);
            int len, rep;
            if (s < 16) { len = s; rep = 1; }
            else if (s == 16) {
                if (!STOP_FIRST && idx == 0) { L.err = 3; return; }
                len = idx ? tmp[idx - 1] : 0;
                rep = 3 + (int)br.bits(2);
            }
            else if (s == 17) { len = 0; rep = 3 + (int)br.bits(3); }
            else { len = 0; rep = 11 + (int)br.bits(7); }
            if (STOP_FIRST && br.pos() > nbits) { L.err = 5; return; }
            if (STOP_FIRST && s == 16 && idx == 0) { L.err = 3; return; }
            if (idx + rep > n) { L.err = 3; return; }
            for (int k = 0; k < rep; ++k) tmp[idx++] = (unsigned char)len;
            if (br.pos() > nbits) { L.err = 5; return; }
        }
        for (int i = 0; i < 288; ++i) L.lens[i] = i < nlen ? tmp[i] : 0;
        for (int i = 0; i < 32; ++i) L.lens[288 + i] = i < ndist ? tmp[nlen + i] : 0;
        if (L.lens[256] == 0) { L.err = 3; return; }
    }
    for (int i = 0; i < 16; ++i) { L.lcnt[i] = 0; L.dcnt[i] = 0; }
    for (int i = 0; i < 288; ++i) L.lcnt[L.lens[i]]++;
    for (int i = 0; i < 32; ++i) L.dcnt[L.lens[288 + i]]++;
    L.lcnt[0] = 0; L.dcnt[0] = 0;
    if (pd_code_check(L.lcnt, false) || pd_code_check(L.dcnt, false)) { L.err = 3; return; }
    unsigned short lo[16], dof[16];
    lo[1] = 0; dof[1] = 0;
    for (int l = 1; l < 15; ++l) { lo[l + 1] = lo[l] + L.lcnt[l]; dof[l + 1] = dof[l] + L.dcnt[l]; }
    for (int s = 0; s < 288; ++s) if (L.lens[s]) L.lsym[lo[L.lens[s]]++] = (unsigned short)s;
    for (int s = 0; s < 32; ++s) if (L.lens[288 + s]) L.dsym[dof[L.lens[288 + s]]++] = (unsigned short)s;
    L.data_pos = br.pos();
}

// all lanes: first-level tables, entry = symbol << 4 | length, 0 for "longer than PD_FB bits or no code"
__device__ __forceinline__ void pd_fast_tables(PdCodes &L)
{
    for (int e = threadIdx.x; e < (1 << PD_FB); e += blockDim.x) {
        int used = 0;
        int s = pd_slow_decode((unsigned long long)e, L.lcnt, L.lsym, PD_FB, &used);
        L.lfast[e] = s < 0 ? 0 : (unsigned short)(s << 4 | used);
        s = pd_slow_decode((unsigned long long)e, L.dcnt, L.dsym, PD_FB, &used);
        L.dfast[e] = s < 0 ? 0 : (unsigned short)(s << 4 | used);
    }
}

// one symbol at the reader's position; -1 (and nothing consumed): no code starts with these bits
template <bool ALIGNED>
__device__ __forceinline__ int pd_symbol(BitReaderT<ALIGNED> &br, const unsigned short *fast, const unsigned short *cnt, const unsigned short *sym)
{
    const unsigned short v = fast[br.buf & ((1u << PD_FB) - 1)];
    if (v) { br.bits(v & 15); return v >> 4; }
    int used = 0;
    const int s = pd_slow_decode(br.buf, cnt, sym, 15, &used);
    if (s >= 0) br.bits(used);
    return s;
}

}  // namespace lars
