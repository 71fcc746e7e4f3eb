// The checksums of the file formats, by a workgroup: CRC-32 (PNG chunks), Adler-32 (zlib streams), and the one table both
// TIFF coders share.  Built on wg_device.h, whose calling contract holds here too: every thread of the workgroup calls the
// wg_ / _wg functions, from uniform control flow.
#pragma once
#include "wg_device.h"

namespace lars {

// ---- CRC-32 (reflected, polynomial 0xEDB88320) -------------------------------------------------------------------------
constexpr unsigned int CRC32_POLY = 0xEDB88320u;

// tab[256] in LDS, filled by all nthreads threads; a barrier must follow before crc_update reads it
__device__ inline void crc_table_fill(unsigned int *tab, int tid, int nthreads)
{
    for (int i = tid; i < 256; i += nthreads) {
        unsigned int c = (unsigned int)i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC32_POLY : c >> 1;
        tab[i] = c;
    }
}

__device__ inline unsigned int crc_update(const unsigned int *tab, unsigned int crc, unsigned int byte)
{
    return tab[(crc ^ byte) & 255u] ^ (crc >> 8);
}

// a * b mod P (reflected)
__device__ inline unsigned int crc_multmodp(unsigned int a, unsigned int b)
{
    unsigned int m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ CRC32_POLY : b >> 1;
    }
    return p;
}

// x2n[i] = x^(2^i) mod P, i < 32: by ONE thread; a barrier must follow before crc_x2nmodp reads it
__device__ inline void crc_x2n_fill(unsigned int *x2n)
{
    unsigned int p = 1u << 30;                   // x^1
    x2n[0] = p;
    for (int i = 1; i < 32; ++i) x2n[i] = p = crc_multmodp(p, p);
}

// x^(n * 2^k) mod P
__device__ inline unsigned int crc_x2nmodp(const unsigned int *x2n, unsigned long long n, unsigned int k)
{
    unsigned int p = 1u << 31;
    while (n) {
        if (n & 1) p = crc_multmodp(x2n[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}

// The finished CRC-32 of the len bytes byte_at(0 .. len - 1), returned to thread 0 (other threads: unspecified).  Each thread
// takes a contiguous piece; crc(A B) = crc(A) x^(8 |B|) ^ crc(B) for finished CRCs, so a piece is shifted by the bytes behind
// it and the pieces XOR together.  tab and x2n (crc_table_fill, crc_x2n_fill) are in LDS and visible.  LDS: part[THREADS / 64].
template <int THREADS, typename ByteAt>
__device__ inline unsigned int wg_crc32(unsigned int len, ByteAt byte_at, const unsigned int *tab, const unsigned int *x2n,
                                        unsigned int *part)
{
    const unsigned int tid = threadIdx.x;
    const unsigned int chunk = (len + THREADS - 1) / THREADS;
    const unsigned int lo = min(len, tid * chunk), hi = min(len, lo + chunk);
    unsigned int crc = 0xFFFFFFFFu;
    for (unsigned int j = lo; j < hi; ++j) crc = crc_update(tab, crc, byte_at(j));
    crc = hi > lo ? ~crc : 0u;
    unsigned int piece = crc ? crc_multmodp(crc_x2nmodp(x2n, len - hi, 3), crc) : 0u;
    for (int off = 32; off >= 1; off >>= 1) piece ^= __shfl_xor(piece, off);
    __syncthreads();
    if ((tid & 63u) == 0) part[tid >> 6] = piece;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < THREADS / 64; ++w) piece ^= part[w];
    return piece;
}

// ---- Adler-32 ----------------------------------------------------------------------------------------------------------
// Of bytes x_0 .. x_(n-1): low half 1 + A, high half n + B, with A = sum x_j and B = sum (n - j) x_j, all mod 65521.
constexpr unsigned long long ADLER_MOD = 65521ull;

// Per-thread sums s1, s2 (any 64-bit values) -> on thread 0, their workgroup sums mod 65521.  LDS: s_w[2 * THREADS / 64].
template <int THREADS>
__device__ inline void adler_wg(unsigned long long &s1, unsigned long long &s2, unsigned long long *s_w)
{
    s1 %= ADLER_MOD;
    s2 %= ADLER_MOD;
    wg_sum2<THREADS>(s1, s2, s_w);                // at most 1024 residues: far from overflow
    s1 %= ADLER_MOD;
    s2 %= ADLER_MOD;
}

// (A, B) of a stream so far, mod 65521, extended by a segment with sums (a_k, b_k) that has bytes_after bytes of the stream
// behind it: B is kept relative to the END of the whole stream, so segments may be appended in any order.
__device__ inline void adler_append(unsigned long long &A, unsigned long long &B, unsigned long long a_k, unsigned long long b_k,
                                    unsigned long long bytes_after)
{
    A = (A + a_k) % ADLER_MOD;
    B = (B + b_k + (bytes_after % ADLER_MOD) * (a_k % ADLER_MOD)) % ADLER_MOD;
}

// the checksum of a stream of n bytes from its (A, B), each below 2^63
__device__ inline unsigned int adler_value(unsigned long long A, unsigned long long B, unsigned long long n)
{
    const unsigned int s1 = (unsigned int)((1ull + A) % ADLER_MOD);
    const unsigned int s2 = (unsigned int)((n % ADLER_MOD + B % ADLER_MOD) % ADLER_MOD);
    return (s2 << 16) | s1;
}

// ---- TIFF LZW ----------------------------------------------------------------------------------------------------------
// width in bits of the i-th code after a Clear (TIFF's early change: the width grows one code early)
__device__ inline int tiff_lzw_width(unsigned long long i) { return i <= 253 ? 9 : i <= 765 ? 10 : i <= 1789 ? 11 : 12; }

}  // namespace lars
