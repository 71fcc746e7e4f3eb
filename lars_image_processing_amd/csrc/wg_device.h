// Workgroup-level building blocks shared by the kernels: prefix sums, two-value sums, the statistics partial.
//
// Common contract: one-dimensional workgroups of THREADS threads (a multiple of 64, at most 1024); EVERY thread of the
// workgroup calls the function, from uniform control flow (each contains barriers).  Each function names the LDS it needs;
// the caller owns it.  All of them begin with a barrier, so any of them may be called twice in a row on the same LDS.
#pragma once
#include "common.h"

namespace lars {

// Exclusive prefix sum of one value per thread, in thread order.  T = unsigned int or unsigned long long (integers: exact whatever
// the order of the additions).  LDS: s_w[THREADS / 64].  *total (optional, may be a local of each thread) = the sum over all threads.
// Wave scan by shuffles, one word per wave, two barriers.  The inclusive value is the result + v.
template <int THREADS, typename T>
__device__ inline T wg_exscan(T v, T *s_w, T *total = nullptr)
{
    static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves, one workgroup");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    __syncthreads();                                         // a second call must not overwrite sums still being read
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    T before = 0, all = 0;
    for (int i = 0; i < THREADS / 64; ++i) {
        if (i < wv) before += s_w[i];
        all += s_w[i];
    }
    if (total) *total = all;
    return before + incl - v;
}

// Exclusive prefix sum of n values by ONE workgroup of 1024 threads, chunk after chunk with a running carry in T:
// store(i, sum of load(0 .. i-1)) for every i < n; returns the total (to every thread).  load(i) is called once per i, before
// store(i, .) and by the same thread, so scanning in place is fine.  LDS: 17 words of T, declared here.  Per chunk: wave scans,
// the sixteen wave sums scanned by the first wave, three barriers (the last one lets the next chunk, or call, reuse the words).
template <typename T, typename Load, typename Store>
__device__ inline T wg_scan_array(long long n, Load load, Store store)
{
    __shared__ T wsum[16];
    __shared__ T chunk_sum;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    T carry = 0;
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + tid;
        const T v = i < n ? (T)load(i) : (T)0;
        T incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const T t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        if (wv == 0) {
            const T s = lane < 16 ? wsum[lane] : (T)0;
            T si = s;
            for (int d = 1; d < 16; d <<= 1) {
                const T t = __shfl_up(si, d);
                if (lane >= d) si += t;
            }
            if (lane < 16) wsum[lane] = si - s;
            if (lane == 15) chunk_sum = si;
        }
        __syncthreads();
        if (i < n) store(i, carry + wsum[wv] + incl - v);
        carry += chunk_sum;
        __syncthreads();
    }
    return carry;
}

// Sums of two 64-bit values per thread: on return thread 0 holds both sums in a and b (other threads: unspecified).
// LDS: s_w[2 * THREADS / 64].
template <int THREADS>
__device__ inline void wg_sum2(unsigned long long &a, unsigned long long &b, unsigned long long *s_w)
{
    static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole waves, one workgroup");
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_w[2 * (threadIdx.x >> 6)] = a; s_w[2 * (threadIdx.x >> 6) + 1] = b; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < THREADS / 64; ++w) { a += s_w[2 * w]; b += s_w[2 * w + 1]; }
}

// The tail of a rank select: per thread, the number of keys <= the selected key and the smallest key above it (~0 if none);
// on return thread 0 holds the workgroup's count and minimum.  LDS: s_w[2 * THREADS / 64].
template <int THREADS>
__device__ inline void wg_count_le_next(unsigned long long &c_le, unsigned long long &nxt, unsigned long long *s_w)
{
    for (int off = 32; off >= 1; off >>= 1) {
        c_le += __shfl_xor(c_le, off);
        const unsigned long long o = __shfl_xor(nxt, off);
        nxt = o < nxt ? o : nxt;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_w[2 * (threadIdx.x >> 6)] = c_le; s_w[2 * (threadIdx.x >> 6) + 1] = nxt; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < THREADS / 64; ++w) {
            c_le += s_w[2 * w];
            nxt = s_w[2 * w + 1] < nxt ? s_w[2 * w + 1] : nxt;
        }
}

// The seven-field statistics partial of an index array.  The order of the floating-point additions is fixed (butterfly offsets
// 32 .. 1 inside a wave, then waves 1, 2, 3 onto wave 0), so the double sums do not depend on timing.
struct StatPartial {
    double sum, sumsq, mn, mx;
    unsigned long long above, nans, count;
    unsigned long long pad;

    __device__ void init()
    {
        sum = 0; sumsq = 0; mn = __builtin_inf(); mx = -__builtin_inf(); above = 0; nans = 0; count = 0; pad = 0;
    }
    // one element; false (and only nans counted) for a NaN.  The two counters are stepped without a branch: a branch that
    // picks which member to increment becomes an indexed access, which puts the record into scratch memory.
    template <typename T>
    __device__ bool push(T v, T thr)
    {
        const bool ok = v == v;
        nans += ok ? 0 : 1;
        count += ok ? 1 : 0;
        if (ok) {
            const double d = (double)v;
            sum += d; sumsq += d * d;
            mn = fmin(mn, d); mx = fmax(mx, d);
            above += (v > thr) ? 1 : 0;
        }
        return ok;
    }
    __device__ void merge(const StatPartial &q)
    {
        sum += q.sum; sumsq += q.sumsq;
        mn = fmin(mn, q.mn); mx = fmax(mx, q.mx);
        above += q.above; nans += q.nans; count += q.count;
    }
    // every lane of the wave ends with the wave's partial
    __device__ void wave_reduce()
    {
        for (int off = 32; off >= 1; off >>= 1) {
            sum += __shfl_xor(sum, off); sumsq += __shfl_xor(sumsq, off);
            mn = fmin(mn, __shfl_xor(mn, off)); mx = fmax(mx, __shfl_xor(mx, off));
            above += __shfl_xor(above, off); nans += __shfl_xor(nans, off); count += __shfl_xor(count, off);
        }
    }
    // workgroup of 256 threads, every thread calls it: thread 0 ends with the workgroup's partial.  LDS: s_part[4].
    __device__ void block_reduce(StatPartial *s_part)
    {
        wave_reduce();
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = *this;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < 4; ++w) merge(s_part[w]);
    }
    // the record's scalar fields (not the histogram)
    __device__ void to_stats(lars_stats *out, double thr) const
    {
        out->sum = sum; out->sumsq = sumsq; out->count = count + nans; out->above = above; out->nans = nans;
        out->min = mn; out->max = mx; out->threshold = thr; out->index_id = 0xFFFFFFFFu; out->reserved = 0;
    }
};

}  // namespace lars
