// The workgroup primitives of wg_device.h and checksum_device.h, each run by one workgroup on device buffers, so that
// tests/test_gpu_wg.py can check their contracts at sizes the product's pictures do not reach.
#include "../checksum_device.h"
#include "lab.h"

namespace lars {
namespace {

// out[0 .. T) = prefixes of in, out[T] = total; then a second call on the inclusive values: out[T + 1 .. 2T + 1), out[2T + 1]
template <int THREADS, typename T>
__global__ __launch_bounds__(THREADS) void k_chk_exscan(const T *in, T *out)
{
    __shared__ T s_w[THREADS / 64];
    const int tid = threadIdx.x;
    T total, total2;
    const T v = in[tid], before = wg_exscan<THREADS>(v, s_w, &total);
    const T before2 = wg_exscan<THREADS>((T)(before + v), s_w, &total2);
    out[tid] = before;
    out[THREADS + 1 + tid] = before2;
    if (tid == 0) { out[THREADS] = total; out[2 * THREADS + 1] = total2; }
}

__global__ __launch_bounds__(1024) void k_chk_scan_widen(const unsigned int *in, unsigned long long *out, long long n)
{
    const unsigned long long t = wg_scan_array<unsigned long long>(n, [&](long long i) { return in[i]; }, [&](long long i, unsigned long long b) { out[i] = b; });
    if (threadIdx.x == 0) out[n] = t;
}

// k_pd_scan_u32's use: in place, the stored prefix saturates, v[n] = min(total, cap)
__global__ __launch_bounds__(1024) void k_chk_scan_saturating(unsigned int *v, long long n, unsigned long long cap)
{
    const unsigned long long t = wg_scan_array<unsigned long long>(
        n, [&](long long i) { return v[i]; }, [&](long long i, unsigned long long b) { v[i] = (unsigned int)min(b, 0xFFFFFFFFull); });
    if (threadIdx.x == 0) v[n] = (unsigned int)min(t, cap);
}

__global__ __launch_bounds__(256) void k_chk_crc32(const uint8_t *in, unsigned int *out, unsigned int n)
{
    __shared__ unsigned int tab[256], x2n[32], part[4];
    crc_table_fill(tab, threadIdx.x, 256);
    if (threadIdx.x == 0) crc_x2n_fill(x2n);
    __syncthreads();
    const unsigned int crc = wg_crc32<256>(n, [&](unsigned int j) { return (unsigned int)in[j]; }, tab, x2n, part);
    if (threadIdx.x == 0) out[0] = crc;
}

// the Adler-32 of in[0 .. n) joined from the segments [0, cut1), [cut1, cut2), [cut2, n)
__global__ __launch_bounds__(256) void k_chk_adler(const uint8_t *in, unsigned int *out, long long n, long long cut1, long long cut2)
{
    __shared__ unsigned long long s_w[8];
    const long long cut[4] = {0, cut1, cut2, n};
    unsigned long long A = 0, B = 0;
    for (int k = 0; k < 3; ++k) {
        unsigned long long s1 = 0, s2 = 0;
        for (long long j = cut[k] + threadIdx.x; j < cut[k + 1]; j += 256) { s1 += in[j]; s2 += (unsigned long long)(cut[k + 1] - j) * in[j]; }
        adler_wg<256>(s1, s2, s_w);
        adler_append(A, B, s1, s2, (unsigned long long)(n - cut[k + 1]));
    }
    if (threadIdx.x == 0) out[0] = adler_value(A, B, (unsigned long long)n);
}

template <typename T>
void exscan_launch(int threads, const void *in, void *out, hipStream_t s)
{
    const T *i = static_cast<const T *>(in);
    T *o = static_cast<T *>(out);
    if (threads == 64) hipLaunchKernelGGL((k_chk_exscan<64, T>), dim3(1), dim3(64), 0, s, i, o);
    else if (threads == 256) hipLaunchKernelGGL((k_chk_exscan<256, T>), dim3(1), dim3(256), 0, s, i, o);
    else hipLaunchKernelGGL((k_chk_exscan<1024, T>), dim3(1), dim3(1024), 0, s, i, o);
}

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" int lars_lab_wg_check(int prim, const void *in, void *out, int64_t n, uint64_t a, uint64_t b, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    hipStream_t s = pick_stream(c, stream);
    const bool exscan = prim == LARS_LAB_WG_EXSCAN32 || prim == LARS_LAB_WG_EXSCAN64;
    if (!out || (!in && prim != LARS_LAB_WG_SCAN_SATURATING) || n < 0 || (exscan && n != 64 && n != 256 && n != 1024) ||
        ((prim == LARS_LAB_WG_CRC32 || prim == LARS_LAB_WG_ADLER) && n >= (1ll << 31)) || (prim == LARS_LAB_WG_ADLER && !(a <= b && b <= (uint64_t)n)))
        return fail(LARS_ERR_INVALID, "lars_lab_wg_check: bad arguments");
    switch (prim) {
    case LARS_LAB_WG_EXSCAN32: exscan_launch<unsigned int>((int)n, in, out, s); break;
    case LARS_LAB_WG_EXSCAN64: exscan_launch<unsigned long long>((int)n, in, out, s); break;
    case LARS_LAB_WG_SCAN_WIDEN:
        hipLaunchKernelGGL(k_chk_scan_widen, dim3(1), dim3(1024), 0, s, static_cast<const unsigned int *>(in), static_cast<unsigned long long *>(out), (long long)n);
        break;
    case LARS_LAB_WG_SCAN_SATURATING:
        hipLaunchKernelGGL(k_chk_scan_saturating, dim3(1), dim3(1024), 0, s, static_cast<unsigned int *>(out), (long long)n, (unsigned long long)a);
        break;
    case LARS_LAB_WG_CRC32:
        hipLaunchKernelGGL(k_chk_crc32, dim3(1), dim3(256), 0, s, static_cast<const uint8_t *>(in), static_cast<unsigned int *>(out), (unsigned int)n);
        break;
    case LARS_LAB_WG_ADLER:
        hipLaunchKernelGGL(k_chk_adler, dim3(1), dim3(256), 0, s, static_cast<const uint8_t *>(in), static_cast<unsigned int *>(out), (long long)n, (long long)a, (long long)b);
        break;
    default: return fail(LARS_ERR_INVALID, "lars_lab_wg_check: primitive %d", prim);
    }
    return launch_check("lars_lab_wg_check");
}
