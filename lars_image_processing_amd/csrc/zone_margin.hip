// Zone margins (DESIGN.md "Zone margins"): the labels of the zone stages with every zone shrunk inward by a distance, so that the
// mixed pixels along a plot's edge stay out of its figures.
//
// The definition.  Labels are L[h][w], 0 = in no zone.  For a pixel p with L(p) != 0, D2(p) is the smallest (di)^2 + (dj)^2 to a
// pixel q of the raster with L(q) != L(p); no such pixel: infinity (outside the raster there are no pixels).  With margin2 = m2 the
// shrunk labels are L'(p) = L(p) if D2(p) > m2, else 0.  Integers only: the same bytes on every run.
//
// Two kernels, r = floor(sqrt(m2)) <= ZM_MARGIN_MAX:
//   k_zm_column  g[i][j] = rows from (i, j) to the nearest pixel of column j with another label, up or down, as far as it matters: a
//                distance above r is written as 255, and so is "none before the raster ends".  One thread per column and segment
//                of rows: it looks back r rows for the run it starts in, walks down, looks ahead r rows and walks up again.
//   k_zm_row     D2(i, j) <= m2 iff some k with k^2 <= m2 has, at column j + k or j - k of row i, another label (k^2 <= m2) or the
//                same label with k^2 + g^2 <= m2; a side ends at the first other label and at the raster's edge.  One workgroup per
//                stretch of ZM_TILE columns of a row, whose labels and g stand in LDS with r columns on either side.  The result
//                goes to a second buffer: the neighbours still read the labels.
//
// Every row and column is held inside the raster and every LDS index inside the stretch read: k <= r <= ZM_MARGIN_MAX.
#include "common.h"

namespace lars {

namespace {

#define ZM_THREADS 256
#define ZM_SEG 32                       // rows of a column segment; a margin above it takes segments of r rows
#define ZM_TILE 256                     // columns of a row stretch: one per thread
#define ZM_MARGIN_MAX 254               // r at most: g fits a byte that saturates at 255, and 255^2 > 254^2
#define ZM_MARGIN2_MAX (ZM_MARGIN_MAX * ZM_MARGIN_MAX)

template <typename T>
__global__ __launch_bounds__(ZM_THREADS) void k_zm_column(const T *__restrict__ labels, long long h, long long w, int r, int seg, long long col_tiles,
                                                          uint8_t *__restrict__ g)
{
    const long long tile = blockIdx.x % col_tiles, band = blockIdx.x / col_tiles;
    const long long j = tile * ZM_THREADS + threadIdx.x;
    if (j >= w) return;
    const long long i0 = band * seg, i1 = i0 + seg < h ? i0 + seg : h;
    // down the segment: the rows to the last other label above
    T prev = labels[i0 * w + j];
    int up = 255;
    for (int k = 1; k <= r && i0 - k >= 0; ++k)
        if (labels[(i0 - k) * w + j] != prev) {
            up = k;
            break;
        }
    g[i0 * w + j] = (uint8_t)up;
    for (long long i = i0 + 1; i < i1; ++i) {
        const T a = labels[i * w + j];
        up = a != prev ? 1 : up < 255 ? up + 1 : 255;
        g[i * w + j] = (uint8_t)up;
        prev = a;
    }
    // and up again: the rows to the next other label below, the smaller of the two kept
    int down = 255;
    for (int k = 1; k <= r && i1 - 1 + k < h; ++k)
        if (labels[(i1 - 1 + k) * w + j] != prev) {
            down = k;
            break;
        }
    for (long long i = i1 - 1; i >= i0; --i) {
        const T a = labels[i * w + j];
        if (i < i1 - 1) down = a != prev ? 1 : down < 255 ? down + 1 : 255;
        const int above = g[i * w + j];
        if (down < above) g[i * w + j] = (uint8_t)down;
        prev = a;
    }
}

template <typename T>
__global__ __launch_bounds__(ZM_THREADS) void k_zm_row(const T *__restrict__ labels, const uint8_t *__restrict__ g, long long w, int r, int m2,
                                                       long long row_tiles, T *__restrict__ out)
{
    __shared__ int s_lab[ZM_TILE + 2 * ZM_MARGIN_MAX];
    __shared__ uint8_t s_g[ZM_TILE + 2 * ZM_MARGIN_MAX];
    const long long i = blockIdx.x / row_tiles, j0 = (blockIdx.x % row_tiles) * ZM_TILE;
    const long long lo = j0 - r > 0 ? j0 - r : 0, hi = j0 + ZM_TILE + r < w ? j0 + ZM_TILE + r : w;
    const long long row = i * w;
    const int n = (int)(hi - lo);                                  // at most ZM_TILE + 2 r
    for (int x = threadIdx.x; x < n; x += ZM_THREADS) {
        s_lab[x] = (int)labels[row + lo + x];
        s_g[x] = g[row + lo + x];
    }
    __syncthreads();
    const long long j = j0 + threadIdx.x;
    if (j >= w) return;
    const int x = (int)(j - lo);
    const int a = s_lab[x];
    if (a == 0) {
        out[row + j] = (T)0;
        return;
    }
    const int g0 = s_g[x];
    bool gone = g0 * g0 <= m2;
    // k <= r: k^2 <= m2, and x + k, x - k stay inside what was read as long as the column is one of the raster
    for (int k = 1; !gone && k <= r && j + k < w; ++k) {
        if (s_lab[x + k] != a) {
            gone = true;
            break;
        }
        const int gk = s_g[x + k];
        gone = k * k + gk * gk <= m2;
    }
    for (int k = 1; !gone && k <= r && j - k >= 0; ++k) {
        if (s_lab[x - k] != a) {
            gone = true;
            break;
        }
        const int gk = s_g[x - k];
        gone = k * k + gk * gk <= m2;
    }
    out[row + j] = gone ? (T)0 : (T)a;
}

template <typename T>
void zm_launch(const void *labels, long long h, long long w, int r, int m2, uint8_t *g, void *out, hipStream_t s)
{
    const int seg = r > ZM_SEG ? r : ZM_SEG;
    const long long tiles = (w + ZM_TILE - 1) / ZM_TILE, bands = (h + seg - 1) / seg;
    hipLaunchKernelGGL((k_zm_column<T>), dim3((unsigned)(tiles * bands)), dim3(ZM_THREADS), 0, s, static_cast<const T *>(labels), h, w, r, seg, tiles, g);
    hipLaunchKernelGGL((k_zm_row<T>), dim3((unsigned)(tiles * h)), dim3(ZM_THREADS), 0, s, static_cast<const T *>(labels), g, w, r, m2, tiles,
                       static_cast<T *>(out));
}

}  // namespace

}  // namespace lars

using namespace lars;

extern "C" int lars_d_zone_shrink(const void *labels, int zone_bytes, int64_t h, int64_t w, int64_t margin2, void *g_scratch, void *out, void *stream)
{
    static const char *who = "lars_d_zone_shrink";
    static_assert(ZM_TILE == ZM_THREADS, "one column of a stretch per thread");
    static_assert(ZM_MARGIN2_MAX == LARS_ZONE_MARGIN2_MAX, "the header's cap is the kernels'");
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!labels || !g_scratch || !out || out == labels || h <= 0 || w <= 0 || (zone_bytes != 1 && zone_bytes != 2 && zone_bytes != 4) ||
        !aligned_to(labels, (uintptr_t)zone_bytes) || !aligned_to(out, (uintptr_t)zone_bytes))
        return fail(LARS_ERR_INVALID, "%s: bad arguments (labels of 1, 2 or 4 bytes, a second buffer for the result)", who);
    if (margin2 < 0 || margin2 > ZM_MARGIN2_MAX) return fail(LARS_ERR_INVALID, "%s: margin2 must be 0 to %d, got %lld", who, ZM_MARGIN2_MAX, (long long)margin2);
    const int64_t tiles = (w + ZM_TILE - 1) / ZM_TILE;
    if (h > (int64_t)1 << 24 || w > (int64_t)1 << 24 || tiles * h > 0x7FFFFFFF)
        return fail(LARS_ERR_INVALID, "%s: the raster is 1 to 2^24 on each side and has fewer than 2^31 stretches of %d columns", who, ZM_TILE);
    int r = 0;
    while ((int64_t)(r + 1) * (r + 1) <= margin2) ++r;
    hipStream_t s = pick_stream(c, stream);
    uint8_t *g = static_cast<uint8_t *>(g_scratch);
    if (zone_bytes == 1) zm_launch<uint8_t>(labels, h, w, r, (int)margin2, g, out, s);
    else if (zone_bytes == 2) zm_launch<uint16_t>(labels, h, w, r, (int)margin2, g, out, s);
    else zm_launch<int32_t>(labels, h, w, r, (int)margin2, g, out, s);
    return launch_check(who);
}
