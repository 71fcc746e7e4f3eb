// Sampled white-balance tables (wb_predict.hip): what the predictor, the gated exact pass (fused_v2.hip, fused.hip) and the
// verifying plane-writing kernel (fused.hip) share -- the rank arithmetic of np.percentile, the condition that proves a
// predicted percentile exact, the gate, the table fill and the reset of a statistics record.
#pragma once
#include "common.h"
#include "device_common.h"

namespace lars {

// np.percentile(x, q), method 'linear', of n values: virtual index (n-1)*q in float64, order statistics lo = floor(vi) and
// hi = lo+1 (clamped), weight t = vi - lo.  k: 0 = the 2 % mark, 1 = the 98 % mark.
__device__ inline void wb_mark_ranks(long long npix, int k, long long &lo, long long &hi, double &t)
{
    const double q = (k == 0 ? 2.0 : 98.0) / 100.0;
    const double vi = (double)(npix - 1) * q;
    const double fl = floor(vi);
    lo = (long long)fl;
    hi = lo + 1;
    if (hi > npix - 1) hi = npix - 1;
    t = vi - fl;
}

// _lerp of numpy: a + (b-a)*t, and b - (b-a)*(1-t) where t >= 0.5
__device__ inline double wb_lerp(double a, double b, double t)
{
    const double d = b - a;
    double r = a + d * t;
    if (t >= 0.5) r = b - d * (1.0 - t);
    return r;
}

// Is the percentile of mark k exactly the value v, given lt = #(x < v) and le = #(x <= v) over all npix samples?  It is iff both
// order statistics that carry weight are v: #(x < v) <= lo and #(x <= v) >= hi + 1 -- with t == 0 (an integral virtual index)
// the upper one carries none and lo stands in for hi.  Everything else, fractional percentiles included, is a miss.
__device__ inline bool wb_mark_exact(long long npix, int k, unsigned int lt, unsigned int le)
{
    long long lo, hi;
    double t;
    wb_mark_ranks(npix, k, lo, hi, t);
    const long long top = t == 0.0 ? lo : hi;
    return (long long)lt <= lo && (long long)le >= top + 1;
}

// counts[12] of one tile: per channel #(x < v_lo), #(x <= v_lo), #(x < v_hi), #(x <= v_hi)
__device__ inline bool wb_tile_exact(long long npix, const unsigned int *counts)
{
    bool ok = true;
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 2; ++k) ok = ok && wb_mark_exact(npix, k, counts[c * 4 + 2 * k], counts[c * 4 + 2 * k + 1]);
    return ok;
}

// Does the gated kernel serve this tile?  (tile: index inside the launch; the gate's arrays start at the launch's first tile)
__device__ inline bool wb_gate_open(const WbGate &g, long long npix, long long tile)
{
    if (!g.pred) return true;
    const bool predicted = g.pred[tile] != 0u;
    if (g.mode == WB_GATE_REFUSED) return !predicted;
    if (g.mode == WB_GATE_PREDICTED) return predicted;
    return predicted && !wb_tile_exact(npix, g.counts + tile * 12);
}

// One channel's 8-bit table from its two percentiles: thread tid writes entry tid (256 threads)
__device__ inline void wb_fill_table_u8(uint8_t *out, int tid, double p_lo, double p_hi, int rgn_variant)
{
    out[tid] = (uint8_t)wb_level(tid, p_lo, p_hi, rgn_variant);
}

// A statistics record of index k in its opened state (what the fused kernels accumulate into)
__device__ inline void stats_open(StatsAccView *a, int k)
{
    a->sum_fx = 0; a->sumsq_fx = 0; a->count = 0; a->above = 0; a->nans = 0;
    a->min_key = ~0ull; a->max_key = 0ull;
    a->threshold = (k == LARS_NDWI) ? 0.0 : (double)0.2f;        // process-images.py:498-502 (float32 compare)
    a->index_id = (unsigned)k; a->reserved = 0;
    for (int b = 0; b < LARS_HIST_BINS; ++b) a->hist[b] = 0;
}

}  // namespace lars
