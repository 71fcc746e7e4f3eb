// Host entry points (lars_h_*): host pointers in, host pointers out.  These are
// what the Python mirror of the reference's functions binds (one call per
// reference function).  Each call stages through the calling
// thread's grow-only device workspace and stream, so concurrent Streamlit
// sessions (threads) do not share mutable state.  The array, colormap, alignment
// and change-detection entry points are here; the picture path (process_image
// and its variants) is host_image.cpp, the zone path (zonal statistics of a
// plane, label_regions, region_outlines, rasterize_zones) host_zones.cpp.
#include <string.h>

#include "common.h"

using namespace lars;

template <typename T>
static int analyze_impl(const T *x, int64_t n, T thr, int want_hist, lars_stats *out, T *median_pair, double *sumsqdev)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || n <= 0 || !out) return fail(LARS_ERR_INVALID, "lars_h_analyze: bad arguments");
    T *dx, *dmed;
    lars_stats *dst;
    double *dss;
    char *dsel;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        dx = d.take<T>(n);
        dst = d.take<lars_stats>(1);
        dmed = d.take<T>(2);
        dss = d.take<double>(1);
        dsel = d.take<char>(lars_select_scratch_bytes());
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * sizeof(T), hipMemcpyHostToDevice, s));
    if (sizeof(T) == 4) {
        LARS_TRY(lars_d_array_stats_f32(reinterpret_cast<const float *>(dx), n, (float)thr, want_hist, dst, s));
        if (median_pair)
            LARS_TRY(lars_d_median_pair_f32(reinterpret_cast<const float *>(dx), n, reinterpret_cast<float *>(dmed), dsel, s));
    } else {
        LARS_TRY(lars_d_array_stats_f64(reinterpret_cast<const double *>(dx), n, (double)thr, want_hist, dst,
                                        sumsqdev ? dss : nullptr, s));
        if (median_pair)
            LARS_TRY(lars_d_median_pair_f64(reinterpret_cast<const double *>(dx), n, reinterpret_cast<double *>(dmed), dsel, s));
    }
    LARS_HIP_TRY(hipMemcpyAsync(out, dst, sizeof(lars_stats), hipMemcpyDeviceToHost, s));
    if (median_pair) LARS_HIP_TRY(hipMemcpyAsync(median_pair, dmed, 2 * sizeof(T), hipMemcpyDeviceToHost, s));
    if (sumsqdev) LARS_HIP_TRY(hipMemcpyAsync(sumsqdev, dss, sizeof(double), hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

extern "C" {

int lars_h_calculate_index_planes(const float *red, const float *green, const float *nir, int64_t n, int index_id,
                                  float *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!red || !green || !nir || !out || n <= 0) return fail(LARS_ERR_INVALID, "lars_h_calculate_index_planes: bad arguments");
    float *dr, *dg, *dn, *dout;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dr = d.take<float>(n), dg = d.take<float>(n), dn = d.take<float>(n), dout = d.take<float>(n); }));
    hipStream_t s = c->stream;
    // only the two bands the index reads cross PCIe
    const float *ha = index_id == LARS_NDWI ? green : nir;
    const float *hb = index_id == LARS_NDVI ? red : (index_id == LARS_GNDVI ? green : nir);
    float *da = index_id == LARS_NDWI ? dg : dn;
    float *db = index_id == LARS_NDVI ? dr : (index_id == LARS_GNDVI ? dg : dn);
    LARS_HIP_TRY(hipMemcpyAsync(da, ha, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(db, hb, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_index_planes_f32(dr, dg, dn, n, index_id, dout, s));
    LARS_HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_ndvi_f64(const void *img, int64_t h, int64_t w, int channels, int dtype, double *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!img || !out || h <= 0 || w <= 0 || channels < 3) return fail(LARS_ERR_INVALID, "lars_h_ndvi_f64: bad arguments");
    if (dtype != LARS_U8 && dtype != LARS_U16) return fail(LARS_ERR_INVALID, "lars_h_ndvi_f64: dtype");
    const size_t npix = (size_t)h * w, esz = dtype == LARS_U8 ? 1 : 2;
    uint8_t *dimg;
    double *dout;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dimg = d.take<uint8_t>(npix * channels * esz), dout = d.take<double>(npix); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dimg, img, npix * channels * esz, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_ndvi_f64(dimg, (int64_t)npix, channels, dtype, dout, s));
    LARS_HIP_TRY(hipMemcpyAsync(out, dout, npix * 8, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_analyze_f32(const float *x, int64_t n, float threshold, int want_hist, lars_stats *out, float median_pair[2])
{
    return analyze_impl<float>(x, n, threshold, want_hist, out, median_pair, nullptr);
}
int lars_h_analyze_f64(const double *x, int64_t n, double threshold, int want_hist, lars_stats *out, double median_pair[2],
                       double *sumsqdev)
{
    return analyze_impl<double>(x, n, threshold, want_hist, out, median_pair, sumsqdev);
}

int lars_h_threshold_mask_f32(const float *x, int64_t n, float threshold, uint8_t *out_mask)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || !out_mask || n <= 0) return fail(LARS_ERR_INVALID, "lars_h_threshold_mask_f32: bad arguments");
    float *dx;
    uint8_t *dm;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dx = d.take<float>(n), dm = d.take<uint8_t>((size_t)n + 4); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_TRY(lars_d_threshold_mask_f32(dx, n, threshold, dm, s));
    LARS_HIP_TRY(hipMemcpyAsync(out_mask, dm, (size_t)n, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

// lars_h_colormap_f32 (range == nullptr) and lars_h_colormap_norm_f32 (range = {vmin, vmax})
static int colormap_impl(const char *who, const float *x, int64_t n, const float *range, const uint8_t *lut_rgba, uint8_t *out_rgba)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!x || !lut_rgba || !out_rgba || n <= 0) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    float *dx;
    uint8_t *dl, *dout;
    LARS_TRY(ws_plan(c, [&](Carver &d) { dx = d.take<float>(n), dl = d.take<uint8_t>(1024), dout = d.take<uint8_t>((size_t)n * 4); }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(dl, lut_rgba, 1024, hipMemcpyHostToDevice, s));
    LARS_TRY(range ? lars_d_colormap_norm_f32(dx, n, range[0], range[1], dl, dout, s) : lars_d_colormap_f32(dx, n, dl, dout, s));
    LARS_HIP_TRY(hipMemcpyAsync(out_rgba, dout, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return LARS_OK;
}

int lars_h_colormap_f32(const float *x, int64_t n, const uint8_t *lut_rgba, uint8_t *out_rgba)
{
    return colormap_impl("lars_h_colormap_f32", x, n, nullptr, lut_rgba, out_rgba);
}

int lars_h_colormap_norm_f32(const float *x, int64_t n, float vmin, float vmax, const uint8_t *lut_rgba, uint8_t *out_rgba)
{
    const float range[2] = {vmin, vmax};
    return colormap_impl("lars_h_colormap_norm_f32", x, n, range, lut_rgba, out_rgba);
}

// device-side registration of `moving` (device, uint8 [h][w][channels]) to `fixed`: estimate + apply
static int align_on_device(ThreadCtx *c, const uint8_t *d_fixed, const uint8_t *d_moving, int64_t h, int64_t w, int channels,
                           double *d_fa, double *d_fb, void *d_scratch, int64_t *d_shift, uint8_t *d_aligned, hipStream_t s)
{
    const int64_t npix = h * w;
    LARS_TRY(lars_d_gray_c128(d_fixed, npix, channels, d_fa, s));
    LARS_TRY(lars_d_gray_c128(d_moving, npix, channels, d_fb, s));
    LARS_TRY(lars_d_phase_correlation(d_fa, d_fb, h, w, d_shift, d_scratch, s));
    LARS_TRY(lars_d_shift_reflect_u8(d_moving, h, w, channels, d_shift, d_aligned, s));
    return LARS_OK;
}

int lars_h_align_images(const uint8_t *fixed, const uint8_t *moving, int64_t h, int64_t w, int channels, uint8_t *out_aligned,
                        double shift[2])
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!fixed || !moving || !out_aligned || h <= 0 || w <= 0 || (channels != 1 && channels != 3))
        return fail(LARS_ERR_INVALID, "lars_h_align_images: two uint8 [h][w][3] (or [h][w]) images of the same shape are required");
    const size_t npix = (size_t)h * w, nbytes = npix * channels;
    uint8_t *df, *dm, *da;
    double *fa, *fb;
    char *sc;
    int64_t *dshift;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        df = d.take<uint8_t>(nbytes), dm = d.take<uint8_t>(nbytes), da = d.take<uint8_t>(nbytes);
        fa = d.take<double>(npix * 2), fb = d.take<double>(npix * 2);
        sc = d.take<char>(lars_phase_scratch_bytes());
        dshift = d.take<int64_t>(2);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(df, fixed, nbytes, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(dm, moving, nbytes, hipMemcpyHostToDevice, s));
    LARS_TRY(align_on_device(c, df, dm, h, w, channels, fa, fb, sc, dshift, da, s));
    int64_t hs[2] = {0, 0};
    LARS_HIP_TRY(hipMemcpyAsync(out_aligned, da, nbytes, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipMemcpyAsync(hs, dshift, sizeof hs, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (shift) { shift[0] = (double)hs[0]; shift[1] = (double)hs[1]; }
    return LARS_OK;
}

int lars_h_change_detection(const uint8_t *early, const uint8_t *late, int64_t h, int64_t w, int channels, int wb_early,
                            int wb_late, int align, int index_id, float *out_early, float *out_late, float *out_diff,
                            uint8_t *out_rgba_diff, const uint8_t *lut_rgba, float vmin, float vmax,
                            uint8_t *out_aligned_late, double shift[2])
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!early || !late || h <= 0 || w <= 0 || channels < 3)
        return fail(LARS_ERR_INVALID, "lars_h_change_detection: two uint8 [h][w][>=3] images of the same shape are required");
    if (index_id < 0 || index_id > 2) return fail(LARS_ERR_INVALID, "lars_h_change_detection: index_id");
    if (align && channels != 3) return fail(LARS_ERR_INVALID, "lars_h_change_detection: registration needs 3-channel images (rgb2gray)");
    if (out_rgba_diff && !lut_rgba) return fail(LARS_ERR_INVALID, "lars_h_change_detection: out_rgba_diff needs lut_rgba");
    const size_t npix = (size_t)h * w, nbytes = npix * channels;
    struct {
        uint8_t *early, *late, *early_wb, *late_wb, *aligned, *table, *rgba, *lut;
        double *pcts, *fa, *fb;
        char *phase;
        int64_t *shift;
        float *idx_early, *idx_late, *diff;
    } B;
    LARS_TRY(ws_plan(c, [&](Carver &d) {
        B.early = d.take<uint8_t>(nbytes), B.late = d.take<uint8_t>(nbytes);
        B.early_wb = d.take<uint8_t>(nbytes), B.late_wb = d.take<uint8_t>(nbytes), B.aligned = d.take<uint8_t>(nbytes);
        B.table = d.take<uint8_t>(lars_wb_table_bytes(LARS_U8));
        B.pcts = d.take<double>(6);
        B.fa = d.take<double>(align ? npix * 2 : 1), B.fb = d.take<double>(align ? npix * 2 : 1);
        B.phase = d.take<char>(lars_phase_scratch_bytes());
        B.shift = d.take<int64_t>(2);
        B.idx_early = d.take<float>(npix), B.idx_late = d.take<float>(npix), B.diff = d.take<float>(npix);
        B.rgba = d.take<uint8_t>(out_rgba_diff ? npix * 4 : 1), B.lut = d.take<uint8_t>(1024);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(B.early, early, nbytes, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemcpyAsync(B.late, late, nbytes, hipMemcpyHostToDevice, s));
    LARS_HIP_TRY(hipMemsetAsync(B.shift, 0, 2 * sizeof(int64_t), s));
    // white balance where the caller holds no cached corrected array (process-images.py:894-902)
    const uint8_t *src[2] = {B.early, B.late};
    uint8_t *wb_out[2] = {B.early_wb, B.late_wb};
    const int want_wb[2] = {wb_early, wb_late};
    for (int k = 0; k < 2; ++k) {
        if (!want_wb[k]) continue;
        LARS_TRY(lars_d_wb_prepare(src[k], 1, (int64_t)npix, channels, LARS_U8, B.table, B.pcts, 0, s));
        lars_fused_args a;
        memset(&a, 0, sizeof a);
        a.tiles = src[k]; a.ntiles = 1; a.npix = (int64_t)npix; a.channels = channels; a.dtype = LARS_U8;
        a.wb_table = B.table; a.out_wb = wb_out[k]; a.stream = s;
        LARS_TRY(lars_d_fused(&a));
        src[k] = wb_out[k];
    }
    // registration of the late image onto the early one (:905-908)
    const uint8_t *late_final = src[1];
    if (align) {
        LARS_TRY(align_on_device(c, src[0], src[1], h, w, channels, B.fa, B.fb, B.phase, B.shift, B.aligned, s));
        late_final = B.aligned;
    }
    // indices (:911-919), difference (:923) and its colour map (:956)
    const uint8_t *imgs[2] = {src[0], late_final};
    float *idx[2] = {B.idx_early, B.idx_late};
    for (int k = 0; k < 2; ++k) {
        lars_fused_args a;
        memset(&a, 0, sizeof a);
        a.tiles = imgs[k]; a.ntiles = 1; a.npix = (int64_t)npix; a.channels = channels; a.dtype = LARS_U8;
        a.index_mask = 1u << index_id; a.out_index[index_id] = idx[k]; a.stream = s;
        LARS_TRY(lars_d_fused(&a));
    }
    LARS_TRY(lars_d_diff_f32(B.idx_early, B.idx_late, (int64_t)npix, B.diff, s));
    if (out_rgba_diff) {
        LARS_HIP_TRY(hipMemcpyAsync(B.lut, lut_rgba, 1024, hipMemcpyHostToDevice, s));
        LARS_TRY(lars_d_colormap_norm_f32(B.diff, (int64_t)npix, vmin, vmax, B.lut, B.rgba, s));
        LARS_HIP_TRY(hipMemcpyAsync(out_rgba_diff, B.rgba, npix * 4, hipMemcpyDeviceToHost, s));
    }
    int64_t hs[2] = {0, 0};
    if (out_early) LARS_HIP_TRY(hipMemcpyAsync(out_early, B.idx_early, npix * 4, hipMemcpyDeviceToHost, s));
    if (out_late) LARS_HIP_TRY(hipMemcpyAsync(out_late, B.idx_late, npix * 4, hipMemcpyDeviceToHost, s));
    if (out_diff) LARS_HIP_TRY(hipMemcpyAsync(out_diff, B.diff, npix * 4, hipMemcpyDeviceToHost, s));
    if (out_aligned_late) LARS_HIP_TRY(hipMemcpyAsync(out_aligned_late, late_final, nbytes, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipMemcpyAsync(hs, B.shift, sizeof hs, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (shift) { shift[0] = (double)hs[0]; shift[1] = (double)hs[1]; }
    return LARS_OK;
}

}  // extern "C"
