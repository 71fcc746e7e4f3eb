// Host steps that the file codecs share (png.hip, jpeg_encode.hip, png_decode.hip, jpeg_decode.hip, tiff_decode.hip) and the thumbnail
// steps they hand decoded pixels to (resize.hip).  Every workspace here is planned once (common.h: Carver, ws_plan).
#pragma once
#include <vector>

#include "common.h"

namespace lars {

// ---- thumbnails (resize.hip) -------------------------------------------------
// lars_h_thumbnail_u8 in three steps, so that a decoder's entry point puts its own buffers and the thumbnail's into one
// workspace: the checked arguments with the resampling coefficients of both axes, the device buffers, the kernels.
struct ThumbJob {
    int64_t h, w, new_h, new_w;
    int channels, fx, fy, rb[4], rw, rh;          // rw x rh: the reduced image
    bool reduce, need_h, need_v, vertical_first;
    int ksh, ksv;
    std::vector<int> bh, kh, bv, kv;
};
struct ThumbBufs {
    uint8_t *in, *pre, *red, *tmp, *out;
    int *bh, *kh, *bv, *kv;
};
int thumbnail_prepare(int64_t h, int64_t w, int channels, int fx, int fy, const int reduce_box[4], const float box[4], int64_t new_h,
                      int64_t new_w, int vertical_first, ThumbJob *T);
ThumbBufs thumbnail_bufs(const ThumbJob &T, bool on_device, Carver &cv);
// img: a host image (uploaded to B.in) or, with on_device, a device image read in place; out: the host thumbnail
int thumbnail_run(ThreadCtx *c, const ThumbJob &T, const ThumbBufs &B, const uint8_t *img, bool on_device, uint8_t *out);

// ---- encoders ----------------------------------------------------------------
// Host picture in, file out: one upload, encode(d_in, d_out, d_len, d_scratch, d_extra, stream) on the device (d_extra:
// extra_bytes for the codec's own uploads), then the file's length (one small read) and its bytes.
template <typename Encode>
int encode_to_host(ThreadCtx *c, const char *who, const uint8_t *img, size_t in_bytes, size_t bound, size_t scratch_bytes,
                   size_t extra_bytes, uint8_t *out, size_t out_cap, int64_t *out_len, Encode &&encode)
{
    uint8_t *d_in, *d_out, *d_extra;
    char *d_scr;
    int64_t *d_len;
    LARS_TRY(ws_plan(c, [&](Carver &cv) {
        d_in = cv.take<uint8_t>(in_bytes);
        d_out = cv.take<uint8_t>(bound);
        d_scr = cv.take<char>(scratch_bytes);
        d_extra = cv.take<uint8_t>(extra_bytes);
        d_len = cv.take<int64_t>(1);
    }));
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(d_in, img, in_bytes, hipMemcpyHostToDevice, s));
    LARS_TRY(encode(d_in, d_out, d_len, d_scr, d_extra, s));
    int64_t n = 0;
    LARS_HIP_TRY(hipMemcpyAsync(&n, d_len, sizeof n, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    if (n <= 0) return fail(LARS_ERR_HIP, "%s: the device did not finish the file", who);
    if ((size_t)n > out_cap) return fail(LARS_ERR_INVALID, "%s: the file needs %lld bytes, out_cap is %zu", who, (long long)n, out_cap);
    LARS_HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    *out_len = n;
    return LARS_OK;
}

// ---- decoders ----------------------------------------------------------------
// A parsed file on the host and its buffers in the workspace.  A codec derives from it and adds what differs from codec
// to codec:
//   int enqueue(hipStream_t s)           its own uploads into d_extra, lars_d_decode_*_u8, its own read-backs
//   int finish(const int status[2])      after the sync: the message of a status, what it read back
struct HostFile {
    const char *who;
    const uint8_t *file;
    int64_t len, h, w;
    int channels;
    int sample_bytes = 1;          // 2, 4: a 16-bit or float32 picture (tiff_decode.hip), which travels as bytes
    size_t extra_bytes, scratch_bytes;
    uint8_t *d_file, *d_img;
    void *d_extra;
    int32_t *d_status;
    char *d_scratch;
    size_t img_bytes() const { return (size_t)h * w * channels * sample_bytes; }
    void carve(Carver &cv)
    {
        d_file = cv.take<uint8_t>((size_t)len);
        d_extra = cv.take<char>(extra_bytes);
        d_img = cv.take<uint8_t>(img_bytes());
        d_status = cv.take<int32_t>(2);
        d_scratch = cv.take<char>(scratch_bytes);
    }
};

// file on the host -> the decoded image on the device (F.d_img), status checked: one upload, one sync
template <typename Codec>
int decode_on_device(ThreadCtx *c, Codec &F)
{
    hipStream_t s = c->stream;
    LARS_HIP_TRY(hipMemcpyAsync(F.d_file, F.file, (size_t)F.len, hipMemcpyHostToDevice, s));
    LARS_TRY(F.enqueue(s));
    int st[2] = {0, 0};
    LARS_HIP_TRY(hipMemcpyAsync(st, F.d_status, sizeof st, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    return F.finish(st);
}

// ... then one download: host file in, host pixels out
template <typename Codec>
int decode_file_to_host(ThreadCtx *c, Codec &F, uint8_t *out, size_t out_cap)
{
    if (out_cap < F.img_bytes()) return fail(LARS_ERR_INVALID, "%s: out_cap %zu < %zu", F.who, out_cap, F.img_bytes());
    LARS_TRY(ws_plan(c, [&](Carver &cv) { F.carve(cv); }));
    LARS_TRY(decode_on_device(c, F));
    LARS_HIP_TRY(hipMemcpyAsync(out, F.d_img, F.img_bytes(), hipMemcpyDeviceToHost, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    return LARS_OK;
}

// ... or the decoded pixels go straight into the thumbnail kernels: host file in, thumbnail out
template <typename Codec>
int thumbnail_file(ThreadCtx *c, Codec &F, int fx, int fy, const int reduce_box[4], const float box[4], int64_t new_h, int64_t new_w,
                   int vertical_first, uint8_t *out)
{
    ThumbJob T;
    LARS_TRY(thumbnail_prepare(F.h, F.w, F.channels, fx, fy, reduce_box, box, new_h, new_w, vertical_first, &T));
    ThumbBufs U;
    LARS_TRY(ws_plan(c, [&](Carver &cv) { F.carve(cv), U = thumbnail_bufs(T, true, cv); }));
    LARS_TRY(decode_on_device(c, F));
    return thumbnail_run(c, T, U, F.d_img, true, out);
}

}  // namespace lars
