// Runtime plumbing of liblars_hip.so: per-thread context, errors, memory,
// streams, events.  (Errors, the ABI version and the host-side fold of statistics records: host_core.cpp.)
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>

#include "common.h"

namespace lars {

static thread_local ThreadCtx g_ctx;

// A thread that used the library gives its stream, workspaces and FFT plan back when it ends (Streamlit sessions
// are threads that come and go).  Thread-local destructors of the main thread run before any atexit handler, so
// the HIP runtime is still alive then.
static void release_ctx(ThreadCtx *c)
{
    if (c->device < 0) return;
    if (hipSetDevice(c->device) != hipSuccess) { c->device = -1; return; }
    align_release();
    if (c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); c->stream = nullptr; }
    if (c->ws) { hipFree(c->ws); c->ws = nullptr; c->ws_bytes = 0; }
    if (c->scratch) { hipFree(c->scratch); c->scratch = nullptr; c->scratch_bytes = 0; }
    if (c->outline) { hipFree(c->outline); c->outline = nullptr; c->outline_bytes = 0; }
    c->u16_win_tiles = 0;
    c->device = -1;
}
struct CtxGuard {
    ~CtxGuard() { release_ctx(&g_ctx); }
};
static thread_local CtxGuard g_ctx_guard;

static int bind_device(ThreadCtx *c, int ordinal)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(LARS_ERR_NO_DEVICE, "no HIP device available (%s); liblars_hip has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (ordinal < 0 || ordinal >= count) return fail(LARS_ERR_INVALID, "device ordinal %d out of range [0,%d)", ordinal, count);
    hipDeviceProp_t prop;
    LARS_HIP_TRY(hipGetDeviceProperties(&prop, ordinal));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(LARS_ERR_NO_DEVICE, "device %d is %s; liblars_hip is built for gfx950 (MI355X) only", ordinal,
                    prop.gcnArchName);
    LARS_HIP_TRY(hipSetDevice(ordinal));
    if (c->stream) { hipStreamDestroy(c->stream); c->stream = nullptr; }
    if (c->ws) { hipFree(c->ws); c->ws = nullptr; c->ws_bytes = 0; }
    if (c->scratch) { hipFree(c->scratch); c->scratch = nullptr; c->scratch_bytes = 0; }
    if (c->outline) { hipFree(c->outline); c->outline = nullptr; c->outline_bytes = 0; }
    c->u16_win_tiles = 0;
    LARS_HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->device = ordinal;
    (void)&g_ctx_guard;                                   // odr-use: constructs this thread's guard
    return LARS_OK;
}

int ensure_ctx(ThreadCtx **out)
{
    ThreadCtx *c = &g_ctx;
    if (c->device < 0) LARS_TRY(bind_device(c, 0));
    else LARS_HIP_TRY(hipSetDevice(c->device));
    *out = c;
    return LARS_OK;
}

static int reserve(void **p, size_t *have, size_t bytes, hipStream_t s)
{
    if (bytes <= *have) return LARS_OK;
    if (*p) {
        LARS_HIP_TRY(hipStreamSynchronize(s));
        LARS_HIP_TRY(hipFree(*p));
        *p = nullptr; *have = 0;
    }
    size_t want = bytes + (bytes >> 3);                  // 12.5 % slack against regrowth
    want = (want + 0xFFFFF) & ~(size_t)0xFFFFF;
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) {
        *p = nullptr;
        return fail(LARS_ERR_OOM, "hipMalloc(%zu) for the library workspace failed: %s", want, hipGetErrorString(e));
    }
    *have = want;
    return LARS_OK;
}
int ws_reserve(ThreadCtx *c, size_t bytes) { return reserve(&c->ws, &c->ws_bytes, bytes, c->stream); }
int scratch_reserve(ThreadCtx *c, size_t bytes)
{
    c->u16_win_tiles = 0;                                 // whoever reserves the scratch writes it: the last pre-pass's report is gone
    return reserve(&c->scratch, &c->scratch_bytes, bytes, c->stream);
}

int outline_reserve(ThreadCtx *c, size_t bytes) { return reserve(&c->outline, &c->outline_bytes, bytes, c->stream); }

static Tuning g_tuning;
Tuning &tuning() { return g_tuning; }

// Every key of lars_set_tuning / lars_get_tuning: a new knob is one field of Tuning (common.h: what it does, its default) and one
// row here (who may write it, which values it takes).  include/lars_hip.h describes the keys for users.
struct Knob {
    const char *name;
    int Tuning::*field;
    enum Access { SET, READ_ONLY, LAB_LAYOUT } access;   // LAB_LAYOUT: set in the laboratory build (make lablayout) only
    bool (*allowed)(int);                                // nullptr: any integer
    const char *domain;                                  // the allowed values as the error message names them
};
#ifdef LARS_LAB_LAYOUT
static const bool kLabLayout = true;
#else
static const bool kLabLayout = false;
#endif
// The READ_ONLY rows are reports: plain ints that a launch from any thread writes, neither per thread nor atomic.
static const Knob KNOBS[] = {
    {"fused_impl", &Tuning::fused_impl, Knob::SET, nullptr, nullptr},
    {"hist_impl", &Tuning::hist_impl, Knob::SET, nullptr, nullptr},
    {"nt_stores", &Tuning::nt_stores, Knob::SET, nullptr, nullptr},
    {"blocks_per_tile", &Tuning::blocks_per_tile, Knob::SET, nullptr, nullptr},
    {"load_policy", &Tuning::load_policy, Knob::SET, [](int v) { return v >= 0 && v <= 2; }, "0 .. 2"},
    {"selq_window", &Tuning::selq_window, Knob::SET, nullptr, nullptr},
    {"selq_list_wgs", &Tuning::selq_list_wgs, Knob::SET, nullptr, nullptr},
    {"joint_depth", &Tuning::joint_depth, Knob::SET, [](int v) { return v == 4 || v == 6 || v == 8 || v == 12; }, "4, 6, 8 or 12"},
    {"joint_window", &Tuning::joint_window, Knob::SET, [](int v) { return v >= 0 && v <= 5; }, "0 .. 5"},
    {"joint_win_depth", &Tuning::joint_win_depth, Knob::SET, [](int v) { return v == 4 || v == 5 || v == 6 || v == 12 || v == 15; }, "4, 5, 6, 12 or 15"},
    {"out_stride_planes", &Tuning::out_stride_planes, Knob::LAB_LAYOUT, nullptr, nullptr},
    {"u16_hist_impl", &Tuning::u16_hist_impl, Knob::SET, [](int v) { return v == 5 || v == 1 || v == 3; }, "5, 1 or 3"},
    {"jpeg_subseq_bits", &Tuning::jpeg_subseq_bits, Knob::SET, [](int v) { return v >= 32 && v <= 65536; }, "32 .. 65536"},
    {"tiff_strip_bytes", &Tuning::tiff_strip_bytes, Knob::SET, [](int v) { return v >= 1 && v <= (1 << 30); }, "1 .. 1073741824"},
    {"deflate_matching", &Tuning::deflate_matching, Knob::SET, [](int v) { return v == 0 || v == 1; }, "0 or 1"},
    {"zone_split_pixels", &Tuning::zone_split_pixels, Knob::SET, [](int v) { return v >= 64 && v <= (1 << 30); }, "64 .. 1073741824"},
    {"wb_predict", &Tuning::wb_predict, Knob::SET, [](int v) { return v >= 0 && v <= 3; }, "0 .. 3"},
    {"wb_predict_sixteenths", &Tuning::wb_predict_sixteenths, Knob::SET, [](int v) { return v >= 2 && v <= 4; }, "2 .. 4"},
    {"wb_predict_k", &Tuning::wb_predict_k, Knob::SET, [](int v) { return v >= 1 && v <= 16; }, "1 .. 16"},
    {"wb_predict_min_pixels", &Tuning::wb_predict_min_pixels, Knob::SET, [](int v) { return v >= 1; }, "1 or more"},
    {"last_fused_kernel", &Tuning::last_fused_kernel, Knob::READ_ONLY, nullptr, nullptr},
    {"jpeg_last_rounds", &Tuning::jpeg_last_rounds, Knob::READ_ONLY, nullptr, nullptr},
};
static const Knob *find_knob(const char *key)
{
    for (const Knob &k : KNOBS)
        if (!strcmp(key, k.name)) return &k;
    return nullptr;
}

int launch_check(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LARS_ERR_HIP, "%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return LARS_OK;
}

}  // namespace lars

using namespace lars;

extern "C" {


int lars_device_count(int *count)
{
    if (!count) return fail(LARS_ERR_INVALID, "lars_device_count: NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(LARS_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return LARS_OK;
}

int lars_set_device(int ordinal) { return bind_device(&g_ctx, ordinal); }

int lars_get_device(int *ordinal)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (ordinal) *ordinal = c->device;
    return LARS_OK;
}

int lars_device_name(char *buf, size_t buflen)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    hipDeviceProp_t prop;
    LARS_HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    snprintf(buf, buflen, "%s (%s, %d CUs, %.1f GiB)", prop.name, prop.gcnArchName, prop.multiProcessorCount,
             (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    return LARS_OK;
}

int lars_malloc(void **dptr, size_t bytes)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!dptr) return fail(LARS_ERR_INVALID, "lars_malloc: NULL");
    const hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) { *dptr = nullptr; return fail(LARS_ERR_OOM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
    return LARS_OK;
}
int lars_free(void *dptr)
{
    if (!dptr) return LARS_OK;
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipFree(dptr));
    return LARS_OK;
}
int lars_memset(void *dptr, int value, size_t bytes, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipMemsetAsync(dptr, value, bytes, pick_stream(c, stream)));
    return LARS_OK;
}
int lars_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    return LARS_OK;
}
int lars_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    return LARS_OK;
}
int lars_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, pick_stream(c, stream)));
    return LARS_OK;
}
int lars_stream_create(void **stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    hipStream_t s;
    LARS_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return LARS_OK;
}
int lars_stream_destroy(void *stream)
{
    if (stream) LARS_HIP_TRY(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
    return LARS_OK;
}
int lars_synchronize(void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipStreamSynchronize(pick_stream(c, stream)));
    return LARS_OK;
}
int lars_shutdown(void)
{
    release_ctx(&g_ctx);
    return LARS_OK;
}

int lars_mem_info(size_t *free_bytes, size_t *total_bytes)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    size_t f = 0, t = 0;
    LARS_HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return LARS_OK;
}

int lars_event_create(void **event)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    hipEvent_t e;
    LARS_HIP_TRY(hipEventCreate(&e));
    *event = e;
    return LARS_OK;
}
int lars_event_destroy(void *event)
{
    if (event) LARS_HIP_TRY(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)));
    return LARS_OK;
}
int lars_event_record(void *event, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    LARS_HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(event), pick_stream(c, stream)));
    return LARS_OK;
}
int lars_stream_wait_event(void *stream, void *event)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!event) return fail(LARS_ERR_INVALID, "lars_stream_wait_event: NULL event");
    LARS_HIP_TRY(hipStreamWaitEvent(pick_stream(c, stream), reinterpret_cast<hipEvent_t>(event), 0));
    return LARS_OK;
}
int lars_event_elapsed_ms(void *start, void *stop, float *ms)
{
    LARS_HIP_TRY(hipEventSynchronize(reinterpret_cast<hipEvent_t>(stop)));
    LARS_HIP_TRY(hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start), reinterpret_cast<hipEvent_t>(stop)));
    return LARS_OK;
}

// Which build-time switches of the kernel sources this library was compiled with: 0 for the product.  A laboratory build
// (csrc/Makefile: lablayout, EXTRA=-D...) answers with the bits of what it changed, so that no measurement or test can mistake it.
unsigned int lars_build_flags(void)
{
    unsigned int f = 0;
#ifdef LARS_LAB_LAYOUT
    f |= LARS_BUILD_LAB_LAYOUT;
#endif
#ifdef LARS_IEEE_DIV
    f |= LARS_BUILD_IEEE_DIV;
#endif
#if LARS_V2_STATS_THREADS != 1024 || LARS_V2_STATS_WAVES != 8
    f |= LARS_BUILD_STATS_GEOMETRY;
#endif
    return f;
}

int lars_set_tuning(const char *key, int value)
{
    if (!key) return fail(LARS_ERR_INVALID, "lars_set_tuning: NULL key");
    const Knob *k = find_knob(key);
    if (!k || k->access == Knob::READ_ONLY) return fail(LARS_ERR_INVALID, "lars_set_tuning: unknown key %s", key);
    if (k->access == Knob::LAB_LAYOUT && !kLabLayout)
        return fail(LARS_ERR_INVALID, "lars_set_tuning: %s exists in the laboratory build only (make lablayout); this library would ignore it", key);
    if (k->allowed && !k->allowed(value)) return fail(LARS_ERR_INVALID, "lars_set_tuning: %s is %s (got %d)", key, k->domain, value);
    tuning().*k->field = value;
    return LARS_OK;
}
int lars_get_tuning(const char *key, int *value)
{
    if (!key || !value) return fail(LARS_ERR_INVALID, "lars_get_tuning: NULL");
    const Knob *k = find_knob(key);
    if (!k) return fail(LARS_ERR_INVALID, "lars_get_tuning: unknown key %s", key);
    *value = tuning().*k->field;
    return LARS_OK;
}

// Exhaustive device self-check of the rcp+fma quotient against IEEE division.
int lars_d_quot_selfcheck(uint32_t max_den, uint64_t *mismatches, uint32_t first_bad[2])
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!mismatches || !first_bad || max_den < 1) return fail(LARS_ERR_INVALID, "lars_d_quot_selfcheck: bad arguments");
    LARS_TRY(scratch_reserve(c, 64));
    unsigned long long *d = static_cast<unsigned long long *>(c->scratch);
    LARS_HIP_TRY(hipMemsetAsync(d, 0, 64, c->stream));
    LARS_TRY(quot_check_launch(max_den, d, reinterpret_cast<unsigned int *>(d + 1), c->stream));
    unsigned long long h[2];
    LARS_HIP_TRY(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, c->stream));
    LARS_HIP_TRY(hipStreamSynchronize(c->stream));
    *mismatches = h[0];
    first_bad[0] = (uint32_t)(h[1] & 0xFFFFFFFFu);
    first_bad[1] = (uint32_t)(h[1] >> 32);
    return LARS_OK;
}

}  // extern "C"
