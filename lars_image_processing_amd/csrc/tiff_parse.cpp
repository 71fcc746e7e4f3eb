// Host side of the TIFF decoder: the first directory of a classic TIFF file, validated without a device (lars_tiff_info, and
// lars_tiff_info_deflate for callers who opt in to Deflate on the device: the same walk with compression 8 / 32946 let through).
// A C++ restatement of the directory walk in tiffio.read_tiff, with the same rules in the same order, so that a file the
// Python reader refuses is refused here for the same cause.  Samples are unsigned integers of 8 or 16 bits or float32 (32 bits
// with SampleFormat 3; info's bits == 32 says so), the latter also with the floating-point predictor.  Every offset and count is checked against the file length in
// 64-bit arithmetic before it is used.  No HIP here: builds into liblars_hip.so and with plain g++ under AddressSanitizer /
// UBSan (`make asan`).
#include <string.h>

#include "host_common.h"

namespace {

struct Field {                        // one directory entry this reader can read (types 1, 3, 4, 6, 8, 9)
    bool present = false;
    int type = 0;
    int64_t n = 0, where = 0;
};

struct Dir {
    const uint8_t *file;
    int64_t len;
    bool big;
    uint32_t u16(int64_t at) const { return big ? (uint32_t)file[at] << 8 | file[at + 1] : (uint32_t)file[at + 1] << 8 | file[at]; }
    uint32_t u32(int64_t at) const
    {
        return big ? (uint32_t)file[at] << 24 | (uint32_t)file[at + 1] << 16 | (uint32_t)file[at + 2] << 8 | file[at + 3]
                   : (uint32_t)file[at + 3] << 24 | (uint32_t)file[at + 2] << 16 | (uint32_t)file[at + 1] << 8 | file[at];
    }
    // value k of a field (k < f.n; the field's bytes were checked to lie inside the file)
    int64_t value(const Field &f, int64_t k) const
    {
        switch (f.type) {
        case 1: return file[f.where + k];
        case 6: return (int8_t)file[f.where + k];
        case 3: return u16(f.where + 2 * k);
        case 8: return (int16_t)u16(f.where + 2 * k);
        case 4: return u32(f.where + 4 * k);
        default: return (int32_t)u32(f.where + 4 * k);
        }
    }
};

enum { T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_STRIP_OFFSETS, T_SPP, T_ROWS_PER_STRIP, T_STRIP_COUNTS, T_PLANAR,
       T_PREDICTOR, T_TILE_WIDTH, T_TILE_LENGTH, T_TILE_OFFSETS, T_TILE_COUNTS, T_EXTRA, T_FORMAT, T_N };
const int TAGS[T_N] = {256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 338, 339};

}  // namespace

using namespace lars;

namespace {

// the walk behind lars_tiff_info and lars_tiff_info_deflate; deflate: compression 8 / 32946 goes the way LZW goes
int tiff_walk(const uint8_t *file, int64_t len, int64_t info[LARS_TIFF_INFO_N], int64_t *chunk_table, int64_t table_cap, bool deflate)
{
    if (!file || len < 0 || !info || table_cap < 0 || (table_cap > 0 && !chunk_table))
        return fail(LARS_ERR_INVALID, "lars_tiff_info: bad arguments");
    memset(info, 0, sizeof(int64_t) * LARS_TIFF_INFO_N);
    if (len < 2 || !((file[0] == 'I' && file[1] == 'I') || (file[0] == 'M' && file[1] == 'M')))
        return fail(LARS_ERR_INVALID, "tiff: not a TIFF file (byte-order mark)");
    Dir d{file, len, file[0] == 'M'};
    info[LARS_TIFF_INFO_BIG_ENDIAN] = d.big;
    if (len < 8) return fail(LARS_ERR_INVALID, "tiff: file shorter than a TIFF header");
    const uint32_t magic = d.u16(2);
    auto unsupported = [&](int reason) { info[LARS_TIFF_INFO_SUPPORTED] = 0; info[LARS_TIFF_INFO_REASON] = reason; return LARS_OK; };
    if (magic == 43) return unsupported(LARS_TIFF_REASON_BIGTIFF);
    if (magic != 42) return fail(LARS_ERR_INVALID, "tiff: bad TIFF magic %u", magic);
    const int64_t first = d.u32(4);
    if (first + 2 > len) return fail(LARS_ERR_INVALID, "tiff: first directory lies outside the file");
    const int64_t count = d.u16(first);
    Field tag[T_N];
    static const int sizes[13] = {0, 1, 1, 2, 4, 8, 1, 1, 2, 4, 8, 4, 8};
    for (int64_t i = 0; i < count; ++i) {
        const int64_t at = first + 2 + 12 * i;
        if (at + 12 > len) return fail(LARS_ERR_INVALID, "tiff: directory entry outside the file");
        const int id = (int)d.u16(at), type = (int)d.u16(at + 2);
        const int64_t n = d.u32(at + 4);
        if (type < 1 || type > 12) continue;                 // unknown field type: the TIFF spec says skip it
        const int64_t nbytes = sizes[type] * n;
        const int64_t where = nbytes <= 4 ? at + 8 : (int64_t)d.u32(at + 8);
        if (where + nbytes > len) return fail(LARS_ERR_INVALID, "tiff: value of tag %d lies outside the file", id);
        if (!(type == 1 || type == 3 || type == 4 || type == 6 || type == 8 || type == 9)) continue;   // rationals, floats, ascii
        for (int t = 0; t < T_N; ++t)
            if (TAGS[t] == id) tag[t] = Field{true, type, n, where};                                   // a repeated tag: the last one holds
    }
    bool missing = false;
    int missing_tag = 0;
    auto one = [&](int t, int64_t fallback, bool required) -> int64_t {
        if (!tag[t].present || tag[t].n == 0) {
            if (required && !missing) { missing = true; missing_tag = TAGS[t]; }
            return fallback;
        }
        return d.value(tag[t], 0);
    };
    const int64_t width = one(T_WIDTH, 0, true), height = one(T_LENGTH, 0, true);
    if (missing) return fail(LARS_ERR_INVALID, "tiff: required tag %d is missing", missing_tag);
    const int64_t spp = one(T_SPP, 1, false);
    info[LARS_TIFF_INFO_WIDTH] = width;
    info[LARS_TIFF_INFO_HEIGHT] = height;
    info[LARS_TIFF_INFO_SAMPLES] = spp;
    info[LARS_TIFF_INFO_PHOTOMETRIC] = one(T_PHOTOMETRIC, -1, false);
    info[LARS_TIFF_INFO_EXTRA_SAMPLES] = tag[T_EXTRA].present ? tag[T_EXTRA].n : 0;
    // BitsPerSample: one value, or one per sample, all equal
    int64_t bits = 1;
    if (tag[T_BITS].present && tag[T_BITS].n > 0) {
        const Field &b = tag[T_BITS];
        bits = d.value(b, 0);
        bool same = true;
        for (int64_t k = 1; k < b.n && same; ++k) same = d.value(b, k) == bits;
        if (!same || (b.n != 1 && b.n != spp)) { info[LARS_TIFF_INFO_BITS] = bits; return unsupported(LARS_TIFF_REASON_BITS); }
    }
    info[LARS_TIFF_INFO_BITS] = bits;
    if (bits != 8 && bits != 16 && bits != 32) return unsupported(LARS_TIFF_REASON_BITS);
    // 8 and 16 bits: unsigned integers (the default); 32 bits: IEEE floats, which the tag has to say for every value it holds
    const int64_t format = bits == 32 ? 3 : 1;
    if (bits == 32 && (!tag[T_FORMAT].present || tag[T_FORMAT].n == 0)) return unsupported(LARS_TIFF_REASON_SAMPLE_FORMAT);
    if (tag[T_FORMAT].present)
        for (int64_t k = 0; k < tag[T_FORMAT].n; ++k)
            if (d.value(tag[T_FORMAT], k) != format) return unsupported(LARS_TIFF_REASON_SAMPLE_FORMAT);
    const int64_t compression = one(T_COMPRESSION, 1, false);
    info[LARS_TIFF_INFO_COMPRESSION] = compression;
    const bool inflated = deflate && (compression == 8 || compression == 32946);
    if (compression != 1 && compression != 5 && !inflated) {
        switch (compression) {
        case 8: case 32946: return unsupported(LARS_TIFF_REASON_DEFLATE);
        case 32773: return unsupported(LARS_TIFF_REASON_PACKBITS);
        case 6: case 7: return unsupported(LARS_TIFF_REASON_JPEG);
        case 2: case 3: case 4: return unsupported(LARS_TIFF_REASON_CCITT);
        default: return unsupported(LARS_TIFF_REASON_COMPRESSION);
        }
    }
    const int64_t predictor = one(T_PREDICTOR, 1, false);
    info[LARS_TIFF_INFO_PREDICTOR] = predictor;
    // the floating-point predictor goes with float samples only
    if (predictor != 1 && predictor != 2 && !(predictor == 3 && bits == 32)) return unsupported(LARS_TIFF_REASON_PREDICTOR);
    const int64_t planar = one(T_PLANAR, 1, false);
    info[LARS_TIFF_INFO_PLANAR] = planar;
    if (planar != 1 && planar != 2) return fail(LARS_ERR_INVALID, "tiff: planar configuration %lld", (long long)planar);
    if (width <= 0 || height <= 0 || spp <= 0) return fail(LARS_ERR_INVALID, "tiff: empty image");
    const int64_t bps = bits / 8;
    const int64_t limit = (int64_t)1 << 31;
    // width, height < 2^32 and spp < 2^32 here, so the product is formed step by step
    if (width >= limit || height >= limit || spp >= limit || width * height >= limit || width * height * spp >= limit ||
        width * height * spp * bps >= limit)
        return unsupported(LARS_TIFF_REASON_SIZE);
    const int64_t planes = planar == 2 ? spp : 1, inner = planar == 2 ? 1 : spp;
    int64_t across, down, chunk_w, chunk_h;
    int t_off, t_cnt;
    const bool tiled = tag[T_TILE_WIDTH].present;
    if (tiled) {
        const int64_t tw = one(T_TILE_WIDTH, 0, true), th = one(T_TILE_LENGTH, 0, true);
        if (missing) return fail(LARS_ERR_INVALID, "tiff: required tag %d is missing", missing_tag);
        if (tw <= 0 || th <= 0) return fail(LARS_ERR_INVALID, "tiff: bad tile size %lld x %lld", (long long)tw, (long long)th);
        if (tw >= limit || th >= limit || tw * th >= limit || tw * th * spp * bps >= limit) return unsupported(LARS_TIFF_REASON_SIZE);
        across = (width + tw - 1) / tw, down = (height + th - 1) / th;
        chunk_w = tw, chunk_h = th;
        t_off = T_TILE_OFFSETS, t_cnt = T_TILE_COUNTS;
    } else {
        int64_t rps = one(T_ROWS_PER_STRIP, height, false);
        if (rps > height) rps = height;
        if (rps <= 0) return fail(LARS_ERR_INVALID, "tiff: rows per strip must be positive");
        across = 1, down = (height + rps - 1) / rps;
        chunk_w = width, chunk_h = rps;
        t_off = T_STRIP_OFFSETS, t_cnt = T_STRIP_COUNTS;
    }
    info[LARS_TIFF_INFO_TILED] = tiled;
    info[LARS_TIFF_INFO_CHUNK_W] = chunk_w;
    info[LARS_TIFF_INFO_CHUNK_H] = chunk_h;
    if (!tag[t_off].present) return fail(LARS_ERR_INVALID, "tiff: no strip / tile offsets");
    const int64_t nchunks = tag[t_off].n;
    const bool counted = tag[t_cnt].present;
    if (!counted && (compression != 1 || nchunks != 1)) return fail(LARS_ERR_INVALID, "tiff: strip / tile byte counts are missing");
    if (nchunks != across * down * planes || (counted && tag[t_cnt].n != nchunks))
        return fail(LARS_ERR_INVALID, "tiff: %lld strips / tiles, %lld expected", (long long)nchunks, (long long)(across * down * planes));
    info[LARS_TIFF_INFO_CHUNKS] = nchunks;
    const int64_t full = chunk_h * chunk_w * inner * bps;               // bytes of a whole strip / tile (< 2^31, see above)
    if ((compression == 5 || inflated) && full * nchunks >= limit) return unsupported(LARS_TIFF_REASON_SIZE);   // the padded chunks, decoded
    bool old_lzw = false;
    for (int64_t k = 0; k < nchunks; ++k) {
        const int64_t off = d.value(tag[t_off], k);
        const int64_t cnt = counted ? d.value(tag[t_cnt], k) : width * height * inner * bps;
        if (off < 0 || cnt < 0 || off > len || cnt > len - off) return fail(LARS_ERR_INVALID, "tiff: strip / tile data outside the file");
        const int64_t row = (k / across) % down;
        const int64_t stored_rows = tiled ? chunk_h : (chunk_h < height - row * chunk_h ? chunk_h : height - row * chunk_h);
        const int64_t want = stored_rows * chunk_w * inner * bps;
        if (compression == 1 && cnt < want)
            return fail(LARS_ERR_INVALID, "tiff: strip / tile holds %lld bytes, %lld expected", (long long)cnt, (long long)want);
        // what lars_h_tiff_lzw_decode refuses: a stream of the old bit order (LSB first) starts with 00 and an odd byte
        if (compression == 5 && cnt >= 2 && file[off] == 0 && (file[off + 1] & 1)) old_lzw = true;
        if (k < table_cap) {
            chunk_table[2 * k] = off;
            chunk_table[2 * k + 1] = cnt;
        }
    }
    if (old_lzw) return unsupported(LARS_TIFF_REASON_OLD_LZW);
    info[LARS_TIFF_INFO_SUPPORTED] = 1;
    return LARS_OK;
}

}  // namespace

extern "C" int lars_tiff_info(const uint8_t *file, int64_t len, int64_t info[LARS_TIFF_INFO_N], int64_t *chunk_table, int64_t table_cap)
{
    return tiff_walk(file, len, info, chunk_table, table_cap, false);
}

extern "C" int lars_tiff_info_deflate(const uint8_t *file, int64_t len, int64_t info[LARS_TIFF_INFO_N], int64_t *chunk_table,
                                      int64_t table_cap)
{
    return tiff_walk(file, len, info, chunk_table, table_cap, true);
}
