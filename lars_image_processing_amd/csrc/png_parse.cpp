// Host side of the PNG decoder: the chunk layout of a PNG file, validated without a device (lars_png_info).  Only chunk
// headers are read, plus the CRC of every chunk that is not IDAT (IDAT CRCs are checked on the device, where the payloads
// are gathered).  No HIP here: builds into liblars_hip.so and with plain g++ under AddressSanitizer / UBSan (`make asan`).
#include <string.h>

#include "host_common.h"

namespace {

uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

uint32_t crc32_bytes(uint32_t crc, const uint8_t *p, size_t n)
{
    struct Table {
        uint32_t t[256];
        Table() {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
                t[i] = c;
            }
        }
    };
    static const Table table;         // initialised once, thread-safe
    const uint32_t *tab = table.t;
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = tab[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return ~crc;
}

bool is_cid(const uint8_t *t)
{
    for (int i = 0; i < 4; ++i)
        if (!((t[i] >= 'A' && t[i] <= 'Z') || (t[i] >= 'a' && t[i] <= 'z'))) return false;
    return true;
}

}  // namespace

using namespace lars;

extern "C" int lars_png_info(const uint8_t *file, int64_t len, int64_t info[LARS_PNG_INFO_N], int64_t *idat_table, int64_t idat_cap)
{
    if (!file || len < 0 || !info || idat_cap < 0 || (idat_cap > 0 && !idat_table))
        return fail(LARS_ERR_INVALID, "lars_png_info: bad arguments");
    memset(info, 0, sizeof(int64_t) * LARS_PNG_INFO_N);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    if (len < 8 || memcmp(file, sig, 8) != 0) return fail(LARS_ERR_INVALID, "png: bad signature (not a PNG file)");
    int64_t pos = 8, nidat = 0, idat_bytes = 0;
    int state = 0;                    // 0 before IDAT, 1 in the IDAT run, 2 after it
    bool ihdr = false, iend = false, apng = false;
    while (pos < len) {
        if (len - pos < 12) return fail(LARS_ERR_INVALID, "png: chunk header at byte %lld runs past the end of the file", (long long)pos);
        const uint32_t n = be32(file + pos);
        const uint8_t *type = file + pos + 4;
        if (n > 0x7FFFFFFFu) return fail(LARS_ERR_INVALID, "png: chunk length %u at byte %lld", n, (long long)pos);
        if (!is_cid(type)) return fail(LARS_ERR_INVALID, "png: broken chunk type at byte %lld", (long long)pos);
        if ((int64_t)n > len - pos - 12)
            return fail(LARS_ERR_INVALID, "png: chunk %.4s at byte %lld runs past the end of the file (%u bytes)", (const char *)type,
                        (long long)pos, n);
        const uint8_t *data = file + pos + 8;
        const bool is_idat = memcmp(type, "IDAT", 4) == 0;
        if (!ihdr && memcmp(type, "IHDR", 4) != 0) return fail(LARS_ERR_INVALID, "png: missing IHDR (first chunk is %.4s)", (const char *)type);
        if (!is_idat && crc32_bytes(crc32_bytes(0, type, 4), data, n) != be32(data + n))
            return fail(LARS_ERR_INVALID, "png: bad CRC in chunk %.4s at byte %lld", (const char *)type, (long long)pos);
        if (memcmp(type, "IHDR", 4) == 0) {
            if (ihdr) return fail(LARS_ERR_INVALID, "png: misplaced IHDR at byte %lld (second IHDR)", (long long)pos);
            if (n != 13) return fail(LARS_ERR_INVALID, "png: IHDR of %u bytes (13 expected)", n);
            ihdr = true;
            const int64_t w = be32(data), h = be32(data + 4);
            info[LARS_PNG_INFO_WIDTH] = w;
            info[LARS_PNG_INFO_HEIGHT] = h;
            info[LARS_PNG_INFO_BIT_DEPTH] = data[8];
            info[LARS_PNG_INFO_COLOR_TYPE] = data[9];
            info[LARS_PNG_INFO_INTERLACE] = data[12];
            if (w == 0 || h == 0 || w > 0x7FFFFFFF || h > 0x7FFFFFFF)
                return fail(LARS_ERR_INVALID, "png: IHDR size %lld x %lld", (long long)w, (long long)h);
            const int d = data[8], ct = data[9];
            const bool ok = (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
                            ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
            if (!ok) return fail(LARS_ERR_INVALID, "png: IHDR bit depth %d with colour type %d", d, ct);
            if (data[10] != 0 || data[11] != 0 || data[12] > 1)
                return fail(LARS_ERR_INVALID, "png: IHDR compression %d, filter %d, interlace %d", data[10], data[11], data[12]);
        } else if (is_idat) {
            if (state == 2) return fail(LARS_ERR_INVALID, "png: misplaced IDAT at byte %lld (IDAT chunks are not consecutive)", (long long)pos);
            state = 1;
            if (nidat < idat_cap) {
                idat_table[2 * nidat] = pos + 8;
                idat_table[2 * nidat + 1] = n;
            }
            ++nidat;
            idat_bytes += n;
        } else {
            if (state == 1) state = 2;
            if (memcmp(type, "acTL", 4) == 0 || memcmp(type, "fcTL", 4) == 0 || memcmp(type, "fdAT", 4) == 0) apng = true;
            if (memcmp(type, "IEND", 4) == 0) {
                iend = true;
                pos += 12 + (int64_t)n;
                break;
            }
        }
        pos += 12 + (int64_t)n;
    }
    if (!ihdr) return fail(LARS_ERR_INVALID, "png: missing IHDR (file ends after the signature)");
    if (!nidat) return fail(LARS_ERR_INVALID, "png: missing IDAT");
    if (!iend) return fail(LARS_ERR_INVALID, "png: missing IEND (file truncated)");
    static const int chans[7] = {1, 0, 3, 1, 2, 0, 4};
    info[LARS_PNG_INFO_CHANNELS] = chans[info[LARS_PNG_INFO_COLOR_TYPE]];
    info[LARS_PNG_INFO_IDAT_BYTES] = idat_bytes;
    info[LARS_PNG_INFO_IDAT_COUNT] = nidat;
    info[LARS_PNG_INFO_APNG] = apng;
    info[LARS_PNG_INFO_SUPPORTED] = info[LARS_PNG_INFO_BIT_DEPTH] == 8 && info[LARS_PNG_INFO_INTERLACE] == 0 && !apng;
    return LARS_OK;
}

// ---- the layout of the filtered stream and of the decoded array (extended decoder) ------------------------------------
namespace {

bool ihdr_pair_ok(int d, int ct)
{
    return (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
           ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
}

int file_channels(int ct)
{
    static const int chans[7] = {1, 0, 3, 1, 2, 0, 4};
    return chans[ct];
}

}  // namespace

extern "C" int lars_png_out_format(int depth, int color_type, int *channels, int *itemsize)
{
    if (!channels || !itemsize) return fail(LARS_ERR_INVALID, "lars_png_out_format: bad arguments");
    if (color_type < 0 || color_type > 6 || !ihdr_pair_ok(depth, color_type))
        return fail(LARS_ERR_INVALID, "png: bit depth %d with colour type %d", depth, color_type);
    // Pillow: 16-bit gray stays 16 bits (I;16); 16-bit LA opens as RGBA (L, L, L, A); every other 16-bit sample gives its high
    // byte; 1 / 2 / 4-bit samples fill a byte each
    *itemsize = (color_type == 0 && depth == 16) ? 2 : 1;
    *channels = (color_type == 4 && depth == 16) ? 4 : file_channels(color_type);
    return LARS_OK;
}

extern "C" int lars_png_layout(int64_t w, int64_t h, int depth, int color_type, int interlace, int64_t passes[7 * LARS_PNGX_PASS_N],
                               int64_t *npass, int64_t *need)
{
    if (!passes || !npass || !need) return fail(LARS_ERR_INVALID, "lars_png_layout: bad arguments");
    *npass = 0;
    *need = 0;
    if (w < 1 || h < 1 || w > 0x7FFFFFFF || h > 0x7FFFFFFF || interlace < 0 || interlace > 1)
        return fail(LARS_ERR_INVALID, "png: size %lld x %lld, interlace %d", (long long)w, (long long)h, interlace);
    if (color_type < 0 || color_type > 6 || !ihdr_pair_ok(depth, color_type))
        return fail(LARS_ERR_INVALID, "png: bit depth %d with colour type %d", depth, color_type);
    static const int ax0[7] = {0, 4, 0, 2, 0, 1, 0}, ay0[7] = {0, 0, 4, 0, 2, 0, 1};
    static const int adx[7] = {8, 8, 4, 4, 2, 2, 1}, ady[7] = {8, 8, 8, 4, 4, 2, 2};
    const int64_t bits = (int64_t)file_channels(color_type) * depth;     // 1 .. 64 per pixel
    const int64_t bpp = bits < 8 ? 1 : bits / 8;
    int64_t n = 0, total = 0;
    for (int p = 0; p < (interlace ? 7 : 1); ++p) {
        const int64_t x0 = interlace ? ax0[p] : 0, y0 = interlace ? ay0[p] : 0, dx = interlace ? adx[p] : 1, dy = interlace ? ady[p] : 1;
        const int64_t pw = (w - x0 + dx - 1) / dx, ph = (h - y0 + dy - 1) / dy;
        if (pw <= 0 || ph <= 0) continue;                                // an empty pass: no bytes at all
        const int64_t rb = (pw * bits + 7) / 8;                          // < 2^34
        int64_t *q = passes + n * LARS_PNGX_PASS_N;
        q[LARS_PNGX_PASS_X0] = x0; q[LARS_PNGX_PASS_Y0] = y0; q[LARS_PNGX_PASS_DX] = dx; q[LARS_PNGX_PASS_DY] = dy;
        q[LARS_PNGX_PASS_W] = pw; q[LARS_PNGX_PASS_H] = ph; q[LARS_PNGX_PASS_ROW_BYTES] = rb; q[LARS_PNGX_PASS_OFFSET] = total;
        q[LARS_PNGX_PASS_BPP] = bpp; q[LARS_PNGX_PASS_INDEX] = interlace ? p + 1 : 0;
        // ph * (rb + 1) can reach 2^31 * 2^35: saturate, never wrap
        total = (rb + 1 > INT64_MAX / ph || ph * (rb + 1) > INT64_MAX - total) ? INT64_MAX : total + ph * (rb + 1);
        ++n;
    }
    *npass = n;
    *need = total;
    return LARS_OK;
}
