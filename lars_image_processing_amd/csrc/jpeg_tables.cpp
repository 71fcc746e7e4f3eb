// Host side of the JPEG encoder: everything of the file that does not depend on the pixels.  Pure C++ (the `make asan`
// build covers it): the standard tables of the JPEG standard's annex K as Pillow / libjpeg write them by default, the
// scaling of the quantisation tables by a quality, the header bytes up to and including SOS, and the bound on the file.
#include <string.h>

#include "host_common.h"
#include "jpeg_tables.h"

namespace lars {

// Annex K.1 (natural order) and K.3, read out of a file Pillow wrote at quality 50 (where the scale factor is 100 %)
static const uint8_t JE_QBASE_LUMA[64] = {
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99,
};
static const uint8_t JE_QBASE_CHROMA[64] = {
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
};
static const uint8_t JE_DC_LUMA_BITS[16] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
};
static const uint8_t JE_DC_LUMA_VALS[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
static const uint8_t JE_AC_LUMA_BITS[16] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
};
static const uint8_t JE_AC_LUMA_VALS[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7,
    34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
    36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40,
    41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
    74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105,
    106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137,
    138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
    168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
    198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
    227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
    249, 250,
};
static const uint8_t JE_DC_CHROMA_BITS[16] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
};
static const uint8_t JE_DC_CHROMA_VALS[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
static const uint8_t JE_AC_CHROMA_BITS[16] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
};
static const uint8_t JE_AC_CHROMA_VALS[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113,
    19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
    21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38,
    39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
    73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104,
    105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
    136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165,
    166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
    196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
    226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248,
    249, 250,
};

const uint8_t JE_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffSpec { const uint8_t *bits, *vals; int nvals; };
static const HuffSpec JE_DC[2] = {{JE_DC_LUMA_BITS, JE_DC_LUMA_VALS, 12}, {JE_DC_CHROMA_BITS, JE_DC_CHROMA_VALS, 12}};
static const HuffSpec JE_AC[2] = {{JE_AC_LUMA_BITS, JE_AC_LUMA_VALS, 162}, {JE_AC_CHROMA_BITS, JE_AC_CHROMA_VALS, 162}};

bool jpeg_enc_geometry(int64_t h, int64_t w, int channels, int subsampling, JpegEncGeo *g)
{
    if (h < 1 || w < 1 || h > 65500 || w > 65500 || (channels != 1 && channels != 3)) return false;
    if (subsampling < 0 || subsampling > 2) return false;
    if (h * w * channels >= (1ll << 31)) return false;
    memset(g, 0, sizeof *g);
    g->w = (int)w;
    g->h = (int)h;
    g->ncomp = channels;
    g->hs = channels == 3 && subsampling >= 1 ? 2 : 1;
    g->vs = channels == 3 && subsampling == 2 ? 2 : 1;
    g->ny = g->hs * g->vs;
    // one component: a scan of its own, one block per MCU whatever its sampling factors say -- but Pillow still writes the
    // factors it was asked for into the frame header, and so does jpeg_enc_header
    g->sof_sampling = (subsampling >= 1 ? 2 : 1) << 4 | (subsampling == 2 ? 2 : 1);
    g->bpm = channels == 3 ? g->ny + 2 : 1;
    g->mcux = (int)((w + 8 * g->hs - 1) / (8 * g->hs));
    g->mcuy = (int)((h + 8 * g->vs - 1) / (8 * g->vs));
    g->nmcu = (long long)g->mcux * g->mcuy;
    g->nblocks = g->nmcu * g->bpm;
    for (int c = 0; c < channels; ++c) {
        const int fh = c ? g->hs : 1, fv = c ? g->vs : 1;
        g->wb[c] = (int)(((w + fh - 1) / fh + 7) / 8);
        g->hb[c] = (int)(((h + fv - 1) / fv + 7) / 8);
    }
    return true;
}

void jpeg_enc_qtable(int quality, int which, uint8_t out[64])
{
    const uint8_t *base = which ? JE_QBASE_CHROMA : JE_QBASE_LUMA;
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; ++i) {
        const int v = (base[i] * s + 50) / 100;
        out[i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

static void codes_of(const HuffSpec &t, uint16_t *code, uint8_t *len)
{
    int c = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {                          // the canonical assignment of annex C
        for (int i = 0; i < t.bits[l - 1]; ++i, ++k, ++c) {
            code[t.vals[k]] = (uint16_t)c;
            len[t.vals[k]] = (uint8_t)l;
        }
        c <<= 1;
    }
}

void jpeg_enc_codes(JpegEncCodes *c)
{
    memset(c, 0, sizeof *c);
    for (int t = 0; t < 2; ++t) {
        uint16_t code[256] = {0};
        uint8_t len[256] = {0};
        codes_of(JE_DC[t], code, len);
        memcpy(c->dc_code[t], code, sizeof c->dc_code[t]);
        memcpy(c->dc_len[t], len, sizeof c->dc_len[t]);
        codes_of(JE_AC[t], c->ac_code[t], c->ac_len[t]);
    }
}

int jpeg_enc_max_block_bits()
{
    JpegEncCodes c;
    jpeg_enc_codes(&c);
    int worst = 0;
    for (int t = 0; t < 2; ++t) {
        int dc = 0, ac = 0;
        for (int s = 0; s < 12; ++s)                         // a DC symbol is its category: that many extra bits follow
            if (c.dc_len[t][s] && c.dc_len[t][s] + s > dc) dc = c.dc_len[t][s] + s;
        for (int s = 0; s < 256; ++s)                        // an AC symbol: run << 4 | size, size extra bits follow
            if (c.ac_len[t][s] && (s & 15) && c.ac_len[t][s] + (s & 15) > ac) ac = c.ac_len[t][s] + (s & 15);
        if (dc + 63 * ac > worst) worst = dc + 63 * ac;
    }
    return worst;
}

static uint8_t *put_segment(uint8_t *p, int marker, int body)
{
    *p++ = 0xFF;
    *p++ = (uint8_t)marker;
    *p++ = (uint8_t)((body + 2) >> 8);
    *p++ = (uint8_t)((body + 2) & 255);
    return p;
}

int jpeg_enc_header(const JpegEncGeo &g, int quality, uint8_t *out)
{
    uint8_t *p = out;
    *p++ = 0xFF;
    *p++ = 0xD8;
    p = put_segment(p, 0xE0, 14);                            // JFIF 1.01, no units, density 1 x 1, no thumbnail
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(p, jfif, 14);
    p += 14;
    const int ntab = g.ncomp == 3 ? 2 : 1;
    for (int t = 0; t < ntab; ++t) {
        uint8_t q[64];
        jpeg_enc_qtable(quality, t, q);
        p = put_segment(p, 0xDB, 65);
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = q[JE_ZIGZAG[k]];
    }
    p = put_segment(p, 0xC0, 6 + 3 * g.ncomp);
    *p++ = 8;
    *p++ = (uint8_t)(g.h >> 8);
    *p++ = (uint8_t)(g.h & 255);
    *p++ = (uint8_t)(g.w >> 8);
    *p++ = (uint8_t)(g.w & 255);
    *p++ = (uint8_t)g.ncomp;
    for (int c = 0; c < g.ncomp; ++c) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c ? 0x11 : g.sof_sampling);
        *p++ = (uint8_t)(c ? 1 : 0);
    }
    for (int t = 0; t < ntab; ++t)
        for (int cls = 0; cls < 2; ++cls) {
            const HuffSpec &h = cls ? JE_AC[t] : JE_DC[t];
            p = put_segment(p, 0xC4, 17 + h.nvals);
            *p++ = (uint8_t)(cls << 4 | t);
            memcpy(p, h.bits, 16);
            memcpy(p + 16, h.vals, (size_t)h.nvals);
            p += 16 + h.nvals;
        }
    p = put_segment(p, 0xDA, 4 + 2 * g.ncomp);
    *p++ = (uint8_t)g.ncomp;
    for (int c = 0; c < g.ncomp; ++c) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c ? 0x11 : 0x00);
    }
    *p++ = 0;
    *p++ = 63;
    *p++ = 0;
    return (int)(p - out);
}

}  // namespace lars

using namespace lars;

extern "C" {

// header + every block at its longest (jpeg_enc_max_block_bits), every byte of that an FF that takes a 00 after it, + EOI
size_t lars_jpeg_bound(int64_t h, int64_t w, int channels, int subsampling)
{
    JpegEncGeo g;
    if (!jpeg_enc_geometry(h, w, channels, subsampling, &g)) return 0;
    uint8_t head[LARS_JPEG_HEADER_MAX];
    const size_t nhead = (size_t)jpeg_enc_header(g, 75, head);
    const size_t data = ((size_t)g.nblocks * (size_t)jpeg_enc_max_block_bits() + 7) / 8;
    return nhead + 2 * data + 2;
}

int64_t lars_jpeg_header(int64_t h, int64_t w, int channels, int subsampling, int quality, uint8_t *out, size_t out_cap)
{
    JpegEncGeo g;
    if (!out || quality < 1 || quality > 100 || !jpeg_enc_geometry(h, w, channels, subsampling, &g)) {
        set_error("lars_jpeg_header: a 1 to 65500 picture of 1 or 3 channels, subsampling 0 to 2, quality 1 to 100");
        return 0;
    }
    uint8_t head[LARS_JPEG_HEADER_MAX];
    const int n = jpeg_enc_header(g, quality, head);
    if ((size_t)n > out_cap) {
        set_error("lars_jpeg_header: the header needs %d bytes, out_cap is %zu", n, out_cap);
        return 0;
    }
    memcpy(out, head, (size_t)n);
    return n;
}

}  // extern "C"
