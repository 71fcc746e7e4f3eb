// Host side of the JPEG decoder: the marker segments of a JPEG file, validated without a device (lars_jpeg_info), and
// the tables the kernels need (jpeg_parse).  Every length is checked against the file before it is used; what the
// decoder does not cover is reported as unsupported with a reason, what is broken as an error.  No HIP here: builds into
// liblars_hip.so and with plain g++ under AddressSanitizer / UBSan (`make asan`).
#include <string.h>

#include "host_common.h"
#include "jpeg_parse.h"
#include "jpeg_tables.h"

namespace {

int be16(const uint8_t *p) { return p[0] << 8 | p[1]; }

void unsupported(lars::JpegHeader *H, int reason)
{
    if (H->supported) {
        H->supported = 0;
        H->reason = reason;
    }
}

}  // namespace

namespace lars {

int jpeg_parse(const uint8_t *file, int64_t len, JpegHeader *H, bool scan_entropy)
{
    memset(H, 0, sizeof *H);
    H->supported = 1;
    H->adobe_transform = -1;
    if (len < 4 || file[0] != 0xFF || file[1] != 0xD8) return fail(LARS_ERR_INVALID, "jpeg: missing SOI (not a JPEG file)");
    int64_t pos = 2;
    bool frame = false;
    for (;;) {
        if (len - pos < 2) return fail(LARS_ERR_INVALID, "jpeg: missing SOS (the file ends at byte %lld)", (long long)pos);
        if (file[pos] != 0xFF) return fail(LARS_ERR_INVALID, "jpeg: byte %#04x at %lld where a marker should be", file[pos], (long long)pos);
        const int m = file[pos + 1];
        if (m == 0xFF) { ++pos; continue; }               // fill byte
        pos += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // markers without a segment
        if (m == 0xD9) return fail(LARS_ERR_INVALID, "jpeg: missing SOS (EOI at byte %lld)", (long long)pos - 2);
        if (m == 0x00) return fail(LARS_ERR_INVALID, "jpeg: stuffed byte outside entropy data at %lld", (long long)pos - 2);
        if (len - pos < 2) return fail(LARS_ERR_INVALID, "jpeg: segment %#04x at byte %lld has no length", m, (long long)pos - 2);
        const int L = be16(file + pos);
        if (L < 2 || L > len - pos)
            return fail(LARS_ERR_INVALID, "jpeg: bad segment length %d of marker %#04x at byte %lld (%lld bytes left)", L, m,
                        (long long)pos - 2, (long long)(len - pos));
        const uint8_t *s = file + pos + 2;
        const int n = L - 2;
        if (m == 0xDB) {                                                     // DQT
            int i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (pq > 1 || tq > 3 || n - i - 1 < (pq ? 128 : 64)) return fail(LARS_ERR_INVALID, "jpeg: bad DQT segment at byte %lld", (long long)pos - 2);
                ++i;
                for (int k = 0; k < 64; ++k) {
                    H->qt[tq][lars::JE_ZIGZAG[k]] = (uint16_t)(pq ? be16(s + i + 2 * k) : s[i + k]);
                }
                i += pq ? 128 : 64;
                H->q_set[tq] = 1;
            }
        } else if (m == 0xC4) {                                              // DHT
            int i = 0;
            while (i < n) {
                if (n - i < 17) return fail(LARS_ERR_INVALID, "jpeg: bad DHT segment at byte %lld", (long long)pos - 2);
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return fail(LARS_ERR_INVALID, "jpeg: bad DHT table id %#04x at byte %lld", s[i], (long long)pos - 2);
                int total = 0;
                long long space = 1;                                         // codes still free at this length
                for (int l = 0; l < 16; ++l) {
                    space = space * 2 - s[i + 1 + l];
                    total += s[i + 1 + l];
                    if (space < 0) return fail(LARS_ERR_INVALID, "jpeg: Huffman table %d/%d is oversubscribed at length %d", tc, th, l + 1);
                }
                if (total > 256 || n - i - 17 < total)
                    return fail(LARS_ERR_INVALID, "jpeg: Huffman table %d/%d holds %d codes in a segment of %d bytes", tc, th, total, n);
                const int t = tc * 4 + th;
                memcpy(H->hcount[t], s + i + 1, 16);
                memset(H->hval[t], 0, 256);
                memcpy(H->hval[t], s + i + 17, (size_t)total);
                H->h_set[t] = 1;
                i += 17 + total;
            }
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {       // SOFn (0xC4 is DHT, handled above)
            if (frame) return fail(LARS_ERR_INVALID, "jpeg: second frame header at byte %lld", (long long)pos - 2);
            if (n < 6) return fail(LARS_ERR_INVALID, "jpeg: frame header of %d bytes", n);
            frame = true;
            H->sof = m;
            H->precision = s[0];
            H->h = be16(s + 1);
            H->w = be16(s + 3);
            H->ncomp = s[5];
            if (H->ncomp < 1 || n != 6 + 3 * H->ncomp) return fail(LARS_ERR_INVALID, "jpeg: frame header of %d bytes for %d components", n, H->ncomp);
            if (H->w == 0) return fail(LARS_ERR_INVALID, "jpeg: frame of width 0");
            if (m == 0xC2) unsupported(H, LARS_JPEG_REASON_PROGRESSIVE);
            else if (m != 0xC0 && m != 0xC1) unsupported(H, LARS_JPEG_REASON_FRAME);
            if (H->precision != 8) unsupported(H, LARS_JPEG_REASON_PRECISION);
            if (H->h == 0) unsupported(H, LARS_JPEG_REASON_DNL);
            if (H->ncomp != 1 && H->ncomp != 3) unsupported(H, LARS_JPEG_REASON_COMPONENTS);
            for (int c = 0; c < H->ncomp && c < 4; ++c) {
                H->cid[c] = s[6 + 3 * c];
                H->hs[c] = s[7 + 3 * c] >> 4;
                H->vs[c] = s[7 + 3 * c] & 15;
                H->tq[c] = s[8 + 3 * c];
                if (H->hs[c] < 1 || H->hs[c] > 4 || H->vs[c] < 1 || H->vs[c] > 4 || H->tq[c] > 3)
                    return fail(LARS_ERR_INVALID, "jpeg: component %d has sampling %d x %d, table %d", c, H->hs[c], H->vs[c], H->tq[c]);
            }
            if (H->ncomp == 1) H->hs[0] = H->vs[0] = 1;                      // a scan of one component has one block per MCU
            if (H->ncomp == 3) {
                const bool y_ok = (H->hs[0] == 1 && H->vs[0] == 1) || (H->hs[0] == 2 && H->vs[0] == 1) || (H->hs[0] == 2 && H->vs[0] == 2);
                if (!y_ok || H->hs[1] != 1 || H->vs[1] != 1 || H->hs[2] != 1 || H->vs[2] != 1) unsupported(H, LARS_JPEG_REASON_SAMPLING);
            }
        } else if (m == 0xDD) {                                              // DRI
            if (n != 2) return fail(LARS_ERR_INVALID, "jpeg: DRI segment of %d bytes", n);
            H->ri = be16(s);
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(s, "JFIF\0", 5) == 0) H->jfif = 1;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { H->adobe = 1; H->adobe_transform = s[11]; }
        } else if (m == 0xDC) {
            unsupported(H, LARS_JPEG_REASON_DNL);
        } else if (m == 0xDA) {                                              // SOS
            if (!frame) return fail(LARS_ERR_INVALID, "jpeg: SOS at byte %lld before any frame header (SOF after SOS)", (long long)pos - 2);
            if (n < 1 || s[0] < 1 || s[0] > 4 || n != 4 + 2 * s[0]) return fail(LARS_ERR_INVALID, "jpeg: bad SOS header at byte %lld", (long long)pos - 2);
            const int ns = s[0];
            if (ns != H->ncomp) unsupported(H, LARS_JPEG_REASON_SCANS);
            for (int c = 0; c < ns && H->supported; ++c) {
                if (s[1 + 2 * c] != H->cid[c]) { unsupported(H, LARS_JPEG_REASON_SCANS); break; }
                H->td[c] = s[2 + 2 * c] >> 4;
                H->ta[c] = s[2 + 2 * c] & 15;
                if (H->td[c] > 3 || H->ta[c] > 3) return fail(LARS_ERR_INVALID, "jpeg: SOS names Huffman tables %d / %d", H->td[c], H->ta[c]);
            }
            if (H->supported && H->ncomp == 3) {                             // libjpeg's colour space rules
                bool ycc = true;
                if (H->jfif) ycc = true;
                else if (H->adobe) ycc = H->adobe_transform != 0;
                else if (H->cid[0] == 'R' && H->cid[1] == 'G' && H->cid[2] == 'B') ycc = false;
                if (!ycc) unsupported(H, LARS_JPEG_REASON_COLORSPACE);
            }
            if (H->supported) {
                if ((int64_t)H->h * H->w * H->ncomp >= (1ll << 31)) unsupported(H, LARS_JPEG_REASON_SIZE);
                for (int c = 0; c < H->ncomp; ++c) {
                    if (!H->q_set[H->tq[c]]) return fail(LARS_ERR_INVALID, "jpeg: missing DQT: quantisation table %d of component %d", H->tq[c], c);
                    if (!H->h_set[H->td[c]]) return fail(LARS_ERR_INVALID, "jpeg: missing DHT: DC table %d of component %d", H->td[c], c);
                    if (!H->h_set[4 + H->ta[c]]) return fail(LARS_ERR_INVALID, "jpeg: missing DHT: AC table %d of component %d", H->ta[c], c);
                    int total = 0;
                    for (int l = 0; l < 16; ++l) total += H->hcount[H->td[c]][l];
                    for (int k = 0; k < total; ++k)
                        if (H->hval[H->td[c]][k] > 15) return fail(LARS_ERR_INVALID, "jpeg: DC table %d holds the category %d", H->td[c], H->hval[H->td[c]][k]);
                }
            }
            pos += L;
            break;
        }
        pos += L;
    }
    H->eoff = pos;
    H->elen = 0;
    if (!scan_entropy) return LARS_OK;
    // the entropy-coded segment ends at the first marker that is neither a stuffed FF, a fill byte nor RSTn
    int64_t p = pos;
    int next = -1;
    while (p < len) {
        const uint8_t *ff = static_cast<const uint8_t *>(memchr(file + p, 0xFF, (size_t)(len - p)));
        if (!ff) { p = len; break; }
        p = ff - file;
        int64_t q = p + 1;
        while (q < len && file[q] == 0xFF) ++q;                              // fill bytes
        if (q >= len) { p = len; break; }                                    // FFs up to the end of the file: part of no marker
        const int b = file[q];
        if (b == 0x00 || (b >= 0xD0 && b <= 0xD7)) { p = q + 1; continue; }
        next = b;
        break;
    }
    H->elen = p - pos;
    if (next == 0xDC) unsupported(H, LARS_JPEG_REASON_DNL);
    else if (next >= 0 && next != 0xD9) unsupported(H, LARS_JPEG_REASON_SCANS);   // more tables or scans follow
    return LARS_OK;
}

}  // namespace lars

using namespace lars;

extern "C" int lars_jpeg_info(const uint8_t *file, int64_t len, int64_t info[LARS_JPEG_INFO_N])
{
    if (!file || len < 0 || !info) return fail(LARS_ERR_INVALID, "lars_jpeg_info: bad arguments");
    memset(info, 0, sizeof(int64_t) * LARS_JPEG_INFO_N);
    JpegHeader H;
    LARS_TRY(jpeg_parse(file, len, &H, true));
    info[LARS_JPEG_INFO_WIDTH] = H.w;
    info[LARS_JPEG_INFO_HEIGHT] = H.h;
    info[LARS_JPEG_INFO_COMPONENTS] = H.ncomp;
    info[LARS_JPEG_INFO_FRAME] = H.sof;
    info[LARS_JPEG_INFO_PRECISION] = H.precision;
    for (int c = 0; c < 3 && c < H.ncomp; ++c) {
        info[LARS_JPEG_INFO_H0 + LARS_JPEG_INFO_SAMPLING_STRIDE * c] = H.hs[c];
        info[LARS_JPEG_INFO_V0 + LARS_JPEG_INFO_SAMPLING_STRIDE * c] = H.vs[c];
    }
    info[LARS_JPEG_INFO_RESTART_INTERVAL] = H.ri;
    info[LARS_JPEG_INFO_ENTROPY_OFFSET] = H.eoff;
    info[LARS_JPEG_INFO_ENTROPY_BYTES] = H.elen;
    info[LARS_JPEG_INFO_SUPPORTED] = H.supported;
    info[LARS_JPEG_INFO_REASON] = H.reason;
    return LARS_OK;
}
