// What the host parser of the JPEG decoder (jpeg_parse.cpp) hands to the device side (jpeg_decode.hip).  No HIP here.
#pragma once
#include <stdint.h>

namespace lars {

struct JpegHeader {
    int w, h, ncomp, sof, precision;   // sof: the frame's marker byte (0xC0 baseline, 0xC1 extended sequential, ...)
    int cid[4], hs[4], vs[4], tq[4];   // frame components: id, sampling, quantisation table
    int td[4], ta[4];                  // scan: DC / AC table of each frame component
    int ri;                            // restart interval in MCUs (0: none)
    int64_t eoff, elen;                // the entropy-coded segment: file[eoff .. eoff + elen)
    int supported, reason;             // LARS_JPEG_REASON_*
    int jfif, adobe, adobe_transform;
    uint8_t q_set[4], h_set[8];        // h index: 0-3 DC tables, 4-7 AC tables
    uint16_t qt[4][64];                // natural (row-major) order
    uint8_t hcount[8][16], hval[8][256];
};

// Walks file[0..len) up to the end of the first scan's entropy data (scan_entropy) or up to the end of its SOS header
// (a file head of exactly that length).  LARS_OK with H->supported / H->reason set, or LARS_ERR_INVALID for damage.
int jpeg_parse(const uint8_t *file, int64_t len, JpegHeader *H, bool scan_entropy);

}  // namespace lars
