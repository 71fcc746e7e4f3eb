// What the host side of the JPEG encoder (jpeg_tables.cpp) hands to the device side (jpeg_encode.hip): the geometry of a
// frame, the quantisation tables of a quality, the standard Huffman codes and the file's header bytes.  No HIP here.
#pragma once
#include <stdint.h>

namespace lars {

#define LARS_JPEG_HEADER_MAX 640           // SOI .. SOS of a three-component file is 623 bytes

struct JpegEncGeo {
    int w, h, ncomp, hs, vs;               // sampling of component 0 (the others are 1 x 1)
    int bpm, ny;                           // blocks per MCU, of which component 0's
    int sof_sampling;                      // component 0's sampling byte of SOF0 (one component: written, not used)
    int mcux, mcuy;
    long long nmcu, nblocks;               // blocks in scan order, dummy blocks included
    int wb[3], hb[3];                      // each component's own size in blocks: beyond it a block of an MCU is a dummy
};

struct JpegEncCodes {                      // [0] luminance, [1] chrominance; length 0: the table has no such symbol
    uint16_t dc_code[2][12], ac_code[2][256];
    uint8_t dc_len[2][12], ac_len[2][256];
};

// subsampling: Pillow's numbers, 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (one channel: only the frame header shows it).  false: cannot be encoded.
bool jpeg_enc_geometry(int64_t h, int64_t w, int channels, int subsampling, JpegEncGeo *g);
// Annex K.1 table `which` (0 luminance, 1 chrominance) scaled as libjpeg's jpeg_set_quality does, natural order
void jpeg_enc_qtable(int quality, int which, uint8_t out[64]);
void jpeg_enc_codes(JpegEncCodes *c);
// the zigzag scan: position k holds the natural (row-major) index of coefficient k
extern const uint8_t JE_ZIGZAG[64];
// the most bits one block can take: the longest DC code plus its extra bits, and that of an AC code for all 63 coefficients
int jpeg_enc_max_block_bits();
// SOI, APP0, DQT(s), SOF0, DHTs, SOS into out[LARS_JPEG_HEADER_MAX]; returns the length
int jpeg_enc_header(const JpegEncGeo &g, int quality, uint8_t *out);

}  // namespace lars
