// TIFF files decoded on the device (lars_h_decode_tiff, lars_h_thumbnail_tiff_u8 and their _deflate siblings): the whole file
// goes up once, every LZW or Deflate strip / tile is decoded by one wave into its own padded buffer, and one assembly pass
// writes the picture: byte order, horizontal predictor, planar -> chunky, tile cropping.  The directory is read on the host
// (tiff_parse.cpp).  Samples are 1 or 2 bytes of an unsigned integer or the 4 bytes of a float32, which the assembly pass moves
// as 32-bit patterns; the floating-point predictor (3, libtiff's fpAcc) is its third branch.
//
// The LZW stage never builds the string table.  Between two Clear codes ("a segment", codes c_0, c_1, ...):
//   * code i is 9 bits wide for i <= 253, 10 for i <= 765, 11 for i <= 1789, 12 after that, so its bit offset is a closed
//     form of i and 64 lanes read 64 codes at once;
//   * table entry 258 + j is str(c_j) + first(str(c_{j+1})): with L_i the output length of code i and P its exclusive
//     prefix sum, a code c_i >= 258 (j = c_i - 258 <= i - 1) has L_i = L_j + 1 and its output is a copy of the L_i bytes
//     that start at P_j, already written earlier in the same segment (j = i - 1, KwKwK, overlaps its own first byte).
// lars_h_tiff_lzw_decode (tiff_codec.cpp) is the specification: what it calls corrupt is corrupt here, at the same code.
// tests/tiff_lzw_model.py restates the phases below in NumPy and checks every index they form.
//
// The Deflate stage (k_td_inflate, only behind the _deflate entry points) takes one zlib stream per strip / tile.  Inside a
// chunk one lane decodes the symbols, so a file written as one huge strip is decoded by one lane; the wave only builds the
// tables and writes the bytes.  tiffio._chunk on zlib is the specification, tests/tiff_inflate_model.py the restatement.
#include <algorithm>
#include <vector>

#include "checksum_device.h"
#include "codec_host.h"
#include "common.h"
#include "inflate_device.h"

namespace lars {

namespace {

constexpr int TD_PCAP = 3840;      // P[] entries kept per segment: entry 258 + j exists for j <= 3837 and needs P[j + 1]
constexpr int TD_STAGE = 4096;     // bytes of one batch staged in LDS; the longest string is 3839 bytes
constexpr int TD_CLEAR = 256, TD_EOI = 257, TD_FIRST = 258;
constexpr int TD_NONE = 0, TD_LZW = 1, TD_DEFLATE = 2;   // TdGeom.codec
constexpr int TD_ZBATCH = 256;     // Deflate: records one lane decodes between two expansions by the wave
constexpr int TD_ZWIN = 2048;      // Deflate: bytes of the stream the wave stages in LDS for one batch (a record takes at most 48 bits)

struct TdGeom {
    long long nchunks, full;       // bytes of a whole strip / tile = the pitch of the chunk buffers
    int width, height, spp, bps;   // bps: bytes per sample (4: float32)
    int planes, inner, across, down, chunk_w, chunk_h;
    int tiled, predictor, big, codec;
};

struct TdCtl {
    int status[2];                 // LARS_TIFD_*, the strip / tile
    int produced, pad;             // bytes that strip / tile gave
};

// bits in front of code i of a segment, and the width of code i
__device__ inline unsigned long long td_bits_before(unsigned long long i)
{
    const unsigned long long a = i < 254 ? i : 254, b = i < 254 ? 0 : (i < 766 ? i - 254 : 512), c = i < 766 ? 0 : (i < 1790 ? i - 766 : 1024),
                             d = i < 1790 ? 0 : i - 1790;
    return 9 * a + 10 * b + 11 * c + 12 * d;
}

// stored rows of chunk k and the bytes the directory says it holds
__device__ __host__ inline long long td_want(const TdGeom &g, long long k)
{
    const long long ty = (k / g.across) % g.down;
    const long long left = (long long)g.height - ty * g.chunk_h;
    const long long rows = g.tiled ? g.chunk_h : (left < g.chunk_h ? left : g.chunk_h);
    return rows * g.chunk_w * g.inner * g.bps;
}

// One wave per strip / tile.  A batch is up to 64 codes of one segment: read, searched for Clear / EOI / the end of the input
// / a code the table does not hold, given lengths and offsets, copied into the LDS stage (sources in front of the batch come
// from the chunk buffer, sources inside it from the stage), and flushed.  produced[k]: bytes that came out; bad[k]: the
// host decoder would have refused the stream before the chunk was full.
__global__ __launch_bounds__(64) void k_td_lzw(const uint8_t *__restrict__ file, long long file_len, const long long *__restrict__ table,
                                               TdGeom g, uint8_t *bufs, int *__restrict__ produced, int *__restrict__ bad)
{
    __shared__ unsigned int P[TD_PCAP];
    __shared__ uint8_t stage[TD_STAGE];
    const int lane = threadIdx.x;
    const long long k = blockIdx.x;
    if (k >= g.nchunks) return;
    const long long off = table[2 * k], cnt = table[2 * k + 1];
    if (off < 0 || cnt < 0 || off > file_len || cnt > file_len - off || g.full <= 0 || g.full >= (1ll << 31)) {   // the parser checked this
        if (lane == 0) produced[k] = 0, bad[k] = 1;
        return;
    }
    const uint8_t *src = file + off;
    uint8_t *dst = bufs + k * g.full;
    const unsigned int ndst = (unsigned int)g.full;
    const unsigned long long nbits = (unsigned long long)cnt * 8;
    unsigned long long seg_bit = 0;      // bit position of code 0 of the segment
    unsigned long long seg_i = 0;        // codes of the segment already written
    unsigned int op = 0;                 // bytes written
    int err = 0;
    for (;;) {
        // ---- 64 codes by closed-form offsets
        const unsigned long long i = seg_i + lane;
        const unsigned long long at = seg_bit + td_bits_before(i);
        const int width = tiff_lzw_width(i);
        const bool avail = at + width <= nbits;
        int code = 0;
        if (avail) {
            const unsigned long long byte = at >> 3;
            unsigned int v = (unsigned int)src[byte] << 16;                       // byte < cnt: at + width <= 8 cnt
            if (byte + 1 < (unsigned long long)cnt) v |= (unsigned int)src[byte + 1] << 8;
            if (byte + 2 < (unsigned long long)cnt) v |= src[byte + 2];
            code = (int)((v >> (24 - (int)(at & 7) - width)) & ((1u << width) - 1u));
        }
        // ---- the first Clear / EOI / end of input, the first code above the fill level (a non-literal first code is one)
        const bool term = !avail || code == TD_CLEAR || code == TD_EOI;
        const long long j = (long long)code - TD_FIRST;                           // the entry's index, for code >= 258
        const bool wrong = !term && code >= TD_FIRST && j > (long long)i - 1;
        const unsigned long long m_term = __ballot(term), m_wrong = __ballot(wrong);
        const int n_term = m_term ? __ffsll((long long)m_term) - 1 : 64, n_wrong = m_wrong ? __ffsll((long long)m_wrong) - 1 : 64;
        const int ndata = n_term < n_wrong ? n_term : n_wrong;
        const bool active = lane < ndata;
        // ---- lengths: L_i = 1, or L_j + 1 with j <= i - 1 <= 3837; j in front of the batch: from P[], inside it: from its lane
        if (lane == 0 && seg_i < TD_PCAP) P[seg_i] = op;
        __syncthreads();
        const bool copy = active && code >= TD_FIRST;
        const bool inside = copy && (unsigned long long)j >= seg_i;
        int L = 0;
        if (active) L = 1;
        if (copy && !inside && j + 1 < TD_PCAP) L = (int)(P[j + 1] - P[j]) + 1;
        bool need = inside;
        const int jl = inside ? (int)((unsigned long long)j - seg_i) : 0;         // < lane
        unsigned long long known = __ballot(!need);
        while (known != ~0ull) {
            const int from = __shfl(L, jl);
            if (need && ((known >> jl) & 1)) L = from + 1, need = false;
            known = __ballot(!need);
        }
        // ---- offsets: the inclusive scan of L
        int incl = L;
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int up = __shfl_up(incl, dlt);
            if (lane >= dlt) incl += up;
        }
        const unsigned long long start64 = (unsigned long long)op + (unsigned int)(incl - L), end64 = (unsigned long long)op + (unsigned int)incl;
        // the host stops after a code that fills the chunk; a first code finds it full only when the literal before a Clear filled it
        const bool stop = active && ((i >= 1 && end64 >= ndst) || (i == 0 && start64 >= ndst));
        const unsigned long long m_stop = __ballot(stop);
        const int n_stop = m_stop ? __ffsll((long long)m_stop) : 65;          // codes up to and including the stopping one
        const int n_stage = __popcll(__ballot(active && incl <= TD_STAGE));   // incl grows with the lane: a prefix
        int nproc = ndata;
        if (n_stop < nproc) nproc = n_stop;
        if (n_stage < nproc) nproc = n_stage;
        const bool mine = lane < nproc;
        const unsigned int start = (unsigned int)start64;                     // < 2^31 + 64 * 3839 for every lane that is `mine`
        if (mine && i < TD_PCAP) P[i] = start;
        // ---- bytes: rounds of lanes whose sources are written
        __syncthreads();
        unsigned int srcpos = 0;
        if (mine && copy && j < TD_PCAP) srcpos = P[j];                       // j <= i - 1: in front of the batch or a lower lane of it
        const int dep_a = (mine && inside) ? jl : -1;                         // the lane of code j
        const int dep_b = (mine && copy && (unsigned long long)(j + 1) >= seg_i && jl + (inside ? 1 : 0) != lane)
                              ? (inside ? jl + 1 : 0) : -1;                   // the lane of code j + 1, unless it is this one (KwKwK)
        bool todo = mine;
        unsigned long long done = __ballot(!todo);
        while (done != ~0ull) {
            const bool ready = todo && (dep_a < 0 || ((done >> dep_a) & 1)) && (dep_b < 0 || ((done >> dep_b) & 1));
            if (ready) {
                const unsigned int base = start - op;
                if (!copy) {
                    if (base < TD_STAGE) stage[base] = (uint8_t)code;
                } else {
                    for (int t = 0; t < L; ++t) {
                        const unsigned int s = srcpos + t;
                        uint8_t b = 0;
                        if (s < op) b = dst[s];                               // s < op <= ndst
                        else if (s - op < TD_STAGE) b = stage[s - op];
                        if (base + t < TD_STAGE) stage[base + t] = b;
                    }
                }
                todo = false;
            }
            __syncthreads();
            done = __ballot(!todo);
        }
        // ---- flush, clipped to the chunk
        const unsigned int total = nproc > 0 ? (unsigned int)__shfl(incl, nproc - 1) : 0;
        for (unsigned int q = lane; q < total && q < TD_STAGE; q += 64)
            if ((unsigned long long)op + q < ndst) dst[op + q] = stage[q];
        __syncthreads();
        // ---- what ended the batch
        if (nproc > 0 && nproc == n_stop) { op = ndst; break; }               // the chunk is full
        const unsigned long long op64 = (unsigned long long)op + total;
        op = (unsigned int)op64;                                              // < ndst: no code stopped
        seg_i += nproc;
        if (nproc < ndata) continue;                                          // the stage was full
        if (n_wrong < n_term) { err = 1; break; }
        if (n_term == 64) continue;
        const int tcode = __shfl(code, n_term);
        const int tavail = __shfl((int)avail, n_term);
        if (!tavail || tcode == TD_EOI) break;                                // out of input: what was decoded stands
        seg_bit += td_bits_before(seg_i) + tiff_lzw_width(seg_i);                   // past the Clear
        seg_i = 0;
    }
    if (lane == 0) produced[k] = (int)op, bad[k] = err;
}

// One wave per strip / tile, each a zlib stream of its own.  Lane 0 reads the zlib header and every block header
// (pd_header_t, in zlib's order: what is cut off is not judged); the wave builds the first-level tables and, for every batch,
// stages the next TD_ZWIN bytes of the stream in LDS (zeros behind the chunk's last byte), where lane 0's reader finds them
// without a trip to memory per word; lane 0 decodes up to TD_ZBATCH records (a literal, or length + distance) into LDS, fewer
// when it comes within 64 bytes of the window's end; the wave writes them: the literals at once, then copy after
// copy, each spread over the lanes with src = o - dist + k % dist, behind a barrier, because a copy reads chunk bytes that
// other lanes stored.  Each lane sums what it stores (sum x_i and sum i x_i) and the wave forms Adler-32 from the sums.
// Every loop below takes bits from the input or ends: a block header takes three, a symbol one.  Stores stay inside
// want <= full bytes of the chunk's buffer, loads inside the chunk's cnt bytes of the file (the reader gives zero bits behind
// them).  produced[k]: bytes that came out; bad[k]: 1 zlib calls the stream corrupt, 2 it wants to go on behind a full chunk.
struct TdInflate : PdCodes {
    unsigned int win[TD_ZWIN / 4];                 // the stream from the word that holds the batch's first bit
    unsigned int rec_o[TD_ZBATCH];                 // where the record's bytes go in the chunk
    unsigned short rec_d[TD_ZBATCH];               // distance 1 .. 32768, or 0: a literal
    unsigned short rec_l[TD_ZBATCH];               // length 1 .. 258, or the literal
    unsigned short cpy[TD_ZBATCH];                 // the records that are copies, in order
    int nrec, ncpy, end;                           // end: 0 the batch is full, 1 end of block, 2 decoding stops, 3 corrupt, 4 past
    unsigned int out;                              // bytes of the chunk behind the batch
    unsigned long long pos;                        // the bit behind the batch
};

__global__ __launch_bounds__(64) void k_td_inflate(const uint8_t *__restrict__ file, long long file_len, const long long *__restrict__ table,
                                                   TdGeom g, uint8_t *bufs, int *__restrict__ produced, int *__restrict__ bad)
{
    __shared__ TdInflate Z;
    const int lane = threadIdx.x;
    const long long k = blockIdx.x;
    if (k >= g.nchunks) return;
    const long long off = table[2 * k], cnt = table[2 * k + 1];
    const long long want64 = td_want(g, k);
    if (off < 0 || cnt < 0 || off > file_len || cnt > file_len - off || g.full <= 0 || g.full >= (1ll << 31) || want64 <= 0 || want64 > g.full) {
        if (lane == 0) produced[k] = 0, bad[k] = 1;      // the parser checked this
        return;
    }
    const uint8_t *src = file + off;
    const unsigned int *words = reinterpret_cast<const unsigned int *>(src);     // the byte reader's handle: never loaded as words
    uint8_t *dst = bufs + k * g.full;
    const unsigned int want = (unsigned int)want64;
    const unsigned long long nbytes = (unsigned long long)cnt, nbits = nbytes * 8;
    unsigned long long s1 = 0, s2 = 0;             // this lane's sum x_i and sum i x_i, below ADLER_MOD between batches
    unsigned long long pos = 16;
    unsigned int op = 0;                           // bytes written
    int status = 0;
    bool ended = false;                            // the final block's end was reached
    bool go = cnt >= 2;
    if (go) {
        const unsigned int cmf = src[0], flg = src[1];
        if (((cmf << 8) | flg) % 31 != 0 || (cmf & 15) != 8 || (cmf >> 4) > 7) status = 1, go = false;
        else if (flg & 32) status = cnt >= 6 ? 1 : 0, go = false;         // zlib asks for a dictionary once its id is there
    }
    while (go) {
        if (lane == 0) pd_header_t<false, true>(Z, words, nbytes, nbits, pos);
        __syncthreads();
        const int herr = Z.err, kind = Z.kind, fin = Z.final_;
        const unsigned long long dp = Z.data_pos;
        const bool cut = herr == 5 && kind == 0 && dp != 0;               // a stored block whose bytes end early
        if (herr && !cut) { status = herr == 5 ? 0 : 1; break; }
        if (kind == 0) {
            const unsigned long long left = (nbits - dp) >> 3;            // dp <= nbits: LEN / NLEN were read
            const unsigned int slen = Z.stored_len;
            const unsigned int there = left < slen ? (unsigned int)left : slen;
            const unsigned int take = there < want - op ? there : want - op;
            const uint8_t *sb = src + (dp >> 3);
            for (unsigned int t = lane; t < take; t += 64) {
                const unsigned int v = sb[t], i = op + t;                 // (dp >> 3) + t < cnt;  i < want
                dst[i] = (uint8_t)v;
                s1 += v; s2 += (unsigned long long)i * v;
            }
            s1 %= ADLER_MOD; s2 %= ADLER_MOD;
            op += take;
            __syncthreads();
            if (there > take) { status = 2; break; }                      // a stored byte that is there and has no room
            if (there < slen) break;
            pos = dp + 8ull * there;
        } else {
            pd_fast_tables(Z);
            if (lane == 0) Z.out = op, Z.pos = dp;
            __syncthreads();
            int end = 0;
            while (!end) {
                const unsigned long long wbase = (Z.pos >> 5) << 2;       // Z.pos <= nbits: wbase <= cnt
                {
                    BitReaderT<false> in;
                    in.w = words; in.nw = nbytes;
                    for (int i = lane; i < TD_ZWIN / 4; i += 64) Z.win[i] = in.word_at(wbase + 4ull * i);
                }
                __syncthreads();
                if (lane == 0) {
                    // positions below are relative to the window; so are nbits and nbytes (shadowing the chunk's)
                    const unsigned long long nbits = (unsigned long long)cnt * 8 - wbase * 8, nbytes = (unsigned long long)cnt - wbase;
                    BitReaderT<false> br;                                 // a reader per batch: it lives in registers
                    br.init(Z.win, TD_ZWIN, Z.pos - wbase * 8);
                    int nrec = 0, ncpy = 0, e = 0;
                    unsigned int out = Z.out;
                    while (nrec < TD_ZBATCH && br.pos() < (TD_ZWIN - 64) * 8ull) {
                        br.refill();
                        unsigned long long before = br.pos();
                        const int s = pd_symbol(br, Z.lfast, Z.lcnt, Z.lsym);
                        if (s < 0) { e = before + 1 > nbits ? 2 : 3; break; }
                        if (br.pos() > nbits) { e = 2; break; }
                        if (s < 256) {
                            if (out == want) { e = ((br.pos() + 7) >> 3) < nbytes ? 4 : 2; break; }
                            Z.rec_o[nrec] = out; Z.rec_d[nrec] = 0; Z.rec_l[nrec] = (unsigned short)s; ++nrec;
                            ++out;
                            continue;
                        }
                        if (s == 256) { e = 1; break; }
                        const int ls = s - 257;
                        if (ls >= 29) { e = 3; break; }
                        const unsigned int len = c_lbase[ls] + br.bits(c_lext[ls]);
                        if (br.pos() > nbits) { e = 2; break; }
                        br.refill();
                        before = br.pos();
                        const int ds = pd_symbol(br, Z.dfast, Z.dcnt, Z.dsym);
                        if (ds < 0) { e = before + 1 > nbits ? 2 : 3; break; }
                        if (br.pos() > nbits) { e = 2; break; }
                        if (ds >= 30) { e = 3; break; }
                        const unsigned int dist = c_dbase[ds] + br.bits(c_dext[ds]);
                        if (br.pos() > nbits) { e = 2; break; }
                        if (out == want) { e = ((br.pos() + 7) >> 3) < nbytes ? 4 : 2; break; }
                        if (dist > out) { e = 3; break; }
                        const unsigned int room = want - out;
                        Z.cpy[ncpy++] = (unsigned short)nrec;
                        Z.rec_o[nrec] = out; Z.rec_d[nrec] = (unsigned short)dist; Z.rec_l[nrec] = (unsigned short)(len < room ? len : room); ++nrec;
                        if (len > room) { out = want; e = ((br.pos() + 7) >> 3) < nbytes ? 4 : 2; break; }
                        out += len;
                    }
                    Z.nrec = nrec; Z.ncpy = ncpy; Z.end = e; Z.out = out; Z.pos = wbase * 8 + br.pos();
                }
                __syncthreads();
                const int nrec = Z.nrec;
                end = Z.end;
                if (end != 3) {
                    for (int r = lane; r < nrec; r += 64) {
                        if (Z.rec_d[r]) continue;
                        const unsigned int v = Z.rec_l[r], i = Z.rec_o[r];
                        if (i < want) dst[i] = (uint8_t)v;                // always: lane 0 counted against want
                        s1 += v; s2 += (unsigned long long)i * v;
                    }
                    const int ncpy = Z.ncpy;
                    for (int c = 0; c < ncpy; ++c) {
                        const int r = Z.cpy[c];                           // < nrec
                        __syncthreads();                                  // what this copy reads, other lanes have stored
                        const unsigned int d = Z.rec_d[r], o = Z.rec_o[r], len = Z.rec_l[r];
                        if (d == 0 || d > o || len > want - o) continue;  // never: lane 0 checked all three
                        for (unsigned int t = lane; t < len; t += 64) {
                            const unsigned int v = dst[o - d + (t < d ? t : t % d)], i = o + t;
                            dst[i] = (uint8_t)v;
                            s1 += v; s2 += (unsigned long long)i * v;
                        }
                    }
                    s1 %= ADLER_MOD; s2 %= ADLER_MOD;
                    op = Z.out;
                }
                pos = Z.pos;
                __syncthreads();                                          // the batch is in the chunk, the records are free again
            }
            if (end == 3) { status = 1; break; }
            if (end == 4) { status = 2; break; }
            if (end == 2) break;
        }
        if (fin) { ended = true; break; }
    }
    // the Adler-32 trailer, when the stream ended and its four bytes are there: 1 + sum x_i, n + n sum x_i - sum i x_i
    if (ended && status == 0) {
        const unsigned long long p = (pos + 7) >> 3;
        unsigned int a1 = (unsigned int)s1, a2 = (unsigned int)s2;
        for (int dlt = 32; dlt > 0; dlt >>= 1) a1 += __shfl_xor(a1, dlt), a2 += __shfl_xor(a2, dlt);   // 64 values below ADLER_MOD
        if (p + 4 <= nbytes) {
            const unsigned long long n = op % ADLER_MOD, t1 = a1 % ADLER_MOD, t2 = a2 % ADLER_MOD;
            const unsigned int a = (unsigned int)((1 + t1) % ADLER_MOD), b = (unsigned int)((n + n * t1 + ADLER_MOD - t2) % ADLER_MOD);
            const unsigned int stored = (unsigned int)src[p] << 24 | (unsigned int)src[p + 1] << 16 | (unsigned int)src[p + 2] << 8 | src[p + 3];
            if ((b << 16 | a) != stored) status = 1;
        }
    }
    if (lane == 0) produced[k] = (int)op, bad[k] = status;
}

// LZW: the first strip / tile the host decoder would refuse, else the first that gave too few bytes (read_tiff decodes every
// LZW chunk before it looks at the lengths).  Deflate: the first strip / tile with either fault (read_tiff inflates chunk by
// chunk).  bad[k]: 1 corrupt, 2 (Deflate only) inflates past its bytes.
__global__ void k_td_check(TdGeom g, const int *__restrict__ produced, const int *__restrict__ bad, TdCtl *ctl)
{
    __shared__ unsigned long long first_bad, first_short;
    if (threadIdx.x == 0) first_bad = first_short = ~0ull;
    __syncthreads();
    for (long long k = threadIdx.x; k < g.nchunks; k += blockDim.x) {
        const bool few = produced[k] < td_want(g, k);
        if (bad[k] || (few && g.codec == TD_DEFLATE)) atomicMin(&first_bad, (unsigned long long)k);
        else if (few) atomicMin(&first_short, (unsigned long long)k);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (first_bad != ~0ull && bad[first_bad] == 0)
            ctl->status[0] = LARS_TIFD_SHORT, ctl->status[1] = (int)first_bad, ctl->produced = produced[first_bad];
        else if (first_bad != ~0ull) ctl->status[0] = bad[first_bad] == 2 ? LARS_TIFD_PAST : LARS_TIFD_CORRUPT, ctl->status[1] = (int)first_bad;
        else if (first_short != ~0ull)
            ctl->status[0] = LARS_TIFD_SHORT, ctl->status[1] = (int)first_short, ctl->produced = produced[first_short];
    }
}

// sample e of a row in the file's byte order; byte loads, since an uncompressed strip starts wherever the file puts it
__device__ inline unsigned int td_sample(const uint8_t *__restrict__ src, long long e, int bps, int big)
{
    if (bps == 1) return src[e];
    if (bps == 2) return big ? (unsigned int)(src[2 * e] << 8 | src[2 * e + 1]) : (unsigned int)(src[2 * e + 1] << 8 | src[2 * e]);
    const uint8_t *b = src + 4 * e;
    return big ? (unsigned int)b[0] << 24 | (unsigned int)b[1] << 16 | (unsigned int)b[2] << 8 | b[3]
               : (unsigned int)b[3] << 24 | (unsigned int)b[2] << 16 | (unsigned int)b[1] << 8 | b[0];
}

// One wave per row of a strip / tile that lies inside the picture: samples in file byte order -> native samples, the running
// sum of predictor 2 as a wave scan per sample (it restarts with the row), planes interleaved, padding columns dropped.
// Predictor 3 (float32 only): the row is four byte planes of chunk_w * inner bytes, most significant first in either byte
// order, and the running sum with stride inner runs through all of them, padding columns included; so for each of the inner
// residues the same scan walks 4 * chunk_w positions, position t being plane t / chunk_w of pixel t % chunk_w, with the carry
// going from one group of 64 into the next and so from one plane into the next.  Each sum is one byte of one float and is
// stored as that byte (plane 0 is byte 3 of the native little-endian sample): no lane ever holds two bytes of one sample.
__global__ __launch_bounds__(256) void k_td_assemble(const uint8_t *__restrict__ file, long long file_len, const long long *__restrict__ table,
                                                     TdGeom g, const uint8_t *__restrict__ bufs, uint8_t *__restrict__ out, const TdCtl *ctl)
{
    if (ctl->status[0]) return;
    const int lane = threadIdx.x & 63;
    const long long units = (long long)g.planes * g.height * g.across;
    const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
    uint16_t *out16 = reinterpret_cast<uint16_t *>(out);
    unsigned int *out32 = reinterpret_cast<unsigned int *>(out);
    for (long long u = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < units; u += nwaves) {
        const long long tx = u % g.across, y = (u / g.across) % g.height, p = u / g.across / g.height;
        const long long ty = y / g.chunk_h, r = y % g.chunk_h;
        const long long k = (p * g.down + ty) * g.across + tx;
        const long long x0 = tx * g.chunk_w;
        const long long cols = g.width - x0 < g.chunk_w ? g.width - x0 : g.chunk_w;
        const long long row_bytes = (long long)g.chunk_w * g.inner * g.bps;
        const uint8_t *src;
        if (g.codec) {
            src = bufs + k * g.full + r * row_bytes;                         // r < chunk_h: inside the chunk buffer
        } else {
            const long long off = table[2 * k], cnt = table[2 * k + 1];
            if (off < 0 || cnt < (r + 1) * row_bytes || off > file_len || cnt > file_len - off) continue;   // the parser checked this
            src = file + off + r * row_bytes;
        }
        const long long o0 = (y * g.width + x0) * g.spp;                      // the row's first sample in the picture
        if (g.predictor == 3) {
            if (g.bps != 4) continue;                                        // the parser lets it through with float32 only
            const long long nt = 4ll * g.chunk_w;
            for (int s = 0; s < g.inner; ++s) {
                unsigned int carry = 0;                                      // only its low byte counts
                for (long long tb = 0; tb < nt; tb += 64) {
                    const long long t = tb + lane;
                    unsigned int v = t < nt ? src[t * g.inner + s] : 0u;     // t * inner + s < 4 * chunk_w * inner = row_bytes
                    for (int dlt = 1; dlt < 64; dlt <<= 1) {
                        const unsigned int up = __shfl_up(v, dlt);
                        if (lane >= dlt) v += up;
                    }
                    v += carry;
                    carry = __shfl(v, 63);
                    if (t < nt) {
                        const long long bp = t / g.chunk_w, x = t - bp * g.chunk_w;
                        if (x < cols) out[4 * (o0 + x * g.spp + (g.planes > 1 ? p : s)) + 3 - bp] = (uint8_t)v;
                    }
                }
            }
            continue;
        }
        if (g.predictor != 2) {
            const long long n = cols * g.inner;
            for (long long e = lane; e < n; e += 64) {
                const long long o = g.planes > 1 ? o0 + e * g.spp + p : o0 + e;
                const unsigned int v = td_sample(src, e, g.bps, g.big);
                if (g.bps == 1) out[o] = (uint8_t)v;
                else if (g.bps == 2) out16[o] = (uint16_t)v;
                else out32[o] = v;
            }
            continue;
        }
        for (int s = 0; s < g.inner; ++s) {
            unsigned int carry = 0;
            for (long long xb = 0; xb < cols; xb += 64) {
                const long long x = xb + lane;
                unsigned int v = 0;
                if (x < cols) {
                    v = td_sample(src, x * g.inner + s, g.bps, g.big);
                }
                for (int dlt = 1; dlt < 64; dlt <<= 1) {
                    const unsigned int up = __shfl_up(v, dlt);
                    if (lane >= dlt) v += up;
                }
                v += carry;
                carry = __shfl(v, 63);
                if (x < cols) {
                    const long long o = o0 + x * g.spp + (g.planes > 1 ? p : s);
                    if (g.bps == 1) out[o] = (uint8_t)v;
                    else if (g.bps == 2) out16[o] = (uint16_t)v;
                    else out32[o] = v;
                }
            }
        }
    }
}

// the TIFF side of the host entry points (codec_host.h)
struct TdFile : HostFile {
    TdGeom g;
    int64_t info[LARS_TIFF_INFO_N];
    std::vector<int64_t> table;
    TdCtl ctl_host;
    TdCtl *d_ctl;
    int *d_produced, *d_bad;
    uint8_t *d_bufs;
    bool deflate = false;          // the _deflate entry points: lars_tiff_info_deflate reads the directory

    int read_info(int64_t *chunk_table, int64_t table_cap)
    {
        return deflate ? lars_tiff_info_deflate(file, len, info, chunk_table, table_cap) : lars_tiff_info(file, len, info, chunk_table, table_cap);
    }
    void plan(Carver &cv)
    {
        d_ctl = cv.take<TdCtl>(1);
        d_produced = cv.take<int>(g.codec ? (size_t)g.nchunks : 0);
        d_bad = cv.take<int>(g.codec ? (size_t)g.nchunks : 0);
        d_bufs = cv.take<uint8_t>(g.codec ? (size_t)(g.nchunks * g.full) : 0);
    }
    int parse(const char *who_, const uint8_t *file_, int64_t len_)
    {
        who = who_; file = file_; len = len_;
        if (!file || len <= 0) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
        LARS_TRY(read_info(nullptr, 0));
        if (!info[LARS_TIFF_INFO_SUPPORTED])
            return fail(LARS_ERR_UNSUPPORTED, "%s: this TIFF file is not decoded on the device (LARS_TIFF_REASON %lld)", who,
                        (long long)info[LARS_TIFF_INFO_REASON]);
        h = info[LARS_TIFF_INFO_HEIGHT]; w = info[LARS_TIFF_INFO_WIDTH]; channels = (int)info[LARS_TIFF_INFO_SAMPLES];
        sample_bytes = (int)info[LARS_TIFF_INFO_BITS] / 8;
        const bool planar = info[LARS_TIFF_INFO_PLANAR] == 2;
        g.nchunks = info[LARS_TIFF_INFO_CHUNKS];
        g.width = (int)w; g.height = (int)h; g.spp = channels; g.bps = sample_bytes;
        g.planes = planar ? channels : 1; g.inner = planar ? 1 : channels;
        g.chunk_w = (int)info[LARS_TIFF_INFO_CHUNK_W]; g.chunk_h = (int)info[LARS_TIFF_INFO_CHUNK_H];
        g.across = (int)((w + g.chunk_w - 1) / g.chunk_w); g.down = (int)((h + g.chunk_h - 1) / g.chunk_h);
        g.tiled = (int)info[LARS_TIFF_INFO_TILED]; g.predictor = (int)info[LARS_TIFF_INFO_PREDICTOR];
        g.big = (int)info[LARS_TIFF_INFO_BIG_ENDIAN]; g.codec = info[LARS_TIFF_INFO_COMPRESSION] == 5 ? TD_LZW : info[LARS_TIFF_INFO_COMPRESSION] == 1 ? TD_NONE : TD_DEFLATE;
        g.full = (long long)g.chunk_h * g.chunk_w * g.inner * g.bps;
        extra_bytes = (size_t)g.nchunks * 16;                 // the chunk table
        Carver size(nullptr);
        plan(size);
        scratch_bytes = size.bytes();
        table.assign((size_t)g.nchunks * 2, 0);
        return read_info(table.data(), g.nchunks);
    }
    int enqueue(hipStream_t s)
    {
        Carver cv(d_scratch);
        plan(cv);
        long long *d_tab = static_cast<long long *>(d_extra);
        LARS_HIP_TRY(hipMemcpyAsync(d_tab, table.data(), extra_bytes, hipMemcpyHostToDevice, s));
        LARS_HIP_TRY(hipMemsetAsync(d_ctl, 0, sizeof(TdCtl), s));
        if (g.codec) {
            if (g.codec == TD_LZW)
                hipLaunchKernelGGL(k_td_lzw, dim3((unsigned)g.nchunks), dim3(64), 0, s, d_file, (long long)len, d_tab, g, d_bufs, d_produced, d_bad);
            else
                hipLaunchKernelGGL(k_td_inflate, dim3((unsigned)g.nchunks), dim3(64), 0, s, d_file, (long long)len, d_tab, g, d_bufs, d_produced, d_bad);
            hipLaunchKernelGGL(k_td_check, dim3(1), dim3(256), 0, s, g, d_produced, d_bad, d_ctl);
        }
        const long long units = (long long)g.planes * g.height * g.across;
        const unsigned grid = (unsigned)std::min<long long>((units + 3) / 4, 1 << 16);
        hipLaunchKernelGGL(k_td_assemble, dim3(grid), dim3(256), 0, s, d_file, (long long)len, d_tab, g, d_bufs, d_img, d_ctl);
        LARS_HIP_TRY(hipMemcpyAsync(d_status, d_ctl->status, 8, hipMemcpyDeviceToDevice, s));
        LARS_HIP_TRY(hipMemcpyAsync(&ctl_host, d_ctl, sizeof ctl_host, hipMemcpyDeviceToHost, s));
        return launch_check(who);
    }
    int finish(const int st[2])
    {
        switch (st[0]) {
        case LARS_TIFD_OK: return LARS_OK;
        case LARS_TIFD_CORRUPT:
            return fail(LARS_ERR_INVALID, "%s: corrupt %s data in chunk %d", who, g.codec == TD_DEFLATE ? "Deflate" : "LZW", st[1]);
        case LARS_TIFD_PAST:
            return fail(LARS_ERR_INVALID, "%s: Deflate strip / tile inflates past its %lld bytes (chunk %d)", who, td_want(g, st[1]), st[1]);
        case LARS_TIFD_SHORT:
            return fail(LARS_ERR_INVALID, "%s: strip / tile holds %d bytes, %lld expected", who, ctl_host.produced, td_want(g, st[1]));
        default: return fail(LARS_ERR_HIP, "%s: internal decoder status %d (%d)", who, st[0], st[1]);
        }
    }
};

}  // namespace

}  // namespace lars

using namespace lars;

extern "C" {

// host file in, host samples out: one upload, the status, one download
int lars_h_decode_tiff(const uint8_t *file, int64_t len, void *out, size_t out_cap)
{
    static const char *who = "lars_h_decode_tiff";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    TdFile F;
    LARS_TRY(F.parse(who, file, len));
    return decode_file_to_host(c, F, static_cast<uint8_t *>(out), out_cap);
}

// the same with Deflate strips / tiles decoded too (k_td_inflate); every other file as lars_h_decode_tiff
int lars_h_decode_tiff_deflate(const uint8_t *file, int64_t len, void *out, size_t out_cap)
{
    static const char *who = "lars_h_decode_tiff_deflate";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    TdFile F;
    F.deflate = true;
    LARS_TRY(F.parse(who, file, len));
    return decode_file_to_host(c, F, static_cast<uint8_t *>(out), out_cap);
}

// host file in, thumbnail out: the decoded pixels go straight into the thumbnail kernels (resize.hip)
static int thumbnail_tiff(const char *who, bool deflate, const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4],
                          const float box[4], int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out || !reduce_box || !box) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    TdFile F;
    F.deflate = deflate;
    LARS_TRY(F.parse(who, file, len));
    const int64_t spp = F.info[LARS_TIFF_INFO_SAMPLES], photometric = F.info[LARS_TIFF_INFO_PHOTOMETRIC];
    if (F.info[LARS_TIFF_INFO_BITS] != 8 || F.info[LARS_TIFF_INFO_EXTRA_SAMPLES] != 0 || !((spp == 1 && photometric == 1) || (spp == 3 && photometric == 2)))
        return fail(LARS_ERR_UNSUPPORTED, "%s: 8-bit files of one BlackIsZero sample or RGB (%lld samples of %lld bits, photometric %lld)", who,
                    (long long)spp, (long long)F.info[LARS_TIFF_INFO_BITS], (long long)photometric);
    return thumbnail_file(c, F, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

int lars_h_thumbnail_tiff_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                             int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    return thumbnail_tiff("lars_h_thumbnail_tiff_u8", false, file, len, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

int lars_h_thumbnail_tiff_deflate_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                                     int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    return thumbnail_tiff("lars_h_thumbnail_tiff_deflate_u8", true, file, len, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

}  // extern "C"
