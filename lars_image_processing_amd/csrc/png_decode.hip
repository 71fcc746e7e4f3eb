// PNG decoding on the device: 8-bit, non-interlaced pictures, and behind a switch every other bit depth and Adam7 interlace.
//
// Reference: load_image_from_db (process-images.py:181-193) opens every stored picture with Image.open(io.BytesIO(...))
// and np.array(img) or img.thumbnail(...): zlib's inflate and libpng-style unfiltering on one host core.  Here the
// compressed file goes up once and the pixels (or only the thumbnail, lars_h_thumbnail_png_u8) come back.
//
// Inflate is serial by nature; the speculation below is checked against the exact serial chain before anything is used,
// so it only changes the speed, never the result.  The host parser (png_parse.cpp) gives the IDAT table.
//   k_pd_chunk_scan  one workgroup: output offset of each IDAT payload (exclusive scan of the lengths).
//   k_pd_gather      one workgroup per IDAT chunk: payload into one contiguous stream, CRC-32 of type + payload (per-thread
//                    pieces shifted by x^(8 * bytes after them) mod P, as k_png_idat builds them) against the stored CRC.
//   k_pd_mark        one thread per bit offset: does a dynamic block start here that zlib's inflate would accept (HLIT,
//                    HDIST bounds, complete code-length code, repeats inside the table, literal/length and distance codes
//                    neither over-subscribed nor incomplete but for zlib's single-code case, an end-of-block code)?
//                    One ballot mask per wave and one count per workgroup.
//   k_pd_scan_u32    one workgroup: exclusive scan of those counts.  k_pd_compact: the sorted candidate list (no atomics).
//   k_pd_pass_a      one wave per candidate: Huffman tables in LDS, decode to end-of-block counting only (capped), record
//                    end bit, BFINAL, byte count, validity, and every PD_CK symbols a checkpoint (bit position, bytes so far).
//   k_pd_walk        one wave: the zlib header, then from bit 16 the true chain of blocks.  At a start that is a valid
//                    candidate it jumps to the candidate's end; anywhere else (stored and fixed-Huffman blocks, capped or
//                    missed candidates) it decodes the block itself, exactly.  Gives the true block list and output offsets.
//   k_pd_pass_b      one wave per segment of a true block (PD_CK symbols from a checkpoint, or a whole block the walker
//                    decoded itself): decode again, literals straight into place, copies as source indices
//                    (src[i] = i - dist); a copy from before the stream start is an error.  Bytes past the image are dropped.
//   k_pd_jump        copy resolution by pointer jumping, src[i] = src[src[i]], one launch per round, at most
//                    ceil(log2 n) + 1 rounds, each exits at once when the round before changed nothing.
//   k_pd_resolve     bytes from their sources into rows padded to 16 bytes (and a filter byte per row), Adler-32 partial
//                    sums per workgroup; k_pd_adler combines and checks them.
//   k_pd_unfilter    one workgroup per image: lane i of a wave owns row 64k + i and at step t reconstructs the 16-byte
//                    chunk t - i of a tile of PD_TILE columns, byte by byte in registers; the chunk above comes from lane
//                    i - 1 one step earlier (__shfl_up), the upper-left bytes are the previous ones.  The waves take 64-row
//                    groups in turn; a group waits for the tile above it with a bounded LDS spin (workgroup-scope acquire /
//                    release), never across workgroups.  k_pd_rows drops the padding.
// The extended decoder (lars_d_decode_png_ex: bit depths 1, 2, 4 and 16, Adam7 interlace) shares everything up to k_pd_jump:
// an interlaced file is still one zlib stream.  After it, the layout of the stream comes from lars_png_layout (png_parse.cpp):
//   k_pdx_resolve    as k_pd_resolve, each pass into its own block of padded rows and its own stretch of filter bytes.
//   k_pdx_unfilter   one workgroup per non-empty pass, each with k_pd_unfilter's wavefront and a 64-bit history (bpp to 8).
//   k_pdx_place      one thread per output pixel, along output rows: unpack 1 / 2 / 4 / 8 / 16-bit samples, scale, swap or
//                    narrow them as Pillow does, write to (y0 + r * dy, x0 + c * dx).
// An 8-bit file without interlace takes the kernels above, unchanged, through either entry point.
// Every error is a status code (LARS_PNGD_*) in device memory; every kernel after a failing one returns at once.
#include <string.h>

#include <algorithm>
#include <vector>

#include "checksum_device.h"
#include "codec_host.h"
#include "inflate_device.h"

namespace lars {

#define PD_BATCH 256                   // symbols decoded by the serial lane between two expansions by the whole wave
#define PD_CAP_SYMBOLS (1 << 17)       // pass A gives up after this many symbols (the walker then decodes the block)
#define PD_CK 4096                     // symbols per pass-B segment of a block pass A has checkpointed
#define PD_CKMAX (PD_CAP_SYMBOLS / PD_CK)
#define PD_MARK_THREADS 256
#define PD_TILE 2048                   // unfilter: columns per tile (a multiple of 16)
#define PD_UNF_WAVES 16
#define PD_AHEAD 4                     // unfilter: loads issued this many steps before their use
#define PD_RESOLVE_BYTES 64            // bytes per thread of k_pd_resolve
#define PD_WAIT_TICKS 1000000000ull    // wall-clock ticks (100 MHz) of one bounded unfilter wait: 10 s

struct PdCtl {
    int status[2];
    unsigned int ncand;
    unsigned int nblocks;
    unsigned long long total;          // decoded bytes of the whole stream
    unsigned long long adler_byte;     // stream byte of the Adler-32 trailer
    unsigned int changed[64];          // k_pd_jump: round r changed something
    unsigned long long adler_sums[2];
};

struct PdCand {                        // one block-start candidate
    unsigned long long pos, end, bytes;
    unsigned int valid, final_, nck, pad_;  // nck: checkpoints pass A left (candidates below the slot count only)
};

struct PdCheck {                       // pass A's state after every PD_CK symbols of a block: bit position, bytes so far
    unsigned long long pos, out;
};

struct PdBlock {                       // one segment of a block of the true chain that writes image bytes
    unsigned long long pos;            // the block's header
    unsigned long long start;          // bit to decode from (0: after the header)
    unsigned long long out;            // output byte of that bit
    unsigned int limit, pad_;          // most symbols to decode (0xFFFFFFFF: to end-of-block)
};

__device__ inline void pd_fail(PdCtl *ctl, int code, int detail)
{
    if (atomicCAS(&ctl->status[0], 0, code) == 0) ctl->status[1] = detail;
}

__device__ inline bool pd_failed(const PdCtl *ctl) { return *(volatile const int *)&ctl->status[0] != 0; }

// ---- k_pd_mark: header test at one bit offset, thread-local ---------------------------------------------------------
__device__ bool pd_dynamic_ok(const unsigned int *words, unsigned long long nw, unsigned long long nbits, unsigned long long pos)
{
    if (pos + 17 > nbits) return false;
    {
        // pre-filter on a raw window of at least 97 bits: block type 2, HLIT / HDIST bounds, a complete code-length code
        // (implied by the full test below, which most offsets never reach)
        const unsigned long long wi = pos >> 5;
        const int sh = (int)(pos & 31);
        unsigned long long a = words[wi] | (unsigned long long)words[wi + 1] << 32;
        unsigned long long b = words[wi + 2] | (unsigned long long)words[wi + 3] << 32;
        if (sh) { a = (a >> sh) | (b << (64 - sh)); b >>= sh; }
        if (((a >> 1) & 3) != 2 || ((a >> 3) & 31) > 29 || ((a >> 8) & 31) > 29) return false;
        const int ncode = (int)((a >> 13) & 15) + 4;
        int kraft = 0;
        for (int i = 0; i < ncode; ++i) {
            const int o = 17 + 3 * i;
            const unsigned int len = (unsigned int)((o >= 64 ? (b >> (o - 64)) : o > 61 ? ((a >> o) | (b << (64 - o))) : (a >> o)) & 7);
            if (len) kraft += 128 >> len;
        }
        if (kraft != 128) return false;
    }
    BitReader br;
    br.init(words, nw, pos);
    br.bits(1);
    if (br.bits(2) != 2) return false;
    const int nlen = (int)br.bits(5) + 257, ndist = (int)br.bits(5) + 1, ncode = (int)br.bits(4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    unsigned short cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) cl[c_clorder[i]] = (unsigned short)br.need(3);
    unsigned short count[16], sym[19], offs[16];
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int i = 0; i < 19; ++i) count[cl[i]]++;
    count[0] = 0;
    if (pd_code_check(count, true)) return false;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l];
    for (int s = 0; s < 19; ++s) if (cl[s]) sym[offs[cl[s]]++] = (unsigned short)s;
    unsigned short lcount[16], dcount[16];
    for (int i = 0; i < 16; ++i) { lcount[i] = 0; dcount[i] = 0; }
    int idx = 0, prev = 0, eob = 0;
    const int n = nlen + ndist;
    while (idx < n) {
        br.refill();
        int used = 0;
        const int s = pd_slow_decode(br.buf, count, sym, 7, &used);
        if (s < 0) return false;
        br.bits(used);
        int len, rep;
        if (s < 16) { len = s; rep = 1; }
        else if (s == 16) { if (idx == 0) return false; len = prev; rep = 3 + (int)br.bits(2); }
        else if (s == 17) { len = 0; rep = 3 + (int)br.bits(3); }
        else { len = 0; rep = 11 + (int)br.bits(7); }
        if (idx + rep > n) return false;
        for (int k = 0; k < rep; ++k, ++idx) {
            if (idx < nlen) { lcount[len]++; if (idx == 256) eob = len; }
            else dcount[len]++;
        }
        prev = len;
        if (br.pos() > nbits) return false;
    }
    lcount[0] = 0; dcount[0] = 0;
    return eob != 0 && !pd_code_check(lcount, false) && !pd_code_check(dcount, false);
}

// ---- one block, decoded by a whole wave (blockDim.x == 64) ---------------------------------------------------------
// the bit reader, the constant tables, pd_code_check, pd_slow_decode, the header parser, the first-level tables and pd_symbol
// are inflate_device.h's, shared with the TIFF decoder
struct PdLds : PdCodes {
    unsigned long long rec_o[PD_BATCH];
    unsigned int rec_d[PD_BATCH], rec_l[PD_BATCH];
    // result, written by lane 0
    int done, nrec;
    unsigned long long end, bytes;
};

// lane 0: the block header at pos into L (kind 0 stored, 1 fixed, 2 dynamic; err LARS_PNGD_DEFLATE detail or 0)
__device__ inline void pd_header(PdLds &L, const unsigned int *words, unsigned long long nw, unsigned long long nbits, unsigned long long pos)
{
    pd_header_t<true, false>(L, words, nw, nbits, pos);
}

// The block at pos, by the whole wave.  write: literals into lit[base + k], source indices into src (copies point back),
// nothing at or past `need`.  cap: most symbols before giving up (L.done = 2).  Results in L: err (LARS_PNGD_DEFLATE
// detail, or -1 for a copy from before the stream start), end, bytes, final_, done (1 finished).
__device__ __forceinline__ void pd_block(PdLds &L, const unsigned int *words, unsigned long long nw, unsigned long long nbits, unsigned long long pos,
                         bool write, unsigned long long base, unsigned long long need, uint8_t *lit, int *src, unsigned int cap,
                         unsigned long long start = 0, PdCheck *ckp = nullptr, unsigned int *nck = nullptr)
{
    const int lane = threadIdx.x;
    if (lane == 0) { pd_header(L, words, nw, nbits, pos); L.done = 0; L.bytes = 0; }
    __syncthreads();
    if (L.err) return;
    if (L.kind == 0) {
        const unsigned int n = L.stored_len;
        if (write) {
            const uint8_t *bytes = reinterpret_cast<const uint8_t *>(words) + L.data_pos / 8;
            for (unsigned int k = lane; k < n; k += blockDim.x) {
                const unsigned long long o = base + k;
                if (o < need) { lit[o] = bytes[k]; src[o] = (int)o; }
            }
        }
        __syncthreads();
        if (lane == 0) { L.end = L.data_pos + 8ull * n; L.bytes = n; L.done = 1; }
        __syncthreads();
        return;
    }
    pd_fast_tables(L);
    __syncthreads();
    BitReader br;
    if (lane == 0) br.init(words, nw, start ? start : L.data_pos);
    unsigned long long out = 0;
    unsigned int nsym = 0;
    if (!write) {
        // counting only: one lane, no records, no barriers; the end of the stream and the cap are checked every 256
        // symbols (past the end the reader gives zero bits, and every symbol takes at least one)
        if (lane == 0) {
            int err = 0, done = 0;
            for (;;) {
                br.refill();
                const int s = pd_symbol(br, L.lfast, L.lcnt, L.lsym);
                if (s < 256) {
                    if (s < 0) { err = 4; break; }
                    ++out;
                } else if (s == 256) {
                    done = 1;
                    break;
                } else {
                    const int ls = s - 257;
                    if (ls >= 29) { err = 4; break; }
                    out += c_lbase[ls] + br.bits(c_lext[ls]);
                    br.refill();
                    const int ds = pd_symbol(br, L.dfast, L.dcnt, L.dsym);
                    if (ds < 0 || ds >= 30) { err = 4; break; }
                    br.bits(c_dext[ds]);
                }
                if ((++nsym & 255u) == 0) {
                    if (br.pos() > nbits) { err = 5; break; }
                    if (ckp && (nsym & (PD_CK - 1)) == 0 && nsym <= PD_CAP_SYMBOLS) {
                        ckp[nsym / PD_CK - 1].pos = br.pos();
                        ckp[nsym / PD_CK - 1].out = out;
                    }
                    if (nsym >= cap) { done = 2; break; }
                }
            }
            if (br.pos() > nbits) { err = 5; done = 0; }
            L.err = err; L.done = done; L.end = br.pos(); L.bytes = out;
            if (nck) *nck = min(nsym / PD_CK, (unsigned int)PD_CKMAX);
        }
        __syncthreads();
        return;
    }
    for (;;) {
        if (lane == 0) {
            int nrec = 0;
            while (nrec < PD_BATCH) {
                br.refill();
                const int s = pd_symbol(br, L.lfast, L.lcnt, L.lsym);
                if (s < 0) { L.err = 4; break; }
                if (s < 256) {
                    L.rec_o[nrec] = out; L.rec_d[nrec] = 0; L.rec_l[nrec] = (unsigned int)s; ++nrec;
                    ++out;
                } else if (s == 256) {
                    L.done = 1;
                    break;
                } else {
                    const int ls = s - 257;
                    if (ls >= 29) { L.err = 4; break; }
                    const unsigned int len = c_lbase[ls] + br.bits(c_lext[ls]);
                    br.refill();
                    const int ds = pd_symbol(br, L.dfast, L.dcnt, L.dsym);
                    if (ds < 0 || ds >= 30) { L.err = 4; break; }
                    const unsigned int dist = c_dbase[ds] + br.bits(c_dext[ds]);
                    if (write && dist > base + out) { L.err = -1; break; }
                    L.rec_o[nrec] = out; L.rec_d[nrec] = dist; L.rec_l[nrec] = len; ++nrec;
                    out += len;
                }
                if (br.pos() > nbits) { L.err = 5; break; }
                if (++nsym >= cap) { L.done = 2; break; }
            }
            L.nrec = nrec;
        }
        __syncthreads();
        if (write) {
            const int nrec = L.nrec;
            for (int r = lane; r < nrec; r += blockDim.x) {
                const unsigned long long o = base + L.rec_o[r];
                const unsigned int d = L.rec_d[r];
                if (d == 0) {
                    if (o < need) { lit[o] = (uint8_t)L.rec_l[r]; src[o] = (int)o; }
                } else {
                    const unsigned int len = L.rec_l[r];
                    for (unsigned int k = 0; k < len && o + k < need; ++k) src[o + k] = (int)(o + k - d);
                }
            }
        }
        const bool stop = L.err != 0 || L.done != 0;
        __syncthreads();
        if (stop) break;
    }
    if (lane == 0) { L.end = br.pos(); L.bytes = out; }
    __syncthreads();
}

// one workgroup: off[i] = sum of len[0..i) over the IDAT table { offset, length } pairs
__global__ __launch_bounds__(1024) void k_pd_chunk_scan(const long long *__restrict__ table, long long n,
                                                         unsigned long long *__restrict__ off)
{
    wg_scan_array<unsigned long long>(n, [&](long long i) { return table[2 * i + 1]; }, [&](long long i, unsigned long long before) { off[i] = before; });
}

#define PD_GATHER_THREADS 256

// one workgroup per IDAT chunk (grid-stride): payload into the stream, CRC check
__global__ __launch_bounds__(PD_GATHER_THREADS) void k_pd_gather(const uint8_t *__restrict__ file, const long long *__restrict__ table,
                                                                 long long n, const unsigned long long *__restrict__ off,
                                                                 uint8_t *__restrict__ stream, PdCtl *ctl)
{
    __shared__ unsigned int tab[256];
    __shared__ unsigned int x2n[32];
    __shared__ unsigned int part[PD_GATHER_THREADS / 64];
    const int tid = threadIdx.x;
    crc_table_fill(tab, tid, PD_GATHER_THREADS);
    if (tid == 0) crc_x2n_fill(x2n);
    __syncthreads();
    for (long long k = blockIdx.x; k < n; k += gridDim.x) {
        const unsigned long long src = (unsigned long long)table[2 * k];
        const unsigned int m = (unsigned int)table[2 * k + 1];
        const uint8_t *z = file + src;
        uint8_t *dst = stream + off[k];
        for (unsigned int j = tid; j < m; j += PD_GATHER_THREADS) dst[j] = z[j];
        const unsigned int crc = wg_crc32<PD_GATHER_THREADS>(m + 4u, [&](unsigned int j) { return (unsigned int)z[(long long)j - 4]; },   // z - 4: "IDAT"
                                                             tab, x2n, part);
        if (tid == 0) {
            const uint8_t *c = z + m;
            const unsigned int want = (unsigned int)c[0] << 24 | (unsigned int)c[1] << 16 | (unsigned int)c[2] << 8 | c[3];
            if (crc != want) pd_fail(ctl, LARS_PNGD_CRC, (int)min(k, 0x7FFFFFFFll));
        }
    }
}

// one thread per bit offset: ballot mask per wave, candidate count per workgroup
__global__ __launch_bounds__(PD_MARK_THREADS) void k_pd_mark(const unsigned int *__restrict__ words, unsigned long long nw,
                                                             unsigned long long nbits, unsigned long long *__restrict__ masks,
                                                             unsigned int *__restrict__ wgcnt, const PdCtl *ctl)
{
    __shared__ unsigned int cnt[PD_MARK_THREADS / 64];
    const unsigned long long pos = (unsigned long long)blockIdx.x * PD_MARK_THREADS + threadIdx.x;
    const bool ok = !pd_failed(ctl) && pos >= 16 && pos < nbits && pd_dynamic_ok(words, nw, nbits, pos);
    const unsigned long long m = __ballot(ok);
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
        masks[(unsigned long long)blockIdx.x * (PD_MARK_THREADS / 64) + wave] = m;
        cnt[wave] = (unsigned int)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int s = 0;
        for (int i = 0; i < PD_MARK_THREADS / 64; ++i) s += cnt[i];
        wgcnt[blockIdx.x] = s;
    }
}

// one workgroup: exclusive scan of n counts in place; ctl->ncand = min(total, cap)
__global__ __launch_bounds__(1024) void k_pd_scan_u32(unsigned int *__restrict__ v, long long n, unsigned int cap, PdCtl *ctl)
{
    const unsigned long long total = wg_scan_array<unsigned long long>(
        n, [&](long long i) { return v[i]; }, [&](long long i, unsigned long long before) { v[i] = (unsigned int)min(before, 0xFFFFFFFFull); });
    if (threadIdx.x == 0) ctl->ncand = (unsigned int)min(total, (unsigned long long)cap);
}

__global__ __launch_bounds__(PD_MARK_THREADS) void k_pd_compact(const unsigned long long *__restrict__ masks,
                                                                const unsigned int *__restrict__ wgbase, unsigned int cap,
                                                                PdCand *__restrict__ cands)
{
    const int wave = threadIdx.x / 64, lane = threadIdx.x & 63;
    const unsigned long long *mk = masks + (unsigned long long)blockIdx.x * (PD_MARK_THREADS / 64);
    const unsigned long long m = mk[wave];
    if (!((m >> lane) & 1ull)) return;
    unsigned long long idx = wgbase[blockIdx.x];
    for (int i = 0; i < wave; ++i) idx += (unsigned long long)__popcll(mk[i]);
    idx += (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (idx < cap) cands[idx].pos = (unsigned long long)blockIdx.x * PD_MARK_THREADS + threadIdx.x;
}

// one wave per candidate (grid-stride): counting decode, capped
__global__ __launch_bounds__(64) void k_pd_pass_a(const unsigned int *__restrict__ words, unsigned long long nw,
                                                  unsigned long long nbits, PdCand *__restrict__ cands, PdCheck *__restrict__ checks,
                                                  unsigned int nslot, const PdCtl *ctl)
{
    __shared__ PdLds L;
    __shared__ unsigned int nck;
    if (pd_failed(ctl)) return;
    const unsigned int n = ctl->ncand;
    for (unsigned int c = blockIdx.x; c < n; c += gridDim.x) {
        const unsigned long long pos = cands[c].pos;
        if (threadIdx.x == 0) nck = 0;
        pd_block(L, words, nw, nbits, pos, false, 0, 0, nullptr, nullptr, PD_CAP_SYMBOLS, 0,
                 c < nslot ? checks + (unsigned long long)c * PD_CKMAX : nullptr, c < nslot ? &nck : nullptr);
        if (threadIdx.x == 0) {
            PdCand r;
            r.pos = pos;
            r.valid = L.err == 0 && L.done == 1;
            r.end = L.end;
            r.bytes = L.bytes;
            r.final_ = (unsigned int)L.final_;
            r.nck = L.kind == 0 ? 0u : nck;
            r.pad_ = 0;
            cands[c] = r;
        }
        __syncthreads();
    }
}

// one wave: the zlib header, then the exact chain of blocks
__global__ __launch_bounds__(64) void k_pd_walk(const unsigned int *__restrict__ words, unsigned long long nw, unsigned long long nbits,
                                                const PdCand *__restrict__ cands, const PdCheck *__restrict__ checks,
                                                unsigned int nslot, PdBlock *__restrict__ blocks, unsigned int block_cap,
                                                unsigned long long need, PdCtl *ctl)
{
    __shared__ PdLds L;
    __shared__ int stop;
    __shared__ unsigned long long s_pos, s_out;
    __shared__ unsigned int s_nb;
    __shared__ int s_hit;
    __shared__ unsigned int s_ci;
    __shared__ PdCand s_c;
    const int lane = threadIdx.x;
    if (pd_failed(ctl)) return;
    if (lane == 0) {
        const uint8_t *b = reinterpret_cast<const uint8_t *>(words);
        const unsigned int cmf = b[0], flg = b[1];
        stop = 0;
        if (nbits < 16 || (cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) {
            pd_fail(ctl, LARS_PNGD_ZLIB_HEADER, nbits < 16 ? -1 : (int)((cmf << 8) | flg));
            stop = 1;
        }
        s_pos = 16; s_out = 0; s_nb = 0;
    }
    __syncthreads();
    if (stop) return;
    const unsigned int ncand = ctl->ncand;
    for (;;) {
        if (lane == 0) {
            // binary search of the sorted candidate list
            unsigned int lo = 0, hi = ncand;
            while (lo < hi) {
                const unsigned int mid = (lo + hi) / 2;
                if (cands[mid].pos < s_pos) lo = mid + 1; else hi = mid;
            }
            s_hit = lo < ncand && cands[lo].pos == s_pos && cands[lo].valid;
            if (s_hit) { s_c = cands[lo]; s_ci = lo; }
        }
        __syncthreads();
        unsigned long long end, bytes;
        int fin;
        if (s_hit) {
            end = s_c.end; bytes = s_c.bytes; fin = (int)s_c.final_;
        } else {
            pd_block(L, words, nw, nbits, s_pos, false, 0, 0, nullptr, nullptr, 0xFFFFFFFFu);
            if (L.err) {
                if (lane == 0) pd_fail(ctl, LARS_PNGD_DEFLATE, L.err);
                return;
            }
            end = L.end; bytes = L.bytes; fin = L.final_;
        }
        if (lane == 0) {
            if (bytes && s_out < need) {
                // a checkpointed block becomes nck + 1 segments of PD_CK symbols; any other block one segment
                const unsigned int nck = (s_hit && s_ci < nslot) ? s_c.nck : 0u;
                if (s_nb + nck + 1 > block_cap) { pd_fail(ctl, LARS_PNGD_INTERNAL, 1); stop = 1; }
                else {
                    PdBlock sg;
                    sg.pos = s_pos; sg.start = 0; sg.out = s_out; sg.limit = nck ? PD_CK : 0xFFFFFFFFu; sg.pad_ = 0;
                    blocks[s_nb++] = sg;
                    for (unsigned int i = 1; i <= nck; ++i) {
                        const PdCheck ck = checks[(unsigned long long)s_ci * PD_CKMAX + i - 1];
                        if (s_out + ck.out >= need) break;
                        sg.start = ck.pos; sg.out = s_out + ck.out; sg.limit = i == nck ? 0xFFFFFFFFu : PD_CK;
                        blocks[s_nb++] = sg;
                    }
                }
            }
            s_out += bytes;
            s_pos = end;
            if (fin) stop = stop ? stop : 2;
        }
        __syncthreads();
        if (stop) break;
    }
    if (lane == 0 && stop == 2) {
        ctl->nblocks = s_nb;
        ctl->total = s_out;
        ctl->adler_byte = (s_pos + 7) / 8;
        // too few bytes is reported by k_pd_jump, after pass B had the chance to find a bad distance (zlib's order)
        if (s_out == need && ctl->adler_byte + 4 > nbits / 8) pd_fail(ctl, LARS_PNGD_DEFLATE, 5);
    }
}

// one wave per segment of a true block (grid-stride): literals into place, copies as source indices
__global__ __launch_bounds__(64) void k_pd_pass_b(const unsigned int *__restrict__ words, unsigned long long nw, unsigned long long nbits,
                                                  const PdBlock *__restrict__ blocks, unsigned long long need, uint8_t *__restrict__ lit,
                                                  int *__restrict__ src, PdCtl *ctl)
{
    __shared__ PdLds L;
    if (pd_failed(ctl)) return;
    const unsigned int n = ctl->nblocks;
    for (unsigned int b = blockIdx.x; b < n; b += gridDim.x) {
        const PdBlock blk = blocks[b];
        pd_block(L, words, nw, nbits, blk.pos, true, blk.out, need, lit, src, blk.limit, blk.start);
        if (threadIdx.x == 0 && L.err)
            pd_fail(ctl, L.err < 0 ? LARS_PNGD_FAR : LARS_PNGD_DEFLATE, L.err < 0 ? (int)(blk.out & 0x7FFFFFFF) : L.err);
        __syncthreads();
    }
}

// one round of pointer jumping (in place: a source read mid-round is older or newer, both lie on the same chain)
__global__ __launch_bounds__(256) void k_pd_jump(int *__restrict__ src, long long n, int round, PdCtl *ctl)
{
    if (pd_failed(ctl) || (round > 0 && *(volatile unsigned int *)&ctl->changed[round - 1] == 0)) return;
    if (ctl->total < (unsigned long long)n) {
        if (blockIdx.x == 0 && threadIdx.x == 0) pd_fail(ctl, LARS_PNGD_SHORT, (int)min(ctl->total, 0x7FFFFFFFull));
        return;
    }
    bool ch = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int s = src[i];
        if (s == (int)i) continue;
        if (s < 0 || (long long)s > i) { pd_fail(ctl, LARS_PNGD_INTERNAL, 2); return; }
        const int t = src[s];
        if (t != s) { src[i] = t; ch = true; }
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) ctl->changed[round] = 1u;
}

// byte i of the stream from its source (a source is always a literal)
__device__ inline unsigned int pd_source_byte(const uint8_t *__restrict__ lit, const int *__restrict__ src, long long i, PdCtl *ctl)
{
    const int s = src[i];
    if (s == (int)i) return lit[i];
    if (s >= 0 && (long long)s < i) return lit[s];
    pd_fail(ctl, LARS_PNGD_INTERNAL, 3);
    return 0u;
}

// a workgroup's Adler-32 partial sums (of 256 threads) -> parts[2 * blockIdx.x ..]
__device__ inline void pd_adler_parts(unsigned long long s1, unsigned long long s2, unsigned long long *s_w, unsigned long long *__restrict__ parts)
{
    adler_wg<256>(s1, s2, s_w);
    if (threadIdx.x == 0) { parts[2 * blockIdx.x] = s1; parts[2 * blockIdx.x + 1] = s2; }
}

// bytes from their sources, into rows padded to rbp bytes and a filter byte per row; Adler-32 partial sums
__global__ __launch_bounds__(256) void k_pd_resolve(const uint8_t *__restrict__ lit, const int *__restrict__ src, long long n,
                                                    unsigned int rb, unsigned int rbp, uint8_t *__restrict__ fpad,
                                                    uint8_t *__restrict__ ftype, unsigned long long *__restrict__ parts, PdCtl *ctl)
{
    __shared__ unsigned long long s_w[8];
    if (pd_failed(ctl)) return;
    const long long lo = ((long long)blockIdx.x * 256 + threadIdx.x) * PD_RESOLVE_BYTES, hi = min(n, lo + PD_RESOLVE_BYTES);
    unsigned long long s1 = 0, s2 = 0;
    for (long long i = lo; i < hi; ++i) {
        const unsigned int v = pd_source_byte(lit, src, i, ctl);
        const unsigned int r = (unsigned int)i / (rb + 1u), col = (unsigned int)i - r * (rb + 1u);
        if (col == 0) ftype[r] = (uint8_t)v;
        else fpad[(unsigned long long)r * rbp + col - 1] = (uint8_t)v;
        s1 += v;
        s2 += (unsigned long long)(n - i) * v;
    }
    pd_adler_parts(s1, s2, s_w, parts);
}

// one workgroup: the Adler-32 of the partial sums (checksum_device.h) against the trailer
__global__ __launch_bounds__(256) void k_pd_adler(const unsigned long long *__restrict__ parts, long long nparts, long long n,
                                                  const uint8_t *__restrict__ stream, PdCtl *ctl)
{
    __shared__ unsigned long long s_w[8];
    if (pd_failed(ctl)) return;
    unsigned long long s1 = 0, s2 = 0;
    for (long long i = threadIdx.x; i < nparts; i += 256) { s1 += parts[2 * i]; s2 += parts[2 * i + 1]; }
    adler_wg<256>(s1, s2, s_w);
    if (threadIdx.x == 0 && ctl->total == (unsigned long long)n) {        // more data than the image: not checked
        const uint8_t *t = stream + ctl->adler_byte;
        const unsigned int want = (unsigned int)t[0] << 24 | (unsigned int)t[1] << 16 | (unsigned int)t[2] << 8 | t[3];
        if (adler_value(s1, s2, (unsigned long long)n) != want) pd_fail(ctl, LARS_PNGD_ADLER, 0);
    }
}

__device__ __forceinline__ unsigned int pd_recon(int f, unsigned int x, unsigned int a, unsigned int b, unsigned int c)
{
    switch (f) {
    case 1: return (x + a) & 255u;
    case 2: return (x + b) & 255u;
    case 3: return (x + ((a + b) >> 1)) & 255u;
    case 4: {
        const int p = (int)a + (int)b - (int)c;
        const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
        return (x + ((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c))) & 255u;
    }
    default: return x;
    }
}

__device__ __forceinline__ unsigned int pd_byte(const uint4 &v, int k)          // k: a compile-time constant after unrolling
{
    const unsigned int d = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w;
    return (d >> (8 * (k & 3))) & 255u;
}

__device__ __forceinline__ uint4 pd_shfl_up(const uint4 &v)
{
    return make_uint4(__shfl_up(v.x, 1, 64), __shfl_up(v.y, 1, 64), __shfl_up(v.z, 1, 64), __shfl_up(v.w, 1, 64));
}

// one workgroup of PD_UNF_WAVES waves: the skewed wavefront (see the top of the file), 16 bytes per lane and step.  Rows are
// padded to rbp (a multiple of 16) bytes in fpad and opad; lane i of a wave reconstructs chunk t - i of its row at step t.
// HIST holds the last bpp bytes of the row and of the row above: 32 bits reach bpp 4, 64 bits bpp 8 (16-bit RGBA).
// filter_detail(row): what a bad filter byte reports.  The bounded wait is workgroup-scope; nothing waits across workgroups.
template <typename HIST, typename Detail>
__device__ __forceinline__ void pd_unfilter_rows(const uint8_t *__restrict__ fpad, const uint8_t *__restrict__ ftype, long long h,
                                                 long long rbp, int bpp, uint8_t *__restrict__ opad, PdCtl *ctl, Detail filter_detail)
{
    __shared__ unsigned int prog[PD_UNF_WAVES];
    __shared__ int abort_;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64, nwaves = blockDim.x / 64;
    if (threadIdx.x < PD_UNF_WAVES) prog[threadIdx.x] = 0;
    if (threadIdx.x == 0) abort_ = 0;
    __syncthreads();
    if (pd_failed(ctl)) return;
    const long long nchunk = rbp / 16, ngroups = (h + 63) / 64, tchunks = PD_TILE / 16, ncb = (nchunk + tchunks - 1) / tchunks;
    const int sh = 8 * (bpp - 1);
    for (long long g = wave; g < ngroups; g += nwaves) {
        const long long row = g * 64 + lane;
        const bool active = row < h;
        int f = active ? ftype[row] : 0;
        if (f > 4) { pd_fail(ctl, LARS_PNGD_FILTER, filter_detail(row)); f = 0; }
        const uint4 *xrow = reinterpret_cast<const uint4 *>(fpad + row * rbp);
        uint4 *orow = reinterpret_cast<uint4 *>(opad + row * rbp);
        const uint4 *uprow = reinterpret_cast<const uint4 *>(opad + (row - 1) * rbp);
        HIST ha = 0, hc = 0;
        uint4 prev = make_uint4(0u, 0u, 0u, 0u);
        for (long long cb = 0; cb < ncb; ++cb) {
            if (g > 0) {
                // the tile above: group g - 1, tile cb, finished by wave (g - 1) % nwaves
                const unsigned int want = (unsigned int)((g - 1) * ncb + cb + 1);
                const unsigned int *p = &prog[(g - 1) % nwaves];
                const unsigned long long t0 = wall_clock64();
                while (__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < want) {
                    if (__hip_atomic_load(&abort_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
                    if (wall_clock64() - t0 > PD_WAIT_TICKS) {
                        if (lane == 0) {
                            pd_fail(ctl, LARS_PNGD_INTERNAL, 4);
                            __hip_atomic_store(&abort_, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        return;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
            }
            const long long k0 = cb * tchunks, k1 = min(nchunk, k0 + tchunks);
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            // loads run PD_AHEAD steps ahead of their use (a ring of registers, indexed by constants after unrolling)
            uint4 xr[PD_AHEAD], ur[PD_AHEAD];
#pragma unroll
            for (int q = 0; q < PD_AHEAD; ++q) {
                const long long kq = k0 + q - lane;
                const bool vq = active && kq >= k0 && kq < k1;
                xr[q] = vq ? xrow[kq] : zero;
                ur[q] = (vq && lane == 0 && row > 0) ? uprow[kq] : zero;
            }
            const long long steps = (k1 - k0) + 63;
            for (long long t = 0; t < steps; t += PD_AHEAD) {
#pragma unroll
                for (int q = 0; q < PD_AHEAD; ++q) {
                    const long long k = k0 + t + q - lane;
                    const bool v = active && k >= k0 && k < k1;
                    const uint4 x = xr[q], u0 = ur[q];
                    const long long kf = k + PD_AHEAD;
                    const bool vf = active && kf >= k0 && kf < k1;
                    xr[q] = vf ? xrow[kf] : zero;
                    ur[q] = (vf && lane == 0 && row > 0) ? uprow[kf] : zero;
                    const uint4 fromleft = pd_shfl_up(prev);   // lane - 1's chunk k of the row above, made one step earlier
                    const uint4 up = lane == 0 ? u0 : fromleft;
                    if (v) {
                        unsigned int o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const unsigned int bb = pd_byte(up, j);
                            const unsigned int a = (unsigned int)(ha >> sh) & 255u, c = (unsigned int)(hc >> sh) & 255u;
                            const unsigned int r = pd_recon(f, pd_byte(x, j), a, bb, c);
                            ha = (ha << 8) | r;
                            hc = (hc << 8) | bb;
                            o[j >> 2] |= r << (8 * (j & 3));
                        }
                        prev = make_uint4(o[0], o[1], o[2], o[3]);
                        orow[k] = prev;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&prog[wave], (unsigned int)(g * ncb + cb + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

__global__ __launch_bounds__(64 * PD_UNF_WAVES) void k_pd_unfilter(const uint8_t *__restrict__ fpad, const uint8_t *__restrict__ ftype,
                                                                   long long h, long long rbp, int bpp, uint8_t *__restrict__ opad,
                                                                   PdCtl *ctl)
{
    pd_unfilter_rows<unsigned int>(fpad, ftype, h, rbp, bpp, opad, ctl, [](long long row) { return (int)min(row, 0x7FFFFFFFll); });
}

// padded rows -> [h][rb]
__global__ __launch_bounds__(256) void k_pd_rows(const uint8_t *__restrict__ opad, long long h, long long rb, long long rbp,
                                                 uint8_t *__restrict__ out, const PdCtl *ctl)
{
    if (pd_failed(ctl)) return;
    const long long n = h * rb;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / rb;
        out[i] = opad[r * rbp + (i - r * rb)];
    }
}

// ---- the extended decoder: rows per pass, any bit depth --------------------------------------------------------------
// What the kernels after the stream know of a file, passed by value.  Every pass has its own block of 16-byte-padded rows
// in fpad / opad (pad_base) and its own stretch of filter bytes (row_base).
struct PdxPass {
    unsigned int off, rb, rbp, ph;      // first stream byte, row bytes, padded row bytes, rows
    unsigned int x0, y0, ldx, ldy;      // first column and row, log2 of the column and row step
    unsigned long long pad_base, row_base;
    int index;                          // Adam7 pass number 1..7, 0 without interlace
    unsigned int pw;                    // columns
};
#define PDX_SUB 0                       // 1, 2, 4 bits: one byte per sample, times mult
#define PDX_BYTES 1                     // 8 bits: the pixel's bytes
#define PDX_GRAY16 2                    // native-endian uint16
#define PDX_HIGH 3                      // 16 bits: the high byte of every sample
#define PDX_LA16 4                      // 16-bit LA: L, L, L, A of the high bytes
struct PdxDev {
    int npass, interlace, depth, inc;   // inc: samples per pixel in the file
    int kind, mult, bpp, pad_;
    int slot[8];                        // Adam7 pass number -> position in p, -1 for an empty pass
    PdxPass p[7];
};

// k_pd_resolve with rows of a length per pass: each thread finds the pass, row and column of its first byte once and
// steps from there
__global__ __launch_bounds__(256) void k_pdx_resolve(const uint8_t *__restrict__ lit, const int *__restrict__ src, long long n,
                                                     const PdxDev D, uint8_t *__restrict__ fpad, uint8_t *__restrict__ ftype,
                                                     unsigned long long *__restrict__ parts, PdCtl *ctl)
{
    __shared__ unsigned long long s_w[8];
    if (pd_failed(ctl)) return;
    const long long lo = ((long long)blockIdx.x * 256 + threadIdx.x) * PD_RESOLVE_BYTES, hi = min(n, lo + PD_RESOLVE_BYTES);
    unsigned long long s1 = 0, s2 = 0;
    if (lo < hi) {
        int p = 0;
        while (p + 1 < D.npass && (unsigned int)lo >= D.p[p + 1].off) ++p;
        PdxPass P = D.p[p];
        long long end = p + 1 < D.npass ? (long long)D.p[p + 1].off : n;
        unsigned int r = ((unsigned int)lo - P.off) / (P.rb + 1u), col = ((unsigned int)lo - P.off) - r * (P.rb + 1u);
        for (long long i = lo; i < hi; ++i) {
            if (i == end) {
                ++p;
                if (p >= D.npass) break;                 // cannot happen: the passes cover [0, n)
                P = D.p[p];
                end = p + 1 < D.npass ? (long long)D.p[p + 1].off : n;
                r = 0; col = 0;
            }
            const unsigned int v = pd_source_byte(lit, src, i, ctl);
            if (r < P.ph) {
                if (col == 0) ftype[P.row_base + r] = (uint8_t)v;
                else fpad[P.pad_base + (unsigned long long)r * P.rbp + col - 1] = (uint8_t)v;
            }
            if (++col > P.rb) { col = 0; ++r; }
            s1 += v;
            s2 += (unsigned long long)(n - i) * v;
        }
    }
    pd_adler_parts(s1, s2, s_w, parts);
}

// one workgroup per pass: the passes are independent pictures, each unfiltered by pd_unfilter_rows with a 64-bit history.  Waves
// a small pass has no 64-row group for do nothing.  A bad filter byte reports pass << 24 | row within the pass.
__global__ __launch_bounds__(64 * PD_UNF_WAVES) void k_pdx_unfilter(const uint8_t *__restrict__ fpad, const uint8_t *__restrict__ ftype,
                                                                    const PdxDev D, uint8_t *__restrict__ opad, PdCtl *ctl)
{
    if ((int)blockIdx.x >= D.npass) return;                // uniform: the whole workgroup leaves
    const PdxPass P = D.p[blockIdx.x];
    pd_unfilter_rows<unsigned long long>(fpad + P.pad_base, ftype + P.row_base, (long long)P.ph, (long long)P.rbp, D.bpp, opad + P.pad_base, ctl,
                                         [&](long long row) { return P.index << 24 | (int)min(row, 0xFFFFFFll); });
}

// unfiltered pass rows -> the array Pillow gives.  One thread per output pixel, a workgroup along an output row, so the
// stores of a row are contiguous whatever pass its pixels come from (the odd rows, half the picture, are pass 7 alone and
// read contiguously too).
__global__ __launch_bounds__(256) void k_pdx_place(const uint8_t *__restrict__ opad, const PdxDev D, long long h, long long w,
                                                   uint8_t *__restrict__ out, const PdCtl *ctl)
{
    if (pd_failed(ctl)) return;
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    for (long long y = blockIdx.y; y < h; y += gridDim.y) {
        int pn = 0;
        if (D.interlace) pn = (y & 1) ? 7 : (x & 1) ? 6 : (y & 2) ? 5 : (x & 2) ? 4 : (y & 4) ? 3 : (x & 4) ? 2 : 1;
        const int slot = D.slot[pn];
        if (slot < 0 || slot >= D.npass) continue;      // cannot happen: a pass that holds a pixel is not empty
        const PdxPass P = D.p[slot];
        const unsigned int r = ((unsigned int)y - P.y0) >> P.ldy, c = ((unsigned int)x - P.x0) >> P.ldx;
        if (r >= P.ph || c >= P.pw) continue;
        const uint8_t *row = opad + P.pad_base + (unsigned long long)r * P.rbp;
        const unsigned long long px = (unsigned long long)y * w + x;
        switch (D.kind) {
        case PDX_SUB: {
            const unsigned int bit = c * D.depth;        // < 2^24 * 4
            const unsigned int v = (row[bit >> 3] >> (8 - D.depth - (bit & 7u))) & ((1u << D.depth) - 1u);
            out[px] = (uint8_t)(v * D.mult);
            break;
        }
        case PDX_BYTES:
            for (int k = 0; k < D.inc; ++k) out[px * D.inc + k] = row[(unsigned long long)c * D.inc + k];
            break;
        case PDX_GRAY16:
            reinterpret_cast<unsigned short *>(out)[px] = (unsigned short)(row[2ull * c] << 8 | row[2ull * c + 1]);
            break;
        case PDX_HIGH:
            for (int k = 0; k < D.inc; ++k) out[px * D.inc + k] = row[2ull * ((unsigned long long)c * D.inc + k)];
            break;
        default: {                                       // PDX_LA16
            const unsigned int l = row[4ull * c], a = row[4ull * c + 2];
            reinterpret_cast<unsigned int *>(out)[px] = l | l << 8 | l << 16 | a << 24;
            break;
        }
        }
    }
}

// sizes and the device scratch of one file: what lars_png_decode_scratch_bytes counts and lars_d_decode_png_u8 points into
struct PdPlan {
    unsigned long long nbits, nw, nmark, ncap, bcap, need, nparts, rbp, nslot;
    PdCtl *ctl;
    unsigned long long *off, *masks, *parts;
    unsigned int *words, *wgcnt;
    PdCand *cands;
    PdCheck *checks;
    PdBlock *blocks;
    uint8_t *lit, *fpad, *ftype, *opad;
    int *src;
};

static bool pd_shape_ok(int64_t h, int64_t w, int channels)
{
    if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24) || channels < 1 || channels > 4) return false;
    return (unsigned long long)h * (1ull + (unsigned long long)w * channels) <= 0x7FFFFFFFull;
}

// the stream's part of a plan: everything up to the resolved bytes, for a filtered stream of `need` bytes
static void pd_plan_stream(PdPlan &P, unsigned long long need, int64_t idat_bytes, int64_t idat_count, Carver &cv)
{
    P.need = need;
    P.nbits = (unsigned long long)idat_bytes * 8;
    P.nw = (((unsigned long long)idat_bytes + 3) / 4 + 4 + 3) & ~3ull;   // whole quads, at least 4 zero words
    P.nmark = (P.nbits + PD_MARK_THREADS - 1) / PD_MARK_THREADS;
    P.ncap = P.nbits / 64 + 256;
    // segments: at most one per block that writes image bytes, plus one per checkpoint
    P.bcap = std::min(P.nbits / 18, P.need) + 2 + P.need / PD_CK + PD_CKMAX;
    P.nslot = std::min(P.ncap, P.nbits / 4096 + 256);   // candidates that keep checkpoints (the rest: one segment per block)
    P.nparts = (P.need + 256ull * PD_RESOLVE_BYTES - 1) / (256ull * PD_RESOLVE_BYTES);
    P.ctl = cv.take<PdCtl>(1);
    P.off = cv.take<unsigned long long>((size_t)idat_count);
    P.words = cv.take<unsigned int>(P.nw);
    P.masks = cv.take<unsigned long long>(P.nmark * (PD_MARK_THREADS / 64));
    P.wgcnt = cv.take<unsigned int>(P.nmark);
    P.cands = cv.take<PdCand>(P.ncap);
    P.checks = cv.take<PdCheck>(P.nslot * PD_CKMAX);
    P.blocks = cv.take<PdBlock>(P.bcap);
    P.lit = cv.take<uint8_t>(P.need);
    P.src = cv.take<int>(P.need);
    P.parts = cv.take<unsigned long long>(P.nparts * 2);
}

static PdPlan pd_plan(int64_t h, int64_t w, int channels, int64_t idat_bytes, int64_t idat_count, Carver &cv)
{
    PdPlan P{};
    pd_plan_stream(P, (unsigned long long)h * (1ull + (unsigned long long)w * channels), idat_bytes, idat_count, cv);
    P.rbp = ((unsigned long long)w * channels + 15) & ~15ull;
    P.fpad = cv.take<uint8_t>((size_t)h * P.rbp);
    P.ftype = cv.take<uint8_t>((size_t)h);
    P.opad = cv.take<uint8_t>((size_t)h * P.rbp);
    return P;
}

// the extended decoder's plan: the layout of the file (lars_png_layout) as the kernels take it, and the scratch
struct PdxPlan {
    PdPlan P;
    PdxDev D;
    unsigned long long pad_bytes, rows;  // all passes: padded row bytes, rows
    long long max_groups;                // 64-row groups of the tallest pass
    int channels, itemsize;              // of the array
    bool plain;                          // 8 bits, no interlace: lars_d_decode_png_u8's path
};

static bool pdx_layout(int64_t h, int64_t w, int depth, int ctype, int interlace, PdxPlan &X)
{
    int64_t passes[7 * LARS_PNGX_PASS_N], npass = 0, need = 0;
    if (h < 1 || w < 1 || h > (1 << 24) || w > (1 << 24)) return false;
    if (lars_png_out_format(depth, ctype, &X.channels, &X.itemsize) != LARS_OK) return false;
    if (lars_png_layout(w, h, depth, ctype, interlace, passes, &npass, &need) != LARS_OK) return false;
    if (npass < 1 || npass > 7 || need < 1 || need > 0x7FFFFFFFll) return false;
    PdxDev &D = X.D;
    memset(&D, 0, sizeof D);
    static const int chans[7] = {1, 0, 3, 1, 2, 0, 4};
    D.npass = (int)npass; D.interlace = interlace; D.depth = depth; D.inc = chans[ctype];
    D.kind = depth < 8 ? PDX_SUB : depth == 8 ? PDX_BYTES : ctype == 0 ? PDX_GRAY16 : ctype == 4 ? PDX_LA16 : PDX_HIGH;
    D.mult = (ctype == 0 && depth > 1 && depth < 8) ? 255 / ((1 << depth) - 1) : 1;
    for (int k = 0; k < 8; ++k) D.slot[k] = -1;
    X.pad_bytes = 0; X.rows = 0; X.max_groups = 0;
    for (int k = 0; k < D.npass; ++k) {
        const int64_t *q = passes + k * LARS_PNGX_PASS_N;
        PdxPass &p = D.p[k];
        p.off = (unsigned int)q[LARS_PNGX_PASS_OFFSET];
        p.rb = (unsigned int)q[LARS_PNGX_PASS_ROW_BYTES];
        p.rbp = (p.rb + 15u) & ~15u;
        p.ph = (unsigned int)q[LARS_PNGX_PASS_H]; p.pw = (unsigned int)q[LARS_PNGX_PASS_W];
        p.x0 = (unsigned int)q[LARS_PNGX_PASS_X0]; p.y0 = (unsigned int)q[LARS_PNGX_PASS_Y0];
        p.ldx = 0; p.ldy = 0;
        while ((1ll << p.ldx) < q[LARS_PNGX_PASS_DX]) ++p.ldx;
        while ((1ll << p.ldy) < q[LARS_PNGX_PASS_DY]) ++p.ldy;
        p.pad_base = X.pad_bytes; p.row_base = X.rows;
        p.index = (int)q[LARS_PNGX_PASS_INDEX];
        D.bpp = (int)q[LARS_PNGX_PASS_BPP];
        D.slot[p.index] = k;
        X.pad_bytes += (unsigned long long)p.ph * p.rbp;
        X.rows += p.ph;
        X.max_groups = std::max<long long>(X.max_groups, ((long long)p.ph + 63) / 64);
    }
    X.P.need = (unsigned long long)need;
    X.plain = depth == 8 && !interlace;
    return true;
}

static void pdx_plan(PdxPlan &X, int64_t idat_bytes, int64_t idat_count, Carver &cv)
{
    pd_plan_stream(X.P, X.P.need, idat_bytes, idat_count, cv);
    X.P.fpad = cv.take<uint8_t>((size_t)X.pad_bytes);
    X.P.ftype = cv.take<uint8_t>((size_t)X.rows);
    X.P.opad = cv.take<uint8_t>((size_t)X.pad_bytes);
}

static const char *pd_deflate_what(int d)
{
    switch (d) {
    case 1: return "invalid block type";
    case 2: return "stored block length does not match its complement";
    case 3: return "invalid code lengths";
    case 4: return "invalid code";
    case 5: return "stream truncated";
    default: return "error";
    }
}

// the message of a device status
static int pd_status_fail(const char *who, const int st[2], bool ex = false)
{
    switch (st[0]) {
    case LARS_PNGD_CRC: return fail(LARS_ERR_INVALID, "%s: bad CRC in IDAT chunk %d", who, st[1]);
    case LARS_PNGD_ZLIB_HEADER: return fail(LARS_ERR_INVALID, "%s: bad zlib header (CMF/FLG %#06x%s)", who, st[1],
                                             st[1] >= 0 && (st[1] & 32) ? ", preset dictionary" : "");
    case LARS_PNGD_DEFLATE: return fail(LARS_ERR_INVALID, "%s: deflate error: %s", who, pd_deflate_what(st[1]));
    case LARS_PNGD_FAR: return fail(LARS_ERR_INVALID, "%s: deflate error: copy distance too far back (block at output byte %d)", who, st[1]);
    case LARS_PNGD_SHORT: return fail(LARS_ERR_INVALID, "%s: too few decoded bytes (%d)", who, st[1]);
    case LARS_PNGD_ADLER: return fail(LARS_ERR_INVALID, "%s: Adler-32 mismatch", who);
    case LARS_PNGD_FILTER:
        if (ex && (st[1] >> 24)) return fail(LARS_ERR_INVALID, "%s: bad filter byte in row %d of pass %d", who, st[1] & 0xFFFFFF, st[1] >> 24);
        return fail(LARS_ERR_INVALID, "%s: bad filter byte in row %d", who, ex ? st[1] & 0xFFFFFF : st[1]);
    default: return fail(LARS_ERR_HIP, "%s: internal decoder status %d (%d)", who, st[0], st[1]);
    }
}

// the PNG side of the host entry points (codec_host.h)
struct PdFile : HostFile {
    int64_t ctype, idat_bytes, nidat;
    int depth, interlace;
    bool ex;                                              // the extended decoder: every IHDR combination but APNG
    std::vector<int64_t> table;

    // parse + checks shared by the host entry points
    int parse(const char *who_, const uint8_t *file_, int64_t len_, bool ex_ = false)
    {
        who = who_; file = file_; len = len_; ex = ex_;
        if (!file || len <= 0) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
        int64_t info[LARS_PNG_INFO_N];
        LARS_TRY(lars_png_info(file, len, info, nullptr, 0));
        h = info[LARS_PNG_INFO_HEIGHT]; w = info[LARS_PNG_INFO_WIDTH]; channels = (int)info[LARS_PNG_INFO_CHANNELS];
        ctype = info[LARS_PNG_INFO_COLOR_TYPE]; idat_bytes = info[LARS_PNG_INFO_IDAT_BYTES]; nidat = info[LARS_PNG_INFO_IDAT_COUNT];
        const long long d = info[LARS_PNG_INFO_BIT_DEPTH], il = info[LARS_PNG_INFO_INTERLACE];
        depth = (int)d; interlace = (int)il;
        if (ex ? info[LARS_PNG_INFO_APNG] != 0 : !info[LARS_PNG_INFO_SUPPORTED])
            return fail(LARS_ERR_UNSUPPORTED, "%s: %s PNG (bit depth %lld, interlace %lld) is not supported", who,
                        info[LARS_PNG_INFO_APNG] ? "APNG" : il ? "interlaced" : "this", d, il);
        if (ex) {
            PdxPlan X{};
            if (!pdx_layout(h, w, depth, (int)ctype, interlace, X))
                return fail(LARS_ERR_INVALID, "%s: %lld x %lld picture (bit depth %lld, colour type %lld) is too large", who, (long long)h,
                            (long long)w, d, (long long)ctype);
            channels = X.channels; sample_bytes = X.itemsize;
            scratch_bytes = lars_png_decode_ex_scratch_bytes(h, w, depth, (int)ctype, interlace, idat_bytes, nidat);
        } else {
            if (!pd_shape_ok(h, w, channels))
                return fail(LARS_ERR_INVALID, "%s: %lld x %lld x %lld picture is too large", who, (long long)h, (long long)w, (long long)channels);
            scratch_bytes = lars_png_decode_scratch_bytes(h, w, channels, idat_bytes, nidat);
        }
        extra_bytes = (size_t)nidat * 16;                 // the IDAT table
        table.assign((size_t)nidat * 2, 0);
        return lars_png_info(file, len, info, table.data(), nidat);
    }
    int enqueue(hipStream_t s)
    {
        int64_t *d_tab = static_cast<int64_t *>(d_extra);
        LARS_HIP_TRY(hipMemcpyAsync(d_tab, table.data(), extra_bytes, hipMemcpyHostToDevice, s));
        if (ex) return lars_d_decode_png_ex(d_file, d_tab, nidat, idat_bytes, h, w, depth, (int)ctype, interlace, d_img, d_status, d_scratch, s);
        return lars_d_decode_png_u8(d_file, d_tab, nidat, idat_bytes, h, w, channels, d_img, d_status, d_scratch, s);
    }
    int finish(const int st[2]) { return st[0] ? pd_status_fail(who, st, ex && !(depth == 8 && !interlace)) : LARS_OK; }
};

// the stream's kernels, shared by both decoders: IDAT payloads to the stream's bytes and the source index of each
static void pd_enqueue_stream(const PdPlan &P, const uint8_t *file, const int64_t *idat_table, int64_t idat_count, hipStream_t s)
{
    PdCtl *ctl = P.ctl;
    const long long *tab = reinterpret_cast<const long long *>(idat_table);
    hipLaunchKernelGGL(k_pd_chunk_scan, dim3(1), dim3(1024), 0, s, tab, (long long)idat_count, P.off);
    hipLaunchKernelGGL(k_pd_gather, dim3((unsigned)std::min<int64_t>(idat_count, 4096)), dim3(PD_GATHER_THREADS), 0, s, file, tab,
                       (long long)idat_count, P.off, reinterpret_cast<uint8_t *>(P.words), ctl);
    if (P.nmark) {
        hipLaunchKernelGGL(k_pd_mark, dim3((unsigned)P.nmark), dim3(PD_MARK_THREADS), 0, s, P.words, P.nw, P.nbits, P.masks, P.wgcnt, ctl);
        hipLaunchKernelGGL(k_pd_scan_u32, dim3(1), dim3(1024), 0, s, P.wgcnt, (long long)P.nmark, (unsigned int)P.ncap, ctl);
        hipLaunchKernelGGL(k_pd_compact, dim3((unsigned)P.nmark), dim3(PD_MARK_THREADS), 0, s, P.masks, P.wgcnt, (unsigned int)P.ncap, P.cands);
        hipLaunchKernelGGL(k_pd_pass_a, dim3(4096), dim3(64), 0, s, P.words, P.nw, P.nbits, P.cands, P.checks, (unsigned int)P.nslot, ctl);
    }
    hipLaunchKernelGGL(k_pd_walk, dim3(1), dim3(64), 0, s, P.words, P.nw, P.nbits, P.cands, P.checks, (unsigned int)P.nslot, P.blocks,
                       (unsigned int)P.bcap, P.need, ctl);
    hipLaunchKernelGGL(k_pd_pass_b, dim3(4096), dim3(64), 0, s, P.words, P.nw, P.nbits, P.blocks, P.need, P.lit, P.src, ctl);
    int rounds = 1;
    while ((1ull << (rounds - 1)) < P.need && rounds < 64) ++rounds;
    const unsigned jgrid = (unsigned)std::min<unsigned long long>((P.need + 255) / 256, 16384);
    for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(k_pd_jump, dim3(jgrid), dim3(256), 0, s, P.src, (long long)P.need, r, ctl);
}

}  // namespace lars

using namespace lars;

extern "C" {

size_t lars_png_decode_scratch_bytes(int64_t h, int64_t w, int channels, int64_t idat_bytes, int64_t idat_count)
{
    if (!pd_shape_ok(h, w, channels) || idat_bytes < 0 || idat_count < 1 || idat_bytes > (1ll << 40)) return 0;
    Carver size(nullptr);
    pd_plan(h, w, channels, idat_bytes, idat_count, size);
    return size.bytes();
}

int lars_d_decode_png_u8(const uint8_t *file, const int64_t *idat_table, int64_t idat_count, int64_t idat_bytes, int64_t h, int64_t w,
                         int channels, uint8_t *out, int32_t *status_dev, void *scratch, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!file || !idat_table || !out || !status_dev || !scratch || idat_count < 1 || idat_bytes < 0 || idat_bytes > (1ll << 40))
        return fail(LARS_ERR_INVALID, "lars_d_decode_png_u8: bad arguments");
    if (!pd_shape_ok(h, w, channels))
        return fail(LARS_ERR_INVALID, "lars_d_decode_png_u8: %lld x %lld x %d picture", (long long)h, (long long)w, channels);
    Carver cv(scratch);
    const PdPlan P = pd_plan(h, w, channels, idat_bytes, idat_count, cv);
    if (P.nmark >= (1ull << 31) || P.ncap >= (1ull << 32) || P.bcap >= (1ull << 32))
        return fail(LARS_ERR_UNSUPPORTED, "lars_d_decode_png_u8: %lld IDAT bytes", (long long)idat_bytes);
    PdCtl *ctl = P.ctl;
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(PdCtl), s));
    LARS_HIP_TRY(hipMemsetAsync(reinterpret_cast<char *>(P.words) + idat_bytes, 0, P.nw * 4 - (size_t)idat_bytes, s));   // zero tail
    pd_enqueue_stream(P, file, idat_table, idat_count, s);
    const long long rb = (long long)w * channels;
    if ((unsigned long long)rb != P.rbp) LARS_HIP_TRY(hipMemsetAsync(P.fpad, 0, (size_t)h * P.rbp, s));   // zero padding columns
    hipLaunchKernelGGL(k_pd_resolve, dim3((unsigned)P.nparts), dim3(256), 0, s, P.lit, P.src, (long long)P.need, (unsigned int)rb,
                       (unsigned int)P.rbp, P.fpad, P.ftype, P.parts, ctl);
    hipLaunchKernelGGL(k_pd_adler, dim3(1), dim3(256), 0, s, P.parts, (long long)P.nparts, (long long)P.need,
                       reinterpret_cast<const uint8_t *>(P.words), ctl);
    const long long ngroups = (h + 63) / 64;
    const int nwaves = (int)std::min<long long>(ngroups, PD_UNF_WAVES);
    hipLaunchKernelGGL(k_pd_unfilter, dim3(1), dim3(64 * nwaves), 0, s, P.fpad, P.ftype, (long long)h, (long long)P.rbp, channels, P.opad, ctl);
    const unsigned rgrid = (unsigned)std::min<long long>((h * rb + 255) / 256, 8192);
    hipLaunchKernelGGL(k_pd_rows, dim3(rgrid), dim3(256), 0, s, P.opad, (long long)h, rb, (long long)P.rbp, out, ctl);
    LARS_HIP_TRY(hipMemcpyAsync(status_dev, ctl->status, 8, hipMemcpyDeviceToDevice, s));
    return launch_check("lars_d_decode_png_u8");
}

size_t lars_png_decode_ex_scratch_bytes(int64_t h, int64_t w, int depth, int color_type, int interlace, int64_t idat_bytes, int64_t idat_count)
{
    PdxPlan X{};
    if (idat_bytes < 0 || idat_count < 1 || idat_bytes > (1ll << 40) || !pdx_layout(h, w, depth, color_type, interlace, X)) return 0;
    if (X.plain) return lars_png_decode_scratch_bytes(h, w, X.D.inc, idat_bytes, idat_count);
    Carver size(nullptr);
    pdx_plan(X, idat_bytes, idat_count, size);
    return size.bytes();
}

int lars_d_decode_png_ex(const uint8_t *file, const int64_t *idat_table, int64_t idat_count, int64_t idat_bytes, int64_t h, int64_t w,
                         int depth, int color_type, int interlace, uint8_t *out, int32_t *status_dev, void *scratch, void *stream)
{
    static const char *who = "lars_d_decode_png_ex";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!file || !idat_table || !out || !status_dev || !scratch || idat_count < 1 || idat_bytes < 0 || idat_bytes > (1ll << 40))
        return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    PdxPlan X{};
    if (!pdx_layout(h, w, depth, color_type, interlace, X))
        return fail(LARS_ERR_INVALID, "%s: %lld x %lld picture, bit depth %d, colour type %d, interlace %d", who, (long long)h, (long long)w,
                    depth, color_type, interlace);
    if (X.plain) return lars_d_decode_png_u8(file, idat_table, idat_count, idat_bytes, h, w, X.D.inc, out, status_dev, scratch, stream);
    if ((X.D.kind == PDX_GRAY16 && (uintptr_t)out % 2) || (X.D.kind == PDX_LA16 && (uintptr_t)out % 4))
        return fail(LARS_ERR_INVALID, "%s: out must be aligned to its %d-byte pixels", who, X.channels * X.itemsize);
    Carver cv(scratch);
    pdx_plan(X, idat_bytes, idat_count, cv);
    const PdPlan &P = X.P;
    if (P.nmark >= (1ull << 31) || P.ncap >= (1ull << 32) || P.bcap >= (1ull << 32))
        return fail(LARS_ERR_UNSUPPORTED, "%s: %lld IDAT bytes", who, (long long)idat_bytes);
    PdCtl *ctl = P.ctl;
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(PdCtl), s));
    LARS_HIP_TRY(hipMemsetAsync(reinterpret_cast<char *>(P.words) + idat_bytes, 0, P.nw * 4 - (size_t)idat_bytes, s));   // zero tail
    pd_enqueue_stream(P, file, idat_table, idat_count, s);
    LARS_HIP_TRY(hipMemsetAsync(P.fpad, 0, (size_t)X.pad_bytes, s));                                                     // zero padding columns
    hipLaunchKernelGGL(k_pdx_resolve, dim3((unsigned)P.nparts), dim3(256), 0, s, P.lit, P.src, (long long)P.need, X.D, P.fpad, P.ftype,
                       P.parts, ctl);
    hipLaunchKernelGGL(k_pd_adler, dim3(1), dim3(256), 0, s, P.parts, (long long)P.nparts, (long long)P.need,
                       reinterpret_cast<const uint8_t *>(P.words), ctl);
    const int nwaves = (int)std::min<long long>(X.max_groups, PD_UNF_WAVES);
    hipLaunchKernelGGL(k_pdx_unfilter, dim3((unsigned)X.D.npass), dim3(64 * nwaves), 0, s, P.fpad, P.ftype, X.D, P.opad, ctl);
    hipLaunchKernelGGL(k_pdx_place, dim3((unsigned)((w + 255) / 256), (unsigned)std::min<int64_t>(h, 32768)), dim3(256), 0, s, P.opad, X.D,
                       (long long)h, (long long)w, out, ctl);
    LARS_HIP_TRY(hipMemcpyAsync(status_dev, ctl->status, 8, hipMemcpyDeviceToDevice, s));
    return launch_check(who);
}

// host file in, host pixels out: one upload, the status, one download
int lars_h_decode_png_u8(const uint8_t *file, int64_t len, uint8_t *out, size_t out_cap)
{
    static const char *who = "lars_h_decode_png_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    PdFile F;
    LARS_TRY(F.parse(who, file, len));
    return decode_file_to_host(c, F, out, out_cap);
}

// host file in, thumbnail out: the decoded pixels go straight into the thumbnail kernels (resize.hip)
int lars_h_thumbnail_png_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                            int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    static const char *who = "lars_h_thumbnail_png_u8";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out || !reduce_box || !box) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    PdFile F;
    LARS_TRY(F.parse(who, file, len));
    if (F.ctype != 0 && F.ctype != 2 && F.ctype != 6)
        return fail(LARS_ERR_UNSUPPORTED, "%s: modes L, RGB and RGBA (colour type %lld)", who, (long long)F.ctype);
    return thumbnail_file(c, F, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

int lars_h_decode_png_ex(const uint8_t *file, int64_t len, uint8_t *out, size_t out_cap)
{
    static const char *who = "lars_h_decode_png_ex";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    PdFile F;
    LARS_TRY(F.parse(who, file, len, true));
    return decode_file_to_host(c, F, out, out_cap);
}

int lars_h_thumbnail_png_ex(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                            int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out)
{
    static const char *who = "lars_h_thumbnail_png_ex";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!out || !reduce_box || !box) return fail(LARS_ERR_INVALID, "%s: bad arguments", who);
    PdFile F;
    LARS_TRY(F.parse(who, file, len, true));
    // Pillow's modes L, RGB and RGBA: not 1 (1-bit gray), I;16, P or LA (8-bit gray + alpha)
    if (F.sample_bytes != 1 || F.ctype == 3 || (F.ctype == 0 && F.depth == 1) || (F.channels != 1 && F.channels != 3 && F.channels != 4))
        return fail(LARS_ERR_UNSUPPORTED, "%s: modes L, RGB and RGBA (colour type %lld, bit depth %d)", who, (long long)F.ctype, F.depth);
    return thumbnail_file(c, F, fx, fy, reduce_box, box, new_h, new_w, vertical_first, out);
}

}  // extern "C"
