// Region outlines (DESIGN.md "Region outlines"): the polygons of the labelled patches, traced on the device from the int32 label
// raster regions.hip writes -- what a GIS, an overlay or next week's process_image_zones(img, polygons) takes.
//
// The definition.  labels[h][w], 0 = background, 1 .. R = regions, every label one connected set under the connectivity; h * w < 2^29.
// Vertices are pixel corners, corner (r, c) the upper-left corner of pixel (r, c).  A pixel (y, x) of label L owns one directed edge
// per side whose neighbour is not L (outside the raster: not L), clockwise on the screen: side 0 top (y, x) -> (y, x + 1), 1 right
// (y, x + 1) -> (y + 1, x + 1), 2 bottom (y + 1, x + 1) -> (y + 1, x), 3 left (y + 1, x) -> (y, x); its id is 4 * (y * w + x) + side.
// The successor of an edge is the first that exists of the right turn (next side, same pixel), straight on (same side, next pixel along
// the edge) and the left turn (previous side of the pixel diagonally ahead on the outer side): in this order under connectivity 4, in
// the opposite order under 8.  With a = "the pixel behind the edge's start is L" and b = "the pixel diagonally behind it on the outer
// side is L" the predecessor is: 8: b ? left : a ? straight : right; 4: !a ? right : !b ? straight : left -- and the start of the edge
// is a vertex unless the predecessor is straight, !(a && !b), whatever the connectivity.  Rings are the cycles; a ring's key is its
// smallest edge id, its vertices start at the first vertex at or after that edge, its doubled area is the shoelace sum over (col, row):
// positive for an outer ring, negative for a hole.  Rings come sorted by (label, key).  Integers only: the same bytes on every run.
//
// The stages are launches on one stream; no workgroup waits for another.  A device-wide exclusive scan here is always three launches
// (k_ol_totals, k_ol_scan_totals, k_ol_place) over chunks of OL_ROUNDS * 256 items.
//   edges      scan of the edges per pixel: pixoff[pixel] = the index of its first edge, eid[index] = the edge id.  Indices are in id
//              order, so the smallest index of a ring is its key's
//   k_ol_init  jump[e] = the index of e's predecessor, found from the labels alone; mo[e] = (e, 0)
//   k_ol_jump  ceil(log2(E)) rounds of pointer doubling, from one pair of arrays into the other: after round k, mo[e] = (the smallest
//              index among e and its 2^k - 1 predecessors, the number of steps back to its first occurrence), jump[e] = 2^k steps back.
//              At the end: (the ring's smallest edge, e's position in the ring counted from it)
//   heads      scan of "e is its ring's smallest edge": rings numbered in key order, with their label and length
//   sort       the rings ordered by label, stably, so by (label, key): a radix sort of the ring numbers, 8 bits of the label a pass
//              (k_ol_sort_hist, k_ol_scan_totals, k_ol_sort_scatter), one pass for up to 255 regions
//   spans      scan of the ring lengths in sorted order: where each ring's edges stand in ring order, and the table rows
//   k_ol_scatter  every edge to its slot base[ring] + position, with its vertex flag; the doubled areas, one wave's stretch of one
//              ring folded before the atomic (integer sums: any order gives the same bits)
//   corners    scan of the vertex flags over the slots: the vertices are written where they belong, sorted rings one after another
//   k_ol_ring_counts  each row's first vertex and vertex count
//
// Every index read from memory (a jump, a ring number, a slot, an edge id) is used only after a range check against the count it
// indexes: damaged arrays give wrong rings, never an access outside the buffers.  Every loop is bounded by a count fixed before it.
#include "common.h"
#include "wg_device.h"

namespace lars {

namespace {

#define OL_ROUNDS 8                     // a scan chunk is OL_ROUNDS * 256 items
#define OL_CHUNK (OL_ROUNDS * 256)
#define OL_SEG 16                       // a wave folds the area terms of OL_SEG * 64 consecutive edges
#define OL_NONE 0xFFFFFFFFu
#define OL_PIXELS_MAX (1ll << 29)       // 4 * h * w fits int32

struct OlGrid {
    const int *labels;
    int h, w;
    __device__ int at(int y, int x) const                                        // 0 outside the raster and for a label below 0
    {
        if ((unsigned int)y >= (unsigned int)h || (unsigned int)x >= (unsigned int)w) return 0;
        const int v = labels[(size_t)y * (size_t)w + (size_t)x];
        return v > 0 ? v : 0;
    }
    // bit s: side s of pixel (y, x) of label L is an edge
    __device__ unsigned int sides(int y, int x, int L) const
    {
        return (at(y - 1, x) != L ? 1u : 0u) | (at(y, x + 1) != L ? 2u : 0u) | (at(y + 1, x) != L ? 4u : 0u) | (at(y, x - 1) != L ? 8u : 0u);
    }
};

__device__ inline int ol_dy(int s) { return (s == 1) - (s == 3); }               // the direction of side s: east, south, west, north
__device__ inline int ol_dx(int s) { return (s == 0) - (s == 2); }

// What the kernels take as counts: the device words, clamped to the room of the arrays.  More edges than the room: nothing is traced.
struct OlCounts {
    const long long *dev;               // [3]: edges, rings, vertices
    long long ecap, qcap;
    __device__ long long edges() const { const long long e = dev[0]; return e >= 0 && e <= ecap ? e : 0; }
    __device__ long long rings() const { const long long q = dev[1]; return edges() && q >= 0 && q <= qcap ? q : 0; }
};

struct OlEdge {
    int y, x, s, L;
    // false for an id outside the raster or on a background pixel
    __device__ bool decode(const OlGrid &G, int id)
    {
        if ((unsigned int)id >= 4u * (unsigned int)G.h * (unsigned int)G.w) return false;
        s = id & 3;
        y = (id >> 2) / G.w;
        x = (id >> 2) % G.w;
        L = G.at(y, x);
        return L != 0;
    }
    // the predecessor; *corner: the start of this edge is a vertex
    template <bool CONN8>
    __device__ OlEdge pred(const OlGrid &G, bool *corner) const
    {
        const int by = y - ol_dy(s), bx = x - ol_dx(s);                          // the pixel behind the start
        const int oy = by + ol_dy((s + 3) & 3), ox = bx + ol_dx((s + 3) & 3);    // and the one diagonally behind, on the outer side
        const bool a = G.at(by, bx) == L, b = G.at(oy, ox) == L;
        *corner = !(a && !b);
        const bool left = CONN8 ? b : (a && b), straight = a && !b;
        OlEdge p = *this;
        if (left) { p.y = oy; p.x = ox; p.s = (s + 1) & 3; }
        else if (straight) { p.y = by; p.x = bx; }
        else p.s = (s + 3) & 3;
        return p;
    }
    // the index of this edge among all edges (to be range-checked: pixoff is memory)
    __device__ long long index(const OlGrid &G, const unsigned int *pixoff) const
    {
        return (long long)pixoff[(size_t)y * (size_t)G.w + (size_t)x] + __builtin_popcount(G.sides(y, x, L) & ((1u << s) - 1u));
    }
    __device__ int row() const { return y + (s >> 1); }                          // the start corner
    __device__ int col() const { return x + ((s == 1 || s == 2) ? 1 : 0); }
    __device__ long long area_term() const                                       // x0 * y1 - x1 * y0 of the unit edge, (x, y) = (col, row)
    {
        return s == 0 ? -(long long)y : s == 1 ? (long long)x + 1 : s == 2 ? (long long)y + 1 : -(long long)x;
    }
};

// ===========================================================================
// the device-wide exclusive scan: Op gives count(), value(i) and place(i, value, sum of the values before i)
// ===========================================================================
template <typename Op>
__global__ __launch_bounds__(256) void k_ol_totals(Op op, long long nchunks, unsigned int *__restrict__ totals)
{
    __shared__ unsigned int s_w[4];
    const long long n = op.count();
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        unsigned int v = 0;
        for (int r = 0; r < OL_ROUNDS; ++r) {
            const long long i = (c * OL_ROUNDS + r) * 256 + threadIdx.x;
            v += i < n ? op.value(i) : 0u;
        }
        unsigned int total;
        wg_exscan<256, unsigned int>(v, s_w, &total);
        if (threadIdx.x == 0) totals[c] = total;
    }
}

__global__ __launch_bounds__(1024) void k_ol_scan_totals(unsigned int *__restrict__ totals, long long n, long long *__restrict__ count_out)
{
    const unsigned int total = wg_scan_array<unsigned int>(
        n, [&](long long i) { return totals[i]; }, [&](long long i, unsigned int before) { totals[i] = before; });
    if (threadIdx.x == 0 && count_out) *count_out = (long long)total;
}

template <typename Op>
__global__ __launch_bounds__(256) void k_ol_place(Op op, long long nchunks, const unsigned int *__restrict__ before)
{
    __shared__ unsigned int s_w[4];
    const long long n = op.count();
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        unsigned int carry = before[c];
        for (int r = 0; r < OL_ROUNDS; ++r) {
            const long long i = (c * OL_ROUNDS + r) * 256 + threadIdx.x;
            const unsigned int v = i < n ? op.value(i) : 0u;
            unsigned int total;
            const unsigned int ex = wg_exscan<256, unsigned int>(v, s_w, &total);
            if (i < n) op.place(i, v, carry + ex);
            carry += total;
        }
    }
}

// ---- the edges of every pixel ----
struct OlPixels {
    OlGrid G;
    unsigned int *pixoff, *eid;
    long long ecap;
    __device__ long long count() const { return (long long)G.h * G.w; }
    __device__ unsigned int mask(long long i) const
    {
        const int y = (int)(i / G.w), x = (int)(i % G.w), L = G.at(y, x);
        return L ? G.sides(y, x, L) : 0u;
    }
    __device__ unsigned int value(long long i) const { return (unsigned int)__builtin_popcount(mask(i)); }
    __device__ void place(long long i, unsigned int, unsigned int first) const
    {
        pixoff[i] = first;
        unsigned int m = mask(i);
        for (long long k = first; m; m &= m - 1u, ++k)                           // at most four
            if (k < ecap) eid[k] = 4u * (unsigned int)i + (unsigned int)__builtin_ctz(m);
    }
};

// ---- the rings, numbered in key order ----
template <bool CONN8>
struct OlHeads {
    OlGrid G;
    OlCounts N;
    const unsigned long long *mo;
    const unsigned int *pixoff, *eid;
    unsigned int *ringno, *head, *rlabel, *rlen;
    __device__ long long count() const { return N.edges(); }
    __device__ unsigned int value(long long e) const { return (long long)(mo[e] >> 32) == e ? 1u : 0u; }
    __device__ void place(long long e, unsigned int is_head, unsigned int k) const
    {
        if (!is_head || (long long)k >= N.qcap) return;
        ringno[e] = k;
        head[k] = (unsigned int)e;
        OlEdge E;
        unsigned int label = 0, len = 1;
        if (E.decode(G, (int)eid[e])) {
            bool corner;
            const long long last = E.pred<CONN8>(G, &corner).index(G, pixoff);   // the ring's last edge stands len - 1 steps from the head
            label = (unsigned int)E.L;
            if (last < N.edges()) len = (unsigned int)mo[last] + 1u;
        }
        rlabel[k] = label;
        rlen[k] = len;
    }
};

// ---- the rings in sorted order: where their edges stand, and their rows ----
struct OlSpans {
    OlCounts N;
    const unsigned int *pay, *rlen, *rlabel, *head, *eid;
    unsigned int *ebase, *spos;
    lars_outline_ring *table;
    long long ring_capacity;
    __device__ long long count() const { return N.rings(); }
    __device__ unsigned int value(long long i) const { const unsigned int k = pay[i]; return (long long)k < N.rings() ? rlen[k] : 0u; }
    __device__ void place(long long i, unsigned int, unsigned int first) const
    {
        const unsigned int k = pay[i];
        if ((long long)k >= N.rings()) return;
        ebase[k] = first;
        spos[k] = (unsigned int)i;
        if (i >= ring_capacity) return;
        const unsigned int e = head[k];
        lars_outline_ring t;
        t.label = (int32_t)rlabel[k];
        t.key = (long long)e < N.edges() ? (int32_t)eid[e] : 0;
        t.start = 0; t.count = 0; t.area2 = 0;
        table[i] = t;
    }
};

// ---- the vertices, in ring order ----
struct OlCorners {
    OlGrid G;
    OlCounts N;
    const unsigned int *ord;
    unsigned int *vidx;
    int32_t *verts;
    long long vert_capacity;
    __device__ long long count() const { return N.edges(); }
    __device__ unsigned int value(long long slot) const { return ord[slot] >> 31; }
    __device__ void place(long long slot, unsigned int is_vertex, unsigned int v) const
    {
        vidx[slot] = v;
        OlEdge E;
        if (!is_vertex || (long long)v >= vert_capacity || !E.decode(G, (int)(ord[slot] & 0x7FFFFFFFu))) return;
        verts[2 * (size_t)v] = E.row();
        verts[2 * (size_t)v + 1] = E.col();
    }
};

// ===========================================================================
// the edge count alone, for the caller who sizes the scratch by it
// ===========================================================================
__global__ __launch_bounds__(256) void k_ol_count(OlPixels P, unsigned long long *__restrict__ edges)
{
    __shared__ unsigned long long s_w[8];
    const long long n = P.count();
    unsigned long long mine = 0, none = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) mine += P.value(i);
    wg_sum2<256>(mine, none, s_w);
    if (threadIdx.x == 0 && mine) atomicAdd(edges, mine);
}

// ===========================================================================
// predecessors and pointer doubling
// ===========================================================================
template <bool CONN8>
__global__ __launch_bounds__(256) void k_ol_init(OlGrid G, OlCounts N, const unsigned int *__restrict__ pixoff, const unsigned int *__restrict__ eid,
                                                 unsigned int *__restrict__ jump, unsigned long long *__restrict__ mo)
{
    const long long n = N.edges();
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        OlEdge E;
        long long p = e;                                                         // an edge that cannot be read stands alone
        if (E.decode(G, (int)eid[e])) {
            bool corner;
            p = E.pred<CONN8>(G, &corner).index(G, pixoff);
            if (p >= n) p = e;
        }
        jump[e] = (unsigned int)p;
        mo[e] = (unsigned long long)e << 32;
    }
}

__global__ __launch_bounds__(256) void k_ol_jump(OlCounts N, const unsigned int *__restrict__ jump_in, const unsigned long long *__restrict__ mo_in,
                                                 unsigned int *__restrict__ jump_out, unsigned long long *__restrict__ mo_out, unsigned int step)
{
    const long long n = N.edges();
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        unsigned int j = jump_in[e];
        if ((long long)j >= n) j = (unsigned int)e;
        unsigned long long mine = mo_in[e];
        const unsigned long long far = mo_in[j];
        if ((far >> 32) < (mine >> 32)) mine = (far & 0xFFFFFFFF00000000ull) | (unsigned long long)((unsigned int)far + step);
        mo_out[e] = mine;
        jump_out[e] = jump_in[j];
    }
}

// ===========================================================================
// the rings ordered by label: a stable radix sort of the ring numbers, 8 bits a pass.  The key of entry i is rlabel[pay_in[i]]
// (pay_in null: the identity, the first pass).  hist[digit * nchunks + chunk], scanned in between, is where a chunk's entries of a digit go.
// ===========================================================================
__device__ inline unsigned int ol_sort_digit(const unsigned int *pay_in, const unsigned int *rlabel, long long i, long long n, int shift,
                                             unsigned int *ring)
{
    const unsigned int k = pay_in ? pay_in[i] : (unsigned int)i;
    *ring = k;
    return (long long)k < n ? (rlabel[k] >> shift) & 255u : 255u;
}

__global__ __launch_bounds__(256) void k_ol_sort_hist(OlCounts N, const unsigned int *__restrict__ pay_in, const unsigned int *__restrict__ rlabel, int shift,
                                                      long long nchunks, unsigned int *__restrict__ hist)
{
    __shared__ unsigned int s_h[256];
    const long long n = N.rings();
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        s_h[threadIdx.x] = 0;
        __syncthreads();
        for (int r = 0; r < OL_ROUNDS; ++r) {
            const long long i = (c * OL_ROUNDS + r) * 256 + threadIdx.x;
            unsigned int ring;
            if (i < n) atomicAdd(&s_h[ol_sort_digit(pay_in, rlabel, i, n, shift, &ring)], 1u);
        }
        __syncthreads();
        hist[(size_t)threadIdx.x * (size_t)nchunks + (size_t)c] = s_h[threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_ol_sort_scatter(OlCounts N, const unsigned int *__restrict__ pay_in, const unsigned int *__restrict__ rlabel, int shift,
                                                         long long nchunks, const unsigned int *__restrict__ hist, unsigned int *__restrict__ pay_out)
{
    __shared__ unsigned int s_base[256], s_cnt[4][256];
    const long long n = N.rings();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        s_base[threadIdx.x] = hist[(size_t)threadIdx.x * (size_t)nchunks + (size_t)c];
        for (int r = 0; r < OL_ROUNDS; ++r) {                                    // 256 entries a round, in order: the sort is stable
            for (int q = 0; q < 4; ++q) s_cnt[q][threadIdx.x] = 0;
            __syncthreads();
            const long long i = (c * OL_ROUNDS + r) * 256 + threadIdx.x;
            const bool live = i < n;
            unsigned int ring = 0;
            const unsigned int d = live ? ol_sort_digit(pay_in, rlabel, i, n, shift, &ring) : 0u;
            unsigned long long same = __ballot(live);                            // the lanes of this wave with my digit
            for (int b = 0; b < 8; ++b) {
                const unsigned long long has = __ballot(live && ((d >> b) & 1u));
                same &= ((d >> b) & 1u) ? has : ~has;
            }
            const unsigned int rank = (unsigned int)__builtin_popcountll(same & ((1ull << lane) - 1ull));
            if (live && rank == 0) s_cnt[wv][d] = (unsigned int)__builtin_popcountll(same);
            __syncthreads();
            if (live) {
                unsigned int dst = s_base[d] + rank;
                for (int q = 0; q < wv; ++q) dst += s_cnt[q][d];
                if ((long long)dst < n) pay_out[dst] = ring;
            }
            __syncthreads();
            s_base[threadIdx.x] += s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
            __syncthreads();
        }
    }
}

// ===========================================================================
// every edge to its place in ring order, and the doubled areas
// ===========================================================================
__device__ inline void ol_area_flush(lars_outline_ring *table, unsigned int row, long long sum, int lane)
{
    if (lane == 0 && row != OL_NONE && sum) atomicAdd(reinterpret_cast<unsigned long long *>(&table[row].area2), (unsigned long long)sum);
}

template <bool CONN8>
__global__ __launch_bounds__(256) void k_ol_scatter(OlGrid G, OlCounts N, const unsigned long long *__restrict__ mo, const unsigned int *__restrict__ eid,
                                                    const unsigned int *__restrict__ ringno, const unsigned int *__restrict__ ebase,
                                                    const unsigned int *__restrict__ spos, unsigned int *__restrict__ ord,
                                                    lars_outline_ring *__restrict__ table, long long ring_capacity)
{
    const long long n = N.edges(), nq = N.rings(), nseg = (n + OL_SEG * 64 - 1) / (OL_SEG * 64);
    const int lane = threadIdx.x & 63;
    unsigned int held = OL_NONE;
    long long held_sum = 0;
    for (long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); seg < nseg; seg += (long long)gridDim.x * 4) {   // wave-uniform
        for (int it = 0; it < OL_SEG; ++it) {
            const long long e = (seg * OL_SEG + it) * 64 + lane;
            unsigned int row = OL_NONE;
            long long term = 0;
            OlEdge E;
            if (e < n && E.decode(G, (int)eid[e])) {
                const unsigned long long m = mo[e];
                const long long first = (long long)(m >> 32);
                const unsigned int k = first < n ? ringno[first] : OL_NONE;
                if ((long long)k < nq) {
                    bool corner;
                    E.pred<CONN8>(G, &corner);
                    const long long slot = (long long)ebase[k] + (long long)(unsigned int)m;
                    if (slot < n) ord[slot] = eid[e] | (corner ? 0x80000000u : 0u);
                    const unsigned int i = spos[k];
                    if ((long long)i < nq && (long long)i < ring_capacity) { row = i; term = E.area_term(); }
                }
            }
            unsigned long long todo = __ballot(row != OL_NONE);                  // every lane stays in every ballot and shuffle
            while (todo) {
                const unsigned int z = __shfl(row, __builtin_ctzll(todo), 64);
                const unsigned long long same = __ballot(row == z);
                long long sum = row == z ? term : 0;
                for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
                if (z != held) {
                    ol_area_flush(table, held, held_sum, lane);
                    held = z;
                    held_sum = 0;
                }
                held_sum += sum;
                todo &= ~same;
            }
        }
    }
    ol_area_flush(table, held, held_sum, lane);
}

__global__ __launch_bounds__(256) void k_ol_ring_counts(OlCounts N, const unsigned int *__restrict__ pay, const unsigned int *__restrict__ ebase,
                                                        const unsigned int *__restrict__ rlen, const unsigned int *__restrict__ vidx,
                                                        lars_outline_ring *__restrict__ table, long long ring_capacity)
{
    const long long n = N.edges(), nq = N.rings(), rows = nq < ring_capacity ? nq : ring_capacity;
    const long long nverts = N.dev[2];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        const unsigned int k = pay[i];
        if ((long long)k >= nq) continue;
        const long long first = ebase[k], end = first + rlen[k];
        const long long v0 = first < n ? vidx[first] : nverts, v1 = end < n ? vidx[end] : nverts;
        table[i].start = (int32_t)v0;
        table[i].count = (int32_t)(v1 - v0);
    }
}

// The buffers of a trace with room for ecap edges, cut from the scratch: 4 bytes a pixel, 35 and a little a byte an edge.
struct OlBufs {
    unsigned int *pixoff, *totals, *eid, *jump[2], *head, *rlabel, *rlen, *ebase, *spos, *pay[2], *hist;
    unsigned long long *mo[2];
    long long qcap, pix_chunks, edge_chunks, ring_chunks;
    OlBufs(Carver &c, long long npix, long long ecap)
    {
        qcap = ecap / 4 + 1;                                                     // a ring has four edges or more
        pix_chunks = (npix + OL_CHUNK - 1) / OL_CHUNK;
        edge_chunks = (ecap + OL_CHUNK - 1) / OL_CHUNK;
        ring_chunks = (qcap + OL_CHUNK - 1) / OL_CHUNK;
        const long long most = pix_chunks > edge_chunks ? pix_chunks : edge_chunks;
        pixoff = c.take<unsigned int>((size_t)npix);
        totals = c.take<unsigned int>((size_t)(most > ring_chunks ? most : ring_chunks) + 1);
        eid = c.take<unsigned int>((size_t)ecap);
        for (int k = 0; k < 2; ++k) jump[k] = c.take<unsigned int>((size_t)ecap), mo[k] = c.take<unsigned long long>((size_t)ecap);
        head = c.take<unsigned int>((size_t)qcap);
        rlabel = c.take<unsigned int>((size_t)qcap);
        rlen = c.take<unsigned int>((size_t)qcap);
        ebase = c.take<unsigned int>((size_t)qcap);
        spos = c.take<unsigned int>((size_t)qcap);
        for (int k = 0; k < 2; ++k) pay[k] = c.take<unsigned int>((size_t)qcap);
        hist = c.take<unsigned int>(256 * (size_t)ring_chunks);
    }
};

unsigned int ol_grid(long long blocks) { return (unsigned int)(blocks < 1 ? 1 : blocks < 65536 ? blocks : 65536); }

template <typename Op>
void ol_scan(const Op &op, long long nchunks, unsigned int *totals, long long *count_out, hipStream_t s)
{
    hipLaunchKernelGGL((k_ol_totals<Op>), dim3(ol_grid(nchunks)), dim3(256), 0, s, op, nchunks, totals);
    hipLaunchKernelGGL(k_ol_scan_totals, dim3(1), dim3(1024), 0, s, totals, nchunks, count_out);
    hipLaunchKernelGGL((k_ol_place<Op>), dim3(ol_grid(nchunks)), dim3(256), 0, s, op, nchunks, totals);
}

bool ol_raster_ok(int64_t h, int64_t w) { return h >= 1 && w >= 1 && h < OL_PIXELS_MAX && w < OL_PIXELS_MAX && h * w < OL_PIXELS_MAX; }

template <bool CONN8>
void ol_trace(const OlGrid &G, const OlCounts &N, const OlBufs &B, int64_t n_labels, lars_outline_ring *rings, int64_t ring_capacity, int32_t *verts,
              int64_t vert_capacity, long long *counts, hipStream_t s)
{
    const long long ecap = N.ecap;
    const dim3 edge_grid(grid_1d(ecap)), ring_grid(ol_grid(B.ring_chunks));
    ol_scan(OlPixels{G, B.pixoff, B.eid, ecap}, B.pix_chunks, B.totals, counts, s);
    hipLaunchKernelGGL((k_ol_init<CONN8>), edge_grid, dim3(256), 0, s, G, N, B.pixoff, B.eid, B.jump[0], B.mo[0]);
    int at = 0;
    for (long long reach = 1; reach < ecap; reach *= 2, at ^= 1)                 // ceil(log2(ecap)) rounds
        hipLaunchKernelGGL(k_ol_jump, edge_grid, dim3(256), 0, s, N, B.jump[at], B.mo[at], B.jump[at ^ 1], B.mo[at ^ 1], (unsigned int)reach);
    const unsigned long long *mo = B.mo[at];
    unsigned int *ringno = B.jump[0], *ord = B.jump[1], *vidx = reinterpret_cast<unsigned int *>(B.mo[at ^ 1]);   // done with: reused
    ol_scan(OlHeads<CONN8>{G, N, mo, B.pixoff, B.eid, ringno, B.head, B.rlabel, B.rlen}, B.edge_chunks, B.totals, counts + 1, s);
    const unsigned int *pay = nullptr;
    int to = 0;
    for (int shift = 0; shift == 0 || (n_labels >> shift) != 0; shift += 8, to ^= 1) {
        hipLaunchKernelGGL(k_ol_sort_hist, ring_grid, dim3(256), 0, s, N, pay, B.rlabel, shift, B.ring_chunks, B.hist);
        hipLaunchKernelGGL(k_ol_scan_totals, dim3(1), dim3(1024), 0, s, B.hist, 256 * B.ring_chunks, (long long *)nullptr);
        hipLaunchKernelGGL(k_ol_sort_scatter, ring_grid, dim3(256), 0, s, N, pay, B.rlabel, shift, B.ring_chunks, B.hist, B.pay[to]);
        pay = B.pay[to];
    }
    ol_scan(OlSpans{N, pay, B.rlen, B.rlabel, B.head, B.eid, B.ebase, B.spos, rings, ring_capacity}, B.ring_chunks, B.totals, nullptr, s);
    hipLaunchKernelGGL((k_ol_scatter<CONN8>), dim3(grid_1d((ecap + OL_SEG * 64 - 1) / (OL_SEG * 64), 4)), dim3(256), 0, s, G, N, mo, B.eid, ringno, B.ebase,
                       B.spos, ord, rings, (long long)ring_capacity);
    ol_scan(OlCorners{G, N, ord, vidx, verts, vert_capacity}, B.edge_chunks, B.totals, counts + 2, s);
    hipLaunchKernelGGL(k_ol_ring_counts, dim3(grid_1d(B.qcap < ring_capacity ? B.qcap : ring_capacity)), dim3(256), 0, s, N, pay, B.ebase, B.rlen, vidx, rings,
                       (long long)ring_capacity);
}

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" size_t lars_region_outline_scratch_bytes(int64_t h, int64_t w, int64_t edge_capacity)
{
    if (!ol_raster_ok(h, w) || edge_capacity < 0 || edge_capacity > 4 * h * w) return 0;
    Carver c(nullptr);
    OlBufs B(c, h * w, edge_capacity);
    return c.bytes();
}

extern "C" int lars_d_region_outline_count(const int32_t *labels, int64_t h, int64_t w, int64_t *edges_dev, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!labels || !edges_dev || !ol_raster_ok(h, w))
        return fail(LARS_ERR_INVALID, "lars_d_region_outline_count: labels, the count and a raster of 1 or more on each side and fewer than 2^29 pixels are required");
    if (!aligned_to(labels, 4) || !aligned_to(edges_dev, 8)) return fail(LARS_ERR_INVALID, "lars_d_region_outline_count: labels must be 4-byte and the count 8-byte aligned");
    hipStream_t s = pick_stream(c, stream);
    LARS_HIP_TRY(hipMemsetAsync(edges_dev, 0, sizeof(int64_t), s));
    const OlPixels P = {{labels, (int)h, (int)w}, nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_ol_count, dim3(grid_1d(h * w, 1024)), dim3(256), 0, s, P, reinterpret_cast<unsigned long long *>(edges_dev));
    return launch_check("lars_d_region_outline_count");
}

extern "C" int lars_d_region_outline(const int32_t *labels, int64_t h, int64_t w, int connectivity, int64_t n_labels, int64_t edge_capacity,
                                     lars_outline_ring *rings, int64_t ring_capacity, int32_t *verts, int64_t vert_capacity, int64_t *counts_dev,
                                     void *scratch, void *stream)
{
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (!ol_raster_ok(h, w))
        return fail(LARS_ERR_INVALID, "lars_d_region_outline: the raster is 1 or more on each side and has fewer than 2^29 pixels (an edge id fits int32), got %lld x %lld",
                    (long long)h, (long long)w);
    if (!labels || !counts_dev || !scratch || (connectivity != 4 && connectivity != 8) || n_labels < 0 || n_labels > 0x7FFFFFFF || edge_capacity < 0 ||
        edge_capacity > 4 * h * w || ring_capacity < 0 || vert_capacity < 0 || (ring_capacity > 0 && !rings) || (vert_capacity > 0 && !verts))
        return fail(LARS_ERR_INVALID, "lars_d_region_outline: bad arguments (connectivity 4 or 8, n_labels 0 to 2^31 - 1, edge_capacity 0 to 4 * h * w, "
                                      "a ring table and a vertex array of capacity >= 0)");
    if (!aligned_to(labels, 4) || !aligned_to(rings, 8) || !aligned_to(verts, 4) || !aligned_to(counts_dev, 8) || !aligned_to(scratch, 256))
        return fail(LARS_ERR_INVALID, "lars_d_region_outline: labels and verts must be 4-byte, rings and counts 8-byte and scratch 256-byte aligned");
    hipStream_t s = pick_stream(c, stream);
    Carver cv(scratch);
    const OlBufs B(cv, h * w, edge_capacity);
    const OlGrid G = {labels, (int)h, (int)w};
    long long *counts = reinterpret_cast<long long *>(counts_dev);
    const OlCounts N = {counts, (long long)edge_capacity, B.qcap};
    LARS_HIP_TRY(hipMemsetAsync(counts_dev, 0, 3 * sizeof(int64_t), s));
    if (connectivity == 8) ol_trace<true>(G, N, B, n_labels, rings, ring_capacity, verts, vert_capacity, counts, s);
    else ol_trace<false>(G, N, B, n_labels, rings, ring_capacity, verts, vert_capacity, counts, s);
    return launch_check("lars_d_region_outline");
}
