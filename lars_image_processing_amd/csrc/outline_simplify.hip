// Simplified outlines (DESIGN.md "Simplified outlines"): Douglas-Peucker with a tolerance on the rings outlines.hip writes, on the
// device, before the vertices cross PCIe.
//
// The definition (include/lars_hip.h "simplified outlines", tests/outline_simplify_model.py).  A ring of n vertices (row, col) is the
// chain v[0] .. v[n], v[n] = v[0]; coordinates are 0 .. 32767.  tq is the tolerance in sixteenths of a pixel, 1 .. 4064.  For a chord
// a -> b and a vertex p: ab = b - a, ap = p - a, len2 = |ab|^2.  len2 == 0: m = |ap|^2, p is far when 256 * m > tq^2.  Otherwise
// dot = ap . ab; m = |ap|^2 * len2 if dot <= 0, |bp|^2 * len2 if dot >= len2, else cross(ab, ap)^2: the squared distance to the segment
// times len2 (m < 2^62, tq^2 * len2 < 2^56); p is far when m > (tq^2 * len2) >> 8.  Both ends of the chain are kept; a stretch (a, b)
// with b - a >= 2 takes the k in (a, b) of the largest m, the smallest k on ties; if that vertex is far it is kept and (a, k), (k, b)
// are treated the same way.  A ring whose result has fewer than 3 vertices, or a doubled area that is 0 or of the other sign than the
// ring's own shoelace sum, stays as given, with all its vertices.  Rings, their order, label and key never change; start, count and
// area2 describe the vertices written.  Integers only: the same bytes on every run.
//
// The recursion runs level by level: stretches do not depend on each other.  One slot per vertex in ring order, and one more per ring
// for the closing copy of v[0]; a slot is kept, done, or inside a stretch whose ends (a, b) it knows.  A stretch is named by its left
// end a, which is a kept slot.  One round is three launches:
//   k_os_measure  every slot inside a stretch computes its m; best_m[a] = the largest of them.  The lanes of a wave that share a stretch
//                 stand side by side, so a segmented reduction by shuffles leaves one atomic per stretch and wave
//   k_os_pick     the slots that hold the largest m, where it is far: best_k[a] = the smallest of them, reduced the same way
//   k_os_split    best_k[a] is kept and every slot of the stretch moves its a or b there; no such slot: the stretch is done
// Maximum and minimum do not depend on the order, so neither do the bytes.  The number of rounds is not known before the run: the host
// reads the longest ring's vertex count, which bounds the rounds, then enqueues OS_BATCH rounds at a time, reads the status words (the
// splits of the batch among them) and stops at 0; no round beyond the bound is enqueued, a split in the last one allowed is an error
// return.  No workgroup waits for another.  Then the kept counts and shoelace sums of every ring
// (k_os_sums: integer sums, one wave's stretch of one ring folded before the atomic), the collapse rule (k_os_decide) and one
// device-wide scan that places the vertices and the rows' starts.  The three-launch scan is a local copy of the one in outlines.hip
// (k_ol_totals, k_ol_scan_totals, k_ol_place), which keeps its own inside its namespace.
//
// Every index read from memory (a ring's start and count, a slot's ring, a stretch's ends, its pick) is used only after a range check:
// damaged rings give wrong rings, never an access outside the buffers.  Coordinates are clamped to 0 .. h and 0 .. w, so no product
// leaves 64 bits.  Every loop is bounded by a count fixed before it.
#include "common.h"
#include "wg_device.h"

namespace lars {

namespace {

#define OS_ROUNDS 8                     // a scan chunk is OS_ROUNDS * 256 items
#define OS_CHUNK (OS_ROUNDS * 256)
#define OS_BATCH 8                      // rounds between two reads of the status
#define OS_NONE 0xFFFFFFFFu
#define OS_SIDE_MAX 32767
#define OS_TQ_MAX 4064
#define OS_CAPACITY_MAX 0x7FFFFFFFll    // rings and vertices each: a slot index fits 32 bits and is never OS_NONE

enum { OS_INSIDE = 0, OS_KEPT = 1, OS_DONE = 2 };

// The status words on the device: what the host reads after a batch.
struct OsStatus {
    long long splits;                   // of the rounds since the host last cleared it
    long long longest;                  // the vertices of the longest ring
    long long rounds;                   // the rounds in which a stretch was split
    long long slots;                    // the vertices of the usable rings, and one a ring
};

// What the kernels take as counts: the tracer's words, clamped to the room of the arrays as OlCounts does it.
struct OsCounts {
    const long long *dev;               // [3]: edges, rings, vertices
    long long qcap, vcap;
    __device__ long long rings() const { const long long q = dev[1]; return q >= 0 && q <= qcap ? q : 0; }
    __device__ long long verts() const { const long long v = dev[2]; return v >= 0 && v <= vcap ? v : 0; }
};

// the vertices of a ring whose row can be followed, else 0: such a ring has no slot and writes nothing
__device__ inline unsigned int os_ring_verts(const lars_outline_ring &t, long long nverts)
{
    const long long s = t.start, c = t.count;
    return s >= 0 && c >= 1 && s + c <= nverts ? (unsigned int)c : 0u;
}

__device__ inline long long os_row(unsigned int p) { return (long long)(p >> 16); }
__device__ inline long long os_col(unsigned int p) { return (long long)(p & 0xFFFFu); }

// m and len2 of vertex P against the chord A -> B, each packed (row << 16) | col
__device__ inline unsigned long long os_measure(unsigned int A, unsigned int B, unsigned int P, unsigned long long *len2_out)
{
    const long long abr = os_row(B) - os_row(A), abc = os_col(B) - os_col(A), apr = os_row(P) - os_row(A), apc = os_col(P) - os_col(A);
    const long long len2 = abr * abr + abc * abc, ap2 = apr * apr + apc * apc;
    *len2_out = (unsigned long long)len2;
    if (len2 == 0) return (unsigned long long)ap2;
    const long long dot = apr * abr + apc * abc;
    if (dot <= 0) return (unsigned long long)(ap2 * len2);
    if (dot >= len2) {
        const long long bpr = os_row(P) - os_row(B), bpc = os_col(P) - os_col(B);
        return (unsigned long long)((bpr * bpr + bpc * bpc) * len2);
    }
    const long long cross = abr * apc - abc * apr;
    return (unsigned long long)(cross * cross);
}

__device__ inline bool os_far(unsigned long long m, unsigned long long len2, unsigned long long tq2) { return m > ((tq2 * (len2 ? len2 : 1ull)) >> 8); }

// x0 * y1 - x1 * y0 over (x, y) = (col, row)
__device__ inline long long os_area_term(unsigned int P, unsigned int Q) { return os_col(P) * os_row(Q) - os_col(Q) * os_row(P); }

// Segmented reductions over the lanes of a wave: lanes with the same key stand side by side; afterwards the first lane of every run
// holds the run's result.  Every lane of the wave calls these.
__device__ inline unsigned long long os_seg_max(unsigned long long v, unsigned int key, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        const unsigned int k = __shfl_down(key, off, 64);
        if (lane + off < 64 && k == key && o > v) v = o;
    }
    return v;
}
__device__ inline unsigned int os_seg_min(unsigned int v, unsigned int key, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int o = __shfl_down(v, off, 64), k = __shfl_down(key, off, 64);
        if (lane + off < 64 && k == key && o < v) v = o;
    }
    return v;
}
__device__ inline long long os_seg_sum(long long v, unsigned int key, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_down(v, off, 64);
        const unsigned int k = __shfl_down(key, off, 64);
        if (lane + off < 64 && k == key) v += o;
    }
    return v;
}
__device__ inline bool os_seg_head(unsigned int key, int lane)
{
    const unsigned int before = __shfl_up(key, 1, 64);
    return lane == 0 || before != key;
}

// ===========================================================================
// the device-wide exclusive scan, as in outlines.hip: Op gives count(), value(i) and place(i, value, sum of the values before i)
// ===========================================================================
template <typename Op>
__global__ __launch_bounds__(256) void k_os_totals(Op op, long long nchunks, unsigned int *__restrict__ totals)
{
    __shared__ unsigned int s_w[4];
    const long long n = op.count();
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        unsigned int v = 0;
        for (int r = 0; r < OS_ROUNDS; ++r) {
            const long long i = (c * OS_ROUNDS + r) * 256 + threadIdx.x;
            v += i < n ? op.value(i) : 0u;
        }
        unsigned int total;
        wg_exscan<256, unsigned int>(v, s_w, &total);
        if (threadIdx.x == 0) totals[c] = total;
    }
}

__global__ __launch_bounds__(1024) void k_os_scan_totals(unsigned int *__restrict__ totals, long long n, long long *__restrict__ count_out)
{
    const unsigned int total = wg_scan_array<unsigned int>(
        n, [&](long long i) { return totals[i]; }, [&](long long i, unsigned int before) { totals[i] = before; });
    if (threadIdx.x == 0 && count_out) *count_out = (long long)total;
}

template <typename Op>
__global__ __launch_bounds__(256) void k_os_place(Op op, long long nchunks, const unsigned int *__restrict__ before)
{
    __shared__ unsigned int s_w[4];
    const long long n = op.count();
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {                // block-uniform
        unsigned int carry = before[c];
        for (int r = 0; r < OS_ROUNDS; ++r) {
            const long long i = (c * OS_ROUNDS + r) * 256 + threadIdx.x;
            const unsigned int v = i < n ? op.value(i) : 0u;
            unsigned int total;
            const unsigned int ex = wg_exscan<256, unsigned int>(v, s_w, &total);
            if (i < n) op.place(i, v, carry + ex);
            carry += total;
        }
    }
}

// The buffers of a run with room for qcap rings and vcap vertices, cut from the scratch: 29 bytes a slot (a vertex, and one more a
// ring) and 29 bytes a ring besides.
struct OsBufs {
    unsigned int *sbase, *totals, *ring, *pts, *a, *b, *best_k;
    unsigned long long *best_m, *acc;
    unsigned char *state, *restored;
    OsStatus *status;
    long long scap, ring_chunks, slot_chunks;
    OsBufs(Carver &c, long long qcap, long long vcap)
    {
        scap = qcap + vcap;
        ring_chunks = (qcap + OS_CHUNK - 1) / OS_CHUNK;
        slot_chunks = (scap + OS_CHUNK - 1) / OS_CHUNK;
        status = c.take<OsStatus>(1);
        sbase = c.take<unsigned int>((size_t)qcap);
        totals = c.take<unsigned int>((size_t)(slot_chunks > ring_chunks ? slot_chunks : ring_chunks) + 1);
        acc = c.take<unsigned long long>(3 * (size_t)qcap);
        restored = c.take<unsigned char>((size_t)qcap);
        ring = c.take<unsigned int>((size_t)scap);
        pts = c.take<unsigned int>((size_t)scap);
        a = c.take<unsigned int>((size_t)scap);
        b = c.take<unsigned int>((size_t)scap);
        best_k = c.take<unsigned int>((size_t)scap);
        best_m = c.take<unsigned long long>((size_t)scap);
        state = c.take<unsigned char>((size_t)scap);
    }
};

// What every kernel of a run reads: the rings and vertices given, their counts, and the slots.
struct OsRun {
    const lars_outline_ring *rings;
    const int32_t *verts;
    OsCounts N;
    OsStatus *status;
    unsigned int *sbase, *ring, *pts, *a, *b, *best_k;
    unsigned long long *best_m, *acc;
    unsigned char *state, *restored;
    long long scap;
    int h, w;
    __device__ long long slots() const { const long long s = status->slots; return s >= 0 && s <= scap ? s : 0; }
    // is slot s (below slots()) the closing copy of its ring's first vertex?
    __device__ bool closing(long long s, long long n) const { return s + 1 >= n || ring[s + 1] != ring[s]; }
};

// ---- the slots of every ring ----
struct OsRingSlots {
    OsRun R;
    __device__ long long count() const { return R.N.rings(); }
    __device__ unsigned int value(long long i) const
    {
        const unsigned int c = os_ring_verts(R.rings[i], R.N.verts());
        return c ? c + 1u : 0u;
    }
    __device__ void place(long long i, unsigned int, unsigned int first) const { R.sbase[i] = first; }
};

__global__ __launch_bounds__(256) void k_os_longest(OsRun R)
{
    const long long n = R.N.rings(), nv = R.N.verts(), span = (n + 63) / 64 * 64;
    unsigned int mine = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < span; i += (long long)gridDim.x * 256) {
        const unsigned int c = i < n ? os_ring_verts(R.rings[i], nv) : 0u;
        mine = c > mine ? c : mine;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned int o = __shfl_xor(mine, off, 64);
        mine = o > mine ? o : mine;
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicMax(reinterpret_cast<unsigned long long *>(&R.status->longest), (unsigned long long)mine);
}

// Every slot finds its ring (the last one whose first slot is not behind it), takes its vertex and its first stretch: the whole ring.
__global__ __launch_bounds__(256) void k_os_init(OsRun R)
{
    const long long n = R.slots(), nq = R.N.rings(), nv = R.N.verts();
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n; s += (long long)gridDim.x * 256) {
        long long lo = 0, hi = nq;                                               // the rings lo .. hi - 1 may hold s; at most 32 steps
        while (hi - lo > 1) {
            const long long mid = lo + (hi - lo) / 2;
            if ((long long)R.sbase[mid] <= s) lo = mid; else hi = mid;
        }
        unsigned int ring = OS_NONE, pt = 0, a = OS_NONE, b = OS_NONE;
        unsigned char state = OS_DONE;
        if (lo < nq) {
            const lars_outline_ring t = R.rings[lo];
            const long long c = os_ring_verts(t, nv), p = s - (long long)R.sbase[lo];
            if (c && p >= 0 && p <= c && (long long)R.sbase[lo] + c < n) {
                const long long v = (long long)t.start + (p == c ? 0 : p);
                int row = R.verts[2 * (size_t)v], col = R.verts[2 * (size_t)v + 1];
                row = row < 0 ? 0 : row > R.h ? R.h : row;
                col = col < 0 ? 0 : col > R.w ? R.w : col;
                ring = (unsigned int)lo;
                pt = ((unsigned int)row << 16) | (unsigned int)col;
                a = R.sbase[lo];
                b = a + (unsigned int)c;
                state = p == 0 || p == c ? OS_KEPT : OS_INSIDE;
            }
        }
        R.ring[s] = ring;
        R.pts[s] = pt;
        R.a[s] = a;
        R.b[s] = b;
        R.state[s] = state;
        R.best_m[s] = 0;
        R.best_k[s] = OS_NONE;
    }
}

// The stretch of slot s, if s is inside one whose ends can be followed: its name (the left end) and m, else OS_NONE.
__device__ inline unsigned int os_stretch(const OsRun &R, long long s, long long n, unsigned long long *m, unsigned long long *len2, unsigned int *right)
{
    *m = 0;
    *len2 = 0;
    *right = OS_NONE;
    if (s >= n || R.state[s] != OS_INSIDE) return OS_NONE;
    const unsigned int a = R.a[s], b = R.b[s];
    if (!((long long)a < s && s < (long long)b && (long long)b < n)) return OS_NONE;
    *m = os_measure(R.pts[a], R.pts[b], R.pts[s], len2);
    *right = b;
    return a;
}

__global__ __launch_bounds__(256) void k_os_measure(OsRun R)
{
    const long long n = R.slots(), span = (n + 63) / 64 * 64;
    const int lane = threadIdx.x & 63;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < span; s += (long long)gridDim.x * 256) {     // wave-uniform
        unsigned long long m, len2;
        unsigned int b;
        const unsigned int key = os_stretch(R, s, n, &m, &len2, &b);
        if (!__any(key != OS_NONE)) continue;
        if (key != OS_NONE && s == (long long)key + 1) R.best_k[key] = OS_NONE;  // nobody reads it in this launch
        const unsigned long long most = os_seg_max(m, key, lane);
        if (os_seg_head(key, lane) && key != OS_NONE && most) atomicMax(&R.best_m[key], most);
    }
}

__global__ __launch_bounds__(256) void k_os_pick(OsRun R, unsigned long long tq2)
{
    const long long n = R.slots(), span = (n + 63) / 64 * 64;
    const int lane = threadIdx.x & 63;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < span; s += (long long)gridDim.x * 256) {     // wave-uniform
        unsigned long long m, len2;
        unsigned int b;
        const unsigned int key = os_stretch(R, s, n, &m, &len2, &b);
        if (!__any(key != OS_NONE)) continue;
        const bool mine = key != OS_NONE && m == R.best_m[key] && os_far(m, len2, tq2);
        const unsigned int first = os_seg_min(mine ? (unsigned int)s : OS_NONE, key, lane);
        if (os_seg_head(key, lane) && key != OS_NONE && first != OS_NONE) atomicMin(&R.best_k[key], first);
    }
}

__global__ __launch_bounds__(256) void k_os_split(OsRun R, long long round)
{
    const long long n = R.slots(), span = (n + 63) / 64 * 64;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < span; s += (long long)gridDim.x * 256) {     // wave-uniform
        bool split = false;
        if (s < n && R.state[s] == OS_INSIDE) {
            const unsigned int a = R.a[s], b = R.b[s];
            const bool sound = (long long)a < s && s < (long long)b && (long long)b < n;
            const unsigned int k = sound ? R.best_k[a] : OS_NONE;
            if (!(k != OS_NONE && a < k && k < b)) {
                R.state[s] = OS_DONE;
            } else if ((long long)k == s) {
                R.state[s] = OS_KEPT;
                R.best_m[s] = 0;                                                 // the stretch to its right starts from nothing
                split = true;
            } else if (s < (long long)k) {
                R.b[s] = k;
                if (s == (long long)a + 1) R.best_m[a] = 0;                      // and so does the one to its left; nobody reads it in this launch
            } else {
                R.a[s] = k;
            }
        }
        const unsigned long long all = __ballot(split);
        if (all && (threadIdx.x & 63) == 0) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&R.status->splits), (unsigned long long)__builtin_popcountll(all));
            atomicMax(reinterpret_cast<unsigned long long *>(&R.status->rounds), (unsigned long long)(round + 1));
        }
    }
}

// ===========================================================================
// the finish: per ring the kept count and both shoelace sums, the collapse rule, the vertices and the rows
// ===========================================================================
__global__ __launch_bounds__(256) void k_os_sums(OsRun R)
{
    const long long n = R.slots(), nq = R.N.rings(), span = (n + 63) / 64 * 64;
    const int lane = threadIdx.x & 63;
    for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < span; s += (long long)gridDim.x * 256) {     // wave-uniform
        unsigned int key = OS_NONE;
        long long kept = 0, kept_area = 0, own_area = 0;
        if (s < n && (long long)R.ring[s] < nq && !R.closing(s, n)) {
            key = R.ring[s];
            const unsigned int p = R.pts[s];
            own_area = os_area_term(p, R.pts[s + 1]);
            if (R.state[s] == OS_KEPT) {
                long long next = R.state[s + 1] == OS_KEPT ? s + 1 : (long long)R.b[s + 1];      // the next kept slot: the right end of what follows
                if (!(next > s && next < n)) next = s + 1;
                kept = 1;
                kept_area = os_area_term(p, R.pts[next]);
            }
        }
        if (!__any(key != OS_NONE)) continue;
        kept = os_seg_sum(kept, key, lane);
        kept_area = os_seg_sum(kept_area, key, lane);
        own_area = os_seg_sum(own_area, key, lane);
        if (os_seg_head(key, lane) && key != OS_NONE) {
            unsigned long long *acc = R.acc + 3 * (size_t)key;
            if (kept) atomicAdd(acc, (unsigned long long)kept);
            if (kept_area) atomicAdd(acc + 1, (unsigned long long)kept_area);
            if (own_area) atomicAdd(acc + 2, (unsigned long long)own_area);
        }
    }
}

// counts_out: [0] rings, [1] vertices written (the scan below), [2] rings that stay as given
__global__ __launch_bounds__(256) void k_os_decide(OsRun R, lars_outline_ring *__restrict__ rings_out, long long *__restrict__ counts_out)
{
    const long long nq = R.N.rings(), nv = R.N.verts(), span = (nq + 63) / 64 * 64;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts_out[0] = nq;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < span; i += (long long)gridDim.x * 256) {     // wave-uniform
        bool back = false;
        if (i < nq) {
            lars_outline_ring t = R.rings[i];
            const long long c = os_ring_verts(t, nv);
            const long long kept = (long long)R.acc[3 * (size_t)i], kept_area = (long long)R.acc[3 * (size_t)i + 1], own_area = (long long)R.acc[3 * (size_t)i + 2];
            back = c && (kept < 3 || kept_area == 0 || (kept_area > 0) != (own_area > 0));
            R.restored[i] = back ? 1 : 0;
            t.start = 0;                                                         // the scan places it
            t.count = (int32_t)(!c ? 0 : back ? c : kept);
            t.area2 = !c ? 0 : back ? own_area : kept_area;
            rings_out[i] = t;
        }
        const unsigned long long all = __ballot(back);
        if (all && (threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(counts_out + 2), (unsigned long long)__builtin_popcountll(all));
    }
}

// ---- the vertices written, in slot order: rings one after another ----
struct OsWrite {
    OsRun R;
    lars_outline_ring *rings_out;
    int32_t *verts_out;
    long long vert_capacity_out;
    __device__ long long count() const { return R.slots(); }
    __device__ unsigned int value(long long s) const
    {
        const unsigned int ring = R.ring[s];
        if ((long long)ring >= R.N.rings() || R.closing(s, R.slots())) return 0u;
        return R.restored[ring] || R.state[s] == OS_KEPT ? 1u : 0u;
    }
    __device__ void place(long long s, unsigned int written, unsigned int v) const
    {
        const unsigned int ring = R.ring[s];
        if ((long long)ring >= R.N.rings()) return;
        if ((long long)R.sbase[ring] == s) rings_out[ring].start = (int32_t)v;
        if (!written || (long long)v >= vert_capacity_out) return;
        verts_out[2 * (size_t)v] = (int32_t)os_row(R.pts[s]);
        verts_out[2 * (size_t)v + 1] = (int32_t)os_col(R.pts[s]);
    }
};

unsigned int os_grid(long long blocks) { return (unsigned int)(blocks < 1 ? 1 : blocks < 65536 ? blocks : 65536); }

template <typename Op>
void os_scan(const Op &op, long long nchunks, unsigned int *totals, long long *count_out, hipStream_t s)
{
    hipLaunchKernelGGL((k_os_totals<Op>), dim3(os_grid(nchunks)), dim3(256), 0, s, op, nchunks, totals);
    hipLaunchKernelGGL(k_os_scan_totals, dim3(1), dim3(1024), 0, s, totals, nchunks, count_out);
    hipLaunchKernelGGL((k_os_place<Op>), dim3(os_grid(nchunks)), dim3(256), 0, s, op, nchunks, totals);
}

bool os_room_ok(int64_t ring_capacity, int64_t vert_capacity)
{
    return ring_capacity >= 0 && vert_capacity >= 0 && ring_capacity <= OS_CAPACITY_MAX && vert_capacity <= OS_CAPACITY_MAX;
}

}  // namespace
}  // namespace lars

using namespace lars;

extern "C" size_t lars_outline_simplify_scratch_bytes(int64_t ring_capacity, int64_t vert_capacity)
{
    if (!os_room_ok(ring_capacity, vert_capacity)) return 0;
    Carver c(nullptr);
    OsBufs B(c, ring_capacity, vert_capacity);
    return c.bytes();
}

extern "C" int lars_d_outline_simplify(const lars_outline_ring *rings, int64_t ring_capacity, const int32_t *verts, int64_t vert_capacity,
                                       const int64_t *counts_dev, int64_t tq, int64_t h, int64_t w, lars_outline_ring *rings_out, int32_t *verts_out,
                                       int64_t vert_capacity_out, int64_t *counts_out_dev, void *scratch, int64_t *rounds_out, void *stream)
{
    static const char *who = "lars_d_outline_simplify";
    ThreadCtx *c;
    LARS_TRY(ensure_ctx(&c));
    if (rounds_out) *rounds_out = -1;
    if (h < 1 || w < 1 || h > OS_SIDE_MAX || w > OS_SIDE_MAX)
        return fail(LARS_ERR_INVALID, "%s: the raster is 1 to %d on each side (every product of coordinates fits 64 bits), got %lld x %lld", who, OS_SIDE_MAX,
                    (long long)h, (long long)w);
    if (tq < 1 || tq > OS_TQ_MAX) return fail(LARS_ERR_INVALID, "%s: tq must be 1 to %d sixteenths of a pixel, got %lld", who, OS_TQ_MAX, (long long)tq);
    if (!counts_dev || !counts_out_dev || !scratch || !os_room_ok(ring_capacity, vert_capacity) || vert_capacity_out < 0 || (ring_capacity > 0 && (!rings || !rings_out)) ||
        (vert_capacity > 0 && !verts) || (vert_capacity_out > 0 && !verts_out) || (rings && rings == rings_out) || (verts && verts == verts_out))
        return fail(LARS_ERR_INVALID, "%s: bad arguments (counts in and out, a scratch, ring tables and vertex arrays of capacity 0 to 2^31 - 1, "
                                      "the results apart from what is given)", who);
    if (!aligned_to(rings, 8) || !aligned_to(rings_out, 8) || !aligned_to(verts, 4) || !aligned_to(verts_out, 4) || !aligned_to(counts_dev, 8) ||
        !aligned_to(counts_out_dev, 8) || !aligned_to(scratch, 256))
        return fail(LARS_ERR_INVALID, "%s: verts must be 4-byte, rings and counts 8-byte and scratch 256-byte aligned", who);
    hipStream_t s = pick_stream(c, stream);
    Carver cv(scratch);
    const OsBufs B(cv, ring_capacity, vert_capacity);
    const OsCounts N = {reinterpret_cast<const long long *>(counts_dev), (long long)ring_capacity, (long long)vert_capacity};
    const OsRun R = {rings, verts, N, B.status, B.sbase, B.ring, B.pts, B.a, B.b, B.best_k, B.best_m, B.acc, B.state, B.restored, B.scap, (int)h, (int)w};
    long long *counts_out = reinterpret_cast<long long *>(counts_out_dev);
    const dim3 slot_grid(grid_1d(B.scap)), ring_grid(grid_1d(ring_capacity));
    LARS_HIP_TRY(hipMemsetAsync(B.status, 0, sizeof(OsStatus), s));
    LARS_HIP_TRY(hipMemsetAsync(counts_out_dev, 0, 3 * sizeof(int64_t), s));
    if (ring_capacity) LARS_HIP_TRY(hipMemsetAsync(B.acc, 0, 3 * (size_t)ring_capacity * sizeof(unsigned long long), s));
    os_scan(OsRingSlots{R}, B.ring_chunks, B.totals, &B.status->slots, s);
    hipLaunchKernelGGL(k_os_longest, ring_grid, dim3(256), 0, s, R);
    hipLaunchKernelGGL(k_os_init, slot_grid, dim3(256), 0, s, R);
    LARS_TRY(launch_check(who));
    // The hard bound before any round: the longest ring's vertex count.  A ring of n vertices has n - 1 slots inside its first stretch and
    // every round that splits one of its stretches keeps one of them, so it splits in its rounds 0 .. n - 2 at most.  No round beyond
    // `longest` is ever enqueued, whatever the status says afterwards, and a split in the last round allowed ends the call as an error.
    const unsigned long long tq2 = (unsigned long long)(tq * tq);
    OsStatus st;
    LARS_HIP_TRY(hipMemcpyAsync(&st, B.status, sizeof st, hipMemcpyDeviceToHost, s));
    LARS_HIP_TRY(hipStreamSynchronize(s));
    const long long longest = st.longest;
    if (longest < 0 || longest > (long long)vert_capacity || st.slots < 0 || st.slots > B.scap)
        return fail(LARS_ERR_HIP, "%s: the status words are damaged (%lld slots, the longest ring %lld)", who, st.slots, longest);
    // rounds, a batch at a time: the host learns from the status whether anything was split
    for (long long round = 0; round < longest;) {
        const long long batch = longest - round < OS_BATCH ? longest - round : OS_BATCH;
        LARS_HIP_TRY(hipMemsetAsync(&B.status->splits, 0, sizeof(long long), s));
        for (long long k = 0; k < batch; ++k, ++round) {
            hipLaunchKernelGGL(k_os_measure, slot_grid, dim3(256), 0, s, R);
            hipLaunchKernelGGL(k_os_pick, slot_grid, dim3(256), 0, s, R, tq2);
            hipLaunchKernelGGL(k_os_split, slot_grid, dim3(256), 0, s, R, round);
        }
        LARS_TRY(launch_check(who));
        LARS_HIP_TRY(hipMemcpyAsync(&st, B.status, sizeof st, hipMemcpyDeviceToHost, s));
        LARS_HIP_TRY(hipStreamSynchronize(s));
        if (st.splits < 0 || st.rounds < 0 || st.rounds > round) return fail(LARS_ERR_HIP, "%s: the status words are damaged", who);
        if (st.splits == 0) break;
    }
    if (longest > 0 && st.rounds >= longest)
        return fail(LARS_ERR_HIP, "%s: still splitting in round %lld; the longest ring has %lld vertices", who, st.rounds, longest);
    if (rounds_out) *rounds_out = st.rounds;
    hipLaunchKernelGGL(k_os_sums, slot_grid, dim3(256), 0, s, R);
    hipLaunchKernelGGL(k_os_decide, ring_grid, dim3(256), 0, s, R, rings_out, counts_out);
    os_scan(OsWrite{R, rings_out, verts_out, (long long)vert_capacity_out}, B.slot_chunks, B.totals, counts_out + 1, s);
    return launch_check(who);
}
