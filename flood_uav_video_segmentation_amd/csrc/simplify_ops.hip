// Outline simplification (include/floodseg_test.h: outline_simplify).  OUR DEFINITION -- the reference emits hard masks only.
// An opt-in pass behind region_outlines: nothing on the shipped routes calls it.
//   outline_simplify  contour rows + vertex lists -> per contour the Ramer-Douglas-Peucker subset of its ring within a tolerance, as rows
//                     (first offset, kept count, area2, flags) + concatenated kept vertices, per frame (rows, kept, rounds, flags)
// Integers throughout, and every result is a function of the inputs alone: a segment's farthest vertex is a 64-bit maximum and, among
// the vertices that hold it, a minimum of indices; the areas are integer sums.  The key, the test and the split rule are
// simplify_defs.h's (__host__ __device__, also run on the CPU by the tests).  The recursion is unrolled into rounds: all open segments
// of all contours of all frames are examined at once, two launches per round, max_rounds + 1 rounds fixed by the argument.  Every loop
// has a bound that follows from the arguments, stated at the loop; nothing waits on another workgroup, nothing is iterated until
// stable, nothing allocates or synchronises.  Every index read from the workspace or the rows is clamped before it is used.
#include "kernels.h"
#include "simplify_defs.h"

#include <algorithm>
#include <climits>

namespace fs {

namespace {

typedef unsigned long long u64;

// The workspace of one frame (simplify_defs.h, frame_words): cells, keys, maxima of both parities; then 32-bit arrays.
struct Space {
    u64 *seg, *key, *qmax;
    int *imin, *row, *orow, *chunk, *end, *hdr;
};
__device__ __forceinline__ Space space_of(u64* ws, int f, int C, int V) {
    u64* p = ws + (size_t)f * smp::frame_words(C, V);
    Space s;
    s.seg = p;
    s.key = p + V;
    s.qmax = p + 2 * (size_t)V;  // parity 0 [V], parity 1 [V]
    int* q = reinterpret_cast<int*>(p + 4 * (size_t)V);
    s.imin = q;  // parity 0 [V], parity 1 [V]
    s.row = q + 2 * (size_t)V;
    s.orow = q + 3 * (size_t)V;
    u64* r = p + 6 * (size_t)V;
    s.chunk = reinterpret_cast<int*>(r);
    s.end = reinterpret_cast<int*>(r + (smp::chunks(V) + 1) / 2);
    s.hdr = reinterpret_cast<int*>(r + (smp::chunks(V) + 1) / 2 + ((size_t)C + 1) / 2);
    return s;
}

__global__ __launch_bounds__(256) void simplify_zero_kernel(u64* __restrict__ a, size_t na, u64* __restrict__ b, size_t nb, u64* __restrict__ c, size_t nc) {
    const size_t all = na + nb + nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < all; i += (size_t)gridDim.x * 256) {  // bounded: the outputs' sizes
        if (i < na) a[i] = 0ull;
        else if (i < na + nb) b[i - na] = 0ull;
        else c[i - na - nb] = 0ull;
    }
}

// ---- sums across a workgroup: the exclusive scan of one count per thread; *all = the workgroup's sum.  part holds THREADS / 64 words.
template <int THREADS>
__device__ __forceinline__ u64 block_scan(u64 v, u64* part, u64* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    u64 before = inc - v, sum = 0;
    for (int w = 0; w < THREADS / 64; ++w) {  // bounded: the waves of a workgroup
        const u64 t = part[w];
        if (w < wave) before += t;
        sum += t;
    }
    __syncthreads();
    *all = sum;
    return before;
}

// Lanes with key >= 0 take part.  True when they all hold ONE key: *leader is then the first of them (-1: nobody takes part), and one
// atomic by the leader serves the wave.  Called by every lane of the wave.
__device__ __forceinline__ bool wave_one_key(int key, int* leader) {
    const u64 in = __ballot(key >= 0);
    *leader = in ? __ffsll((long long)in) - 1 : -1;
    const int first = __shfl(key, in ? *leader : 0);
    return __ballot(key >= 0 && key != first) == 0ull;
}

// ---- a contour as the later passes read it: its row, first vertex and vertex count, forced into the frame whatever the cells hold
struct Ring {
    int c, off, m;
};
__device__ __forceinline__ Ring ring_of(const long long* __restrict__ contours, int f, int C, int V, int c, int rows) {
    Ring g;
    g.c = smp::clamp_int(c, 0, rows - 1);  // rows >= 1 wherever a vertex is live
    const long long* row = contours + ((size_t)f * C + g.c) * 6;
    g.m = (int)std::min<long long>(std::max<long long>(row[2], 3), V);
    g.off = (int)std::min<long long>(std::max<long long>(row[1], 0), V - g.m);
    return g;
}
struct Pt {
    int x, y;
};
// vertex j of a ring (j = m is vertex 0 again), coordinates clamped
__device__ __forceinline__ Pt vertex_of(const int* __restrict__ vertices, int f, int V, const Ring& g, int j) {
    const int at = g.off + (j >= g.m ? 0 : j);  // < V: off + m <= V
    const int2 v = *reinterpret_cast<const int2*>(vertices + ((size_t)f * V + at) * 2);
    return Pt{smp::clamp_coord(v.x), smp::clamp_coord(v.y)};
}

// ------------------------------------------------------------------ pass 1: is the frame what region_outlines guarantees?
// One workgroup per frame.  The loop runs ceil(rows / 1024) <= 1024 times (rows <= max_contours <= 2^20).  A frame that fails gets no
// rows and no vertices under them (hdr), so no later pass touches it; its flag is decided here, on the device.
__global__ __launch_bounds__(1024) void simplify_validate_kernel(const long long* __restrict__ contours, const long long* __restrict__ counts, int C, int V,
                                                                 u64* ws) {
    __shared__ u64 part[16];
    __shared__ int bad;
    const int f = blockIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const long long* cnt = counts + 4 * (size_t)f;
    const long long found = cnt[0], rows = cnt[1], total = cnt[2], flags_in = cnt[3];
    if (threadIdx.x == 0) bad = 0;
    for (int k = threadIdx.x; k < smp::HDR_INTS; k += 1024) sp.hdr[k] = 0;
    __syncthreads();
    bool ok = !(flags_in & 1) && rows >= 0 && rows <= C && total <= V;  // the same for the whole workgroup
    u64 carry = 0;
    if (ok) {
        for (long long base = 0; base < rows; base += 1024) {
            const long long c = base + threadIdx.x;
            long long off = 0, m = 0;
            if (c < rows) {
                const long long* row = contours + ((size_t)f * C + c) * 6;
                off = row[1];
                m = row[2];
            }
            const bool fine = c >= rows || (m >= 3 && m <= V);
            u64 all;
            const u64 before = block_scan<1024>(c < rows && fine ? (u64)m : 0ull, part, &all);
            if (c < rows && (!fine || off != (long long)(carry + before))) bad = 1;  // every writer stores the same value
            carry += all;  // <= 2^20 * 2^22
        }
    }
    __syncthreads();
    ok = ok && !bad && (long long)carry <= total;
    if (threadIdx.x == 0) {
        sp.hdr[smp::HDR_ROWS] = ok ? (int)rows : 0;
        sp.hdr[smp::HDR_END] = ok ? (int)carry : 0;  // <= total <= V
        sp.hdr[smp::HDR_FLAGS] = (flags_in & 1) ? smp::FLAG_INPUT_OVERFLOW : (!ok ? smp::FLAG_INCONSISTENT : (found > rows ? smp::FLAG_INPUT_TRUNCATED : 0));
        sp.hdr[smp::HDR_OPEN] = ok && carry > 0;
    }
}

// ------------------------------------------------------------------ pass 2: every vertex's row; the first cells and slots
// One vertex per thread.  Its row is the last one whose offset is not behind it: a bisection of the rows' offsets, at most 21 steps
// (rows <= 2^20).  Vertex 0 of a ring is kept; every other one starts as an interior vertex of the whole ring (0, m).
__global__ __launch_bounds__(256) void simplify_init_kernel(const long long* __restrict__ contours, int C, int V, u64* ws) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int end = smp::clamp_int(sp.hdr[smp::HDR_END], 0, V), rows = smp::clamp_int(sp.hdr[smp::HDR_ROWS], 0, C);
    if (i >= end) return;
    const long long* table = contours + (size_t)f * C * 6;
    int lo = 0, hi = rows - 1;
    for (int step = 0; step < 21 && lo < hi; ++step) {  // bounded: the interval halves
        const int mid = (lo + hi + 1) >> 1;
        if (table[(size_t)mid * 6 + 1] <= i) lo = mid;
        else hi = mid - 1;
    }
    const Ring g = ring_of(contours, f, C, V, lo, rows);
    sp.row[i] = lo;
    sp.seg[i] = i == g.off ? smp::pack_seg(smp::KEPT, 0) : smp::pack_seg(0, g.m);
    sp.qmax[i] = 0ull;
    sp.imin[i] = INT_MAX;
}

// The cell of an open vertex after the split that round `round` decided for its segment (l, r); marks the round when it is the vertex
// that splits.  Cells, maxima and indices come from the workspace: l, r and s are forced into 0 <= l < s < r <= m.
__device__ __forceinline__ u64 apply_split(const Space& sp, const int* __restrict__ vertices, int f, int V, const Ring& g, int j, int l, int r, int round,
                                           int tol_q) {
    const size_t slot = (size_t)(round & 1) * V + g.off + l;
    const u64 q = sp.qmax[slot];
    const int s = smp::clamp_int(sp.imin[slot], l + 1, r - 1);
    const Pt a = vertex_of(vertices, f, V, g, l), b = vertex_of(vertices, f, V, g, r);
    const int64_t ux = b.x - a.x, uy = b.y - a.y;
    const bool split = smp::splits(round, (int64_t)std::min<u64>(q, (u64)1 << 58), ux * ux + uy * uy, tol_q);
    if (split && j == s) sp.hdr[smp::HDR_SPLIT + round] = 1;  // every writer stores the same value
    return smp::split_seg(l, r, j, split, s);
}
// an open cell's (l, r), forced into 0 <= l < r <= m with room for an interior vertex
__device__ __forceinline__ void open_bounds(u64 cell, int m, int* l, int* r) {
    *l = smp::clamp_int(smp::seg_l(cell), 0, m - 2);
    *r = smp::clamp_int(smp::seg_r(cell), *l + 2, m);
}

// ------------------------------------------------------------------ round k, launch A: take the split of round k - 1, measure
// One vertex per thread.  An open vertex first moves to its half of the segment round k - 1 split (or is settled), then computes its
// key against its segment and raises the segment's maximum: the slot is the segment's left vertex, in the buffer of the round's
// parity (cleared by launch B of the round before, read by launch A of the next one).  A wave whose open lanes share one segment --
// nearly all of them in the early rounds, when segments are long -- issues one atomic.  A frame without an open segment in the
// round before costs one early return.
__global__ __launch_bounds__(256) void simplify_measure_kernel(const long long* __restrict__ contours, const int* __restrict__ vertices, int C, int V, int tol_q,
                                                               int round, u64* ws) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int end = smp::clamp_int(sp.hdr[smp::HDR_END], 0, V), rows = smp::clamp_int(sp.hdr[smp::HDR_ROWS], 0, C);
    if ((int)(blockIdx.x * 256) >= end || !sp.hdr[smp::HDR_OPEN + (round ? round - 1 : 0)]) return;  // the whole workgroup
    int slot = -1;
    u64 q = 0;
    if (i < end) {
        u64 cell = sp.seg[i];
        if (smp::seg_l(cell) >= 0) {
            const Ring g = ring_of(contours, f, C, V, sp.row[i], rows);
            const int j = smp::clamp_int(i - g.off, 1, g.m - 1);
            int l, r;
            open_bounds(cell, g.m, &l, &r);
            if (round > 0) {
                cell = apply_split(sp, vertices, f, V, g, j, l, r, round - 1, tol_q);
                sp.seg[i] = cell;
            }
            if (smp::seg_l(cell) >= 0) {
                open_bounds(cell, g.m, &l, &r);
                const Pt a = vertex_of(vertices, f, V, g, l), b = vertex_of(vertices, f, V, g, r), p = vertex_of(vertices, f, V, g, j);
                int64_t L;
                q = (u64)smp::seg_key(a.x, a.y, b.x, b.y, p.x, p.y, &L);
                sp.key[i] = q;
                sp.hdr[smp::HDR_OPEN + round] = 1;  // every writer stores the same value
                if (q) slot = g.off + l;             // a key of 0 is what the slot holds already
            }
        }
    }
    u64* qmax = sp.qmax + (size_t)(round & 1) * V;
    int leader;
    if (wave_one_key(slot, &leader)) {
        u64 m = slot >= 0 ? q : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = std::max<u64>(m, __shfl_xor(m, d));
        if ((int)(threadIdx.x & 63) == leader) atomicMax(&qmax[slot], m);
    } else if (slot >= 0) {
        atomicMax(&qmax[slot], q);
    }
}

// ------------------------------------------------------------------ round k, launch B: the smallest index among the farthest
// One vertex per thread: an open vertex whose key is its segment's maximum offers its index.  Every vertex clears its own slot of the
// other parity for the next round.
__global__ __launch_bounds__(256) void simplify_pick_kernel(const long long* __restrict__ contours, int C, int V, int round, u64* ws) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int end = smp::clamp_int(sp.hdr[smp::HDR_END], 0, V), rows = smp::clamp_int(sp.hdr[smp::HDR_ROWS], 0, C);
    if (i >= end || !sp.hdr[smp::HDR_OPEN + round]) return;
    const size_t mine = (size_t)(round & 1) * V, other = (size_t)(~round & 1) * V;
    const u64 cell = sp.seg[i];
    if (smp::seg_l(cell) >= 0) {
        const Ring g = ring_of(contours, f, C, V, sp.row[i], rows);
        int l, r;
        open_bounds(cell, g.m, &l, &r);
        if (sp.key[i] == sp.qmax[mine + g.off + l]) atomicMin(&sp.imin[mine + g.off + l], smp::clamp_int(i - g.off, 1, g.m - 1));
    }
    sp.qmax[other + i] = 0ull;
    sp.imin[other + i] = INT_MAX;
}

// ------------------------------------------------------------------ the closing pass: the last round's split; what is open stays
// One vertex per thread.  A vertex still open after the last round is kept, and its contour and frame are flagged unconverged.
__global__ __launch_bounds__(256) void simplify_close_kernel(const long long* __restrict__ contours, const int* __restrict__ vertices, int C, int V, int tol_q,
                                                             int last, u64* ws, long long* __restrict__ simple) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int end = smp::clamp_int(sp.hdr[smp::HDR_END], 0, V), rows = smp::clamp_int(sp.hdr[smp::HDR_ROWS], 0, C);
    if (i >= end || !sp.hdr[smp::HDR_OPEN + last]) return;
    u64 cell = sp.seg[i];
    if (smp::seg_l(cell) < 0) return;
    const Ring g = ring_of(contours, f, C, V, sp.row[i], rows);
    int l, r;
    open_bounds(cell, g.m, &l, &r);
    cell = apply_split(sp, vertices, f, V, g, smp::clamp_int(i - g.off, 1, g.m - 1), l, r, last, tol_q);
    if (smp::seg_l(cell) >= 0) {
        cell = smp::pack_seg(smp::KEPT, 0);
        simple[((size_t)f * C + g.c) * 4 + 3] = 1;  // every writer stores the same value
        sp.hdr[smp::HDR_UNCONVERGED] = 1;
    }
    sp.seg[i] = cell;
}

__device__ __forceinline__ u64 kept_at(const Space& sp, int i, int end) { return i < end && smp::seg_l(sp.seg[i]) == smp::KEPT ? 1ull : 0ull; }

// ------------------------------------------------------------------ scan 1: the kept vertices per chunk of 1024
__global__ __launch_bounds__(1024) void simplify_count_kernel(int C, int V, u64* ws) {
    __shared__ u64 part[16];
    const Space sp = space_of(ws, blockIdx.y, C, V);
    const int end = smp::clamp_int(sp.hdr[smp::HDR_END], 0, V);
    u64 all;
    block_scan<1024>(kept_at(sp, blockIdx.x * smp::CHUNK + threadIdx.x, end), part, &all);
    if (threadIdx.x == 0) sp.chunk[blockIdx.x] = (int)all;
}

// ------------------------------------------------------------------ scan 2: the chunks' offsets; the frame's counts
// One workgroup per frame: ceil(chunks / 1024) <= 4 rounds of the loop.  rounds = the largest round that split a segment.
__global__ __launch_bounds__(1024) void simplify_counts_kernel(int C, int V, int last, u64* ws, long long* __restrict__ simple_counts) {
    __shared__ u64 part[16];
    __shared__ int rounds;
    const int f = blockIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int chunks = (int)smp::chunks(V);
    if (threadIdx.x == 0) rounds = 0;
    u64 carry = 0;
    for (int base = 0; base < chunks; base += 1024) {
        const int c = base + threadIdx.x;
        const u64 v = c < chunks ? (u64)(unsigned)sp.chunk[c] : 0ull;
        u64 all;
        const u64 before = block_scan<1024>(v, part, &all);  // its barriers also order `rounds = 0` before the maxima below
        if (c < chunks) sp.chunk[c] = (int)(carry + before);
        carry += all;
    }
    if ((int)threadIdx.x <= last && sp.hdr[smp::HDR_SPLIT + threadIdx.x]) atomicMax(&rounds, (int)threadIdx.x);  // last <= 256 < 1024
    __syncthreads();
    if (threadIdx.x == 0) {
        sp.hdr[smp::HDR_KEPT] = (int)carry;
        long long* out = simple_counts + 4 * (size_t)f;
        out[0] = sp.hdr[smp::HDR_ROWS];
        out[1] = (long long)carry;
        out[2] = rounds;
        out[3] = sp.hdr[smp::HDR_FLAGS] | (sp.hdr[smp::HDR_UNCONVERGED] ? smp::FLAG_UNCONVERGED : 0);
    }
}

// ------------------------------------------------------------------ scatter: the kept vertices in input order; every ring's place
// The exclusive scan of the kept flags inside the chunk on top of the chunk's offset is a kept vertex's place.  The rings lie back to
// back in row order, so vertex 0 of a ring (always kept) holds the ring's first offset and its last vertex the ring's end.
__global__ __launch_bounds__(1024) void simplify_scatter_kernel(const long long* __restrict__ contours, const int* __restrict__ vertices, int C, int V, u64* ws,
                                                                long long* __restrict__ simple, int* __restrict__ simple_vertices) {
    __shared__ u64 part[16];
    const int f = blockIdx.y, i = blockIdx.x * smp::CHUNK + threadIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int end = smp::clamp_int(sp.hdr[smp::HDR_END], 0, V), rows = smp::clamp_int(sp.hdr[smp::HDR_ROWS], 0, C);
    if ((int)(blockIdx.x * smp::CHUNK) >= end) return;  // the whole workgroup
    const u64 kept = kept_at(sp, i, end);
    u64 all;
    const int at = sp.chunk[blockIdx.x] + (int)block_scan<1024>(kept, part, &all);
    if (i >= end || at < 0 || at + (int)kept > V) return;
    const Ring g = ring_of(contours, f, C, V, sp.row[i], rows);
    const int j = i - g.off;
    if (kept) {
        const Pt p = vertex_of(vertices, f, V, g, smp::clamp_int(j, 0, g.m - 1));
        *reinterpret_cast<int2*>(simple_vertices + ((size_t)f * V + at) * 2) = make_int2(p.x, p.y);
        sp.orow[at] = g.c;
    }
    if (j == 0) simple[((size_t)f * C + g.c) * 4] = at;
    if (j == g.m - 1) sp.end[g.c] = at + (int)kept;
}

// ------------------------------------------------------------------ the kept rings' counts and areas
// One kept vertex per thread: its term x0 y1 - x1 y0 with the next kept vertex of its ring goes to the ring's row.  A wave whose
// vertices share one ring adds once.  Integer sums do not depend on the order of arrival.
__global__ __launch_bounds__(256) void simplify_area_kernel(int C, int V, u64* ws, long long* __restrict__ simple, const int* __restrict__ simple_vertices) {
    const int f = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, C, V);
    const int kept = smp::clamp_int(sp.hdr[smp::HDR_KEPT], 0, V), rows = smp::clamp_int(sp.hdr[smp::HDR_ROWS], 0, C);
    if ((int)(blockIdx.x * 256) >= kept) return;  // the whole workgroup
    int c = -1;
    long long term = 0;
    if (p < kept) {
        c = smp::clamp_int(sp.orow[p], 0, rows - 1);
        long long* row = simple + ((size_t)f * C + c) * 4;
        const int first = (int)std::min<long long>(std::max<long long>(row[0], 0), p);
        const int last = smp::clamp_int(sp.end[c], p + 1, kept);
        const int next = p + 1 < last ? p + 1 : first;
        const int2 v0 = *reinterpret_cast<const int2*>(simple_vertices + ((size_t)f * V + p) * 2);
        const int2 v1 = *reinterpret_cast<const int2*>(simple_vertices + ((size_t)f * V + next) * 2);
        term = (long long)v0.x * v1.y - (long long)v1.x * v0.y;
        if (p == first) row[1] = last - first;
    }
    u64* area = reinterpret_cast<u64*>(simple) + (size_t)f * C * 4 + 2;
    int leader;
    if (wave_one_key(c, &leader)) {
        u64 sum = (u64)term;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&area[(size_t)c * 4], sum);
    } else if (c >= 0) {
        atomicAdd(&area[(size_t)c * 4], (u64)term);
    }
}

}  // namespace

int launch_outline_simplify(const long long* contours, const int* vertices, const long long* counts, int n, int max_contours, int max_vertices, int tol_q,
                            int max_rounds, long long* simple, int* simple_vertices, long long* simple_counts, void* workspace, hipStream_t s) {
    FS_REQUIRE(contours && vertices && counts && simple && simple_vertices && simple_counts && workspace, "outline_simplify: null pointer");
    FS_REQUIRE(n >= 1 && n <= 65535, "outline_simplify: n=%d frames out of range (1..65535)", n);
    FS_REQUIRE(max_contours >= 1 && max_contours <= smp::MAX_CONTOURS, "outline_simplify: max_contours=%d out of range (1..2^20)", max_contours);
    FS_REQUIRE(max_vertices >= smp::MIN_VERTICES && max_vertices <= smp::MAX_VERTICES, "outline_simplify: max_vertices=%d out of range (4..2^22)",
               max_vertices);
    FS_REQUIRE(tol_q >= 0 && tol_q <= smp::MAX_TOL_Q, "outline_simplify: tol_q=%d out of range (0..2^20)", tol_q);
    FS_REQUIRE(max_rounds >= 1 && max_rounds <= smp::MAX_ROUNDS, "outline_simplify: max_rounds=%d out of range (1..256)", max_rounds);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "outline_simplify: the workspace is not aligned to 8 bytes");
    u64* ws = static_cast<u64*>(workspace);
    const int C = max_contours, V = max_vertices;
    const unsigned chunks = (unsigned)smp::chunks(V), blocks = (unsigned)cdiv(V, 256), frames = (unsigned)n;
    const size_t zs = (size_t)n * C * 4, zv = (size_t)n * V, zn = (size_t)n * 4;
    hipLaunchKernelGGL(simplify_zero_kernel, dim3((unsigned)std::min<size_t>((zs + zv + zn + 255) / 256, 1u << 16)), dim3(256), 0, s,
                       reinterpret_cast<u64*>(simple), zs, reinterpret_cast<u64*>(simple_vertices), zv, reinterpret_cast<u64*>(simple_counts), zn);
    hipLaunchKernelGGL(simplify_validate_kernel, dim3(frames), dim3(1024), 0, s, contours, counts, C, V, ws);
    hipLaunchKernelGGL(simplify_init_kernel, dim3(blocks, frames), dim3(256), 0, s, contours, C, V, ws);
    for (int k = 0; k <= max_rounds; ++k) {  // round 0 finds the vertex farthest from the anchor; rounds 1 .. max_rounds <= 256 test
        hipLaunchKernelGGL(simplify_measure_kernel, dim3(blocks, frames), dim3(256), 0, s, contours, vertices, C, V, tol_q, k, ws);
        hipLaunchKernelGGL(simplify_pick_kernel, dim3(blocks, frames), dim3(256), 0, s, contours, C, V, k, ws);
    }
    hipLaunchKernelGGL(simplify_close_kernel, dim3(blocks, frames), dim3(256), 0, s, contours, vertices, C, V, tol_q, max_rounds, ws, simple);
    hipLaunchKernelGGL(simplify_count_kernel, dim3(chunks, frames), dim3(1024), 0, s, C, V, ws);
    hipLaunchKernelGGL(simplify_counts_kernel, dim3(frames), dim3(1024), 0, s, C, V, max_rounds, ws, simple_counts);
    hipLaunchKernelGGL(simplify_scatter_kernel, dim3(chunks, frames), dim3(1024), 0, s, contours, vertices, C, V, ws, simple, simple_vertices);
    hipLaunchKernelGGL(simplify_area_kernel, dim3(blocks, frames), dim3(256), 0, s, C, V, ws, simple, simple_vertices);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
