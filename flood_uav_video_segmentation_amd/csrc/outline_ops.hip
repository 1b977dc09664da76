// Region outlines (include/floodseg_test.h: region_outlines).  OUR DEFINITION -- the reference emits hard masks only.
// An opt-in pass behind region_table: nothing on the shipped routes calls it.
//   region_outlines  index planes -> per frame the ordered contours of every region (table + concatenated vertex lists), per region its
//                    perimeter, contour and vertex counts, per frame the totals and two overflow flags
// Integers throughout, and every result is a function of the inputs alone: the nodes (run starts) are compacted in slot order, a
// contour's anchor is a minimum, its vertices' places are distances along the contour, and the sums are integer sums.  The slot
// packing, the successor rule and the ranking cell are outline_defs.h's (__host__ __device__, also run on the CPU by the tests).
// Every loop has a bound that follows from the arguments, stated at the loop; nothing waits on another workgroup, nothing is iterated
// until stable, nothing allocates or synchronises.  Global atomics are issued per run of equal rows in a wave (the shape sums), per
// run of cracks (a contour's length and area) or per contour -- never per pixel.
#include "kernels.h"
#include "outline_defs.h"

#include <algorithm>

namespace fs {

namespace {

typedef unsigned long long u64;

// The workspace of one frame, in 8-byte words (V = max_vertices, P = ceil(V / 2), PC = pixel chunks, NC = node chunks):
//   rank cells A, B [V] each; then the 32-bit arrays slot, next, jump A, jump B, len, crank, coff [2 P] each; the pixel chunks' run-start
//   counts [PC, padded to even]; the node chunks' (contours << 32 | vertices) sums [NC] as words; four 32-bit figures (run starts in the
//   frame, nodes = the same or 0 when they do not fit, two spare).
struct Space {
    u64 *val_a, *val_b, *nchunk;
    int *slot, *next, *jump_a, *jump_b, *len, *crank, *coff, *pchunk, *hdr;
};
__host__ __device__ inline size_t pixel_chunks(int H, int W) { return ((size_t)H * W + otl::CHUNK - 1) / otl::CHUNK; }
__host__ __device__ inline size_t node_chunks(int V) { return ((size_t)V + otl::CHUNK - 1) / otl::CHUNK; }
__host__ __device__ inline size_t frame_words(int H, int W, int V) {
    return 2 * (size_t)V + 7 * (((size_t)V + 1) / 2) + (pixel_chunks(H, W) + 1) / 2 + node_chunks(V) + 2;
}
__device__ __forceinline__ Space space_of(u64* ws, int f, int H, int W, int V) {
    u64* p = ws + (size_t)f * frame_words(H, W, V);
    const size_t P = ((size_t)V + 1) / 2;
    Space s;
    s.val_a = p;
    s.val_b = p + V;
    int* q = reinterpret_cast<int*>(p + 2 * (size_t)V);
    s.slot = q;
    s.next = q + 2 * P;
    s.jump_a = q + 4 * P;
    s.jump_b = q + 6 * P;
    s.len = q + 8 * P;
    s.crank = q + 10 * P;
    s.coff = q + 12 * P;
    s.pchunk = q + 14 * P;
    u64* r = p + 2 * (size_t)V + 7 * P + (pixel_chunks(H, W) + 1) / 2;
    s.nchunk = r;
    s.hdr = reinterpret_cast<int*>(r + node_chunks(V));
    return s;
}

__global__ __launch_bounds__(256) void outline_zero_kernel(u64* __restrict__ a, size_t na, u64* __restrict__ b, size_t nb, u64* __restrict__ c, size_t nc,
                                                           u64* __restrict__ d, size_t nd) {
    const size_t all = na + nb + nc + nd;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < all; i += (size_t)gridDim.x * 256) {  // bounded: the outputs' sizes
        if (i < na) a[i] = 0ull;
        else if (i < na + nb) b[i - na] = 0ull;
        else if (i < na + nb + nc) c[i - na - nb] = 0ull;
        else d[i - na - nb - nc] = 0ull;
    }
}

// ---- sums across a workgroup.  wave_scan: the inclusive scan of one 64-bit value per lane (6 shuffles).
__device__ __forceinline__ u64 wave_scan(u64 v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
// The exclusive scan of one value per thread over a workgroup of THREADS; *all = the workgroup's sum.  part holds THREADS / 64 words.
template <int THREADS>
__device__ __forceinline__ u64 block_scan(u64 v, u64* part, u64* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 inc = wave_scan(v, lane);
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

// the cracks and run starts of pixel i of a plane: row (-1: none), crack bits, run-start bits
__device__ __forceinline__ int pixel_bits(const otl::Plane& p, int i, unsigned* cracks, unsigned* starts) {
    const int y = i / p.W, x = i - y * p.W;
    const int r = p.at(x, y);
    *cracks = *starts = 0u;
    if (r >= 0) {
        const unsigned same = otl::same_bits(p, x, y, r);
        *cracks = otl::crack_bits(same);
        *starts = otl::start_bits(same);
    }
    return r;
}

// ------------------------------------------------------------------ pass 1: count the run starts per chunk; the local shape sums
// grid = (pixel chunks, frames).  Thread t owns chunk pixels t, t + 256, ...: a wave is 64 consecutive pixels in raster order.  Runs of
// equal row inside the wave are summed across lanes by one inclusive wave scan of (cracks | run starts << 16) (at most 256 each), and
// the run's first lane adds them to the row's perimeter and vertices: two atomics per run, not per pixel.
__global__ __launch_bounds__(256) void outline_mark_kernel(const int* __restrict__ index, int H, int W, int R, int V, u64* ws, u64* __restrict__ shape) {
    __shared__ u64 part[4];
    const int f = blockIdx.y, HW = H * W, lane = threadIdx.x & 63;
    const otl::Plane p = {index + (size_t)f * HW, H, W, R};
    const int begin = blockIdx.x * otl::CHUNK;  // < HW (grid)
    unsigned mine = 0;
    for (int k = 0; k < otl::CHUNK / 256; ++k) {
        const int i = begin + k * 256 + threadIdx.x;  // < HW + 1024 <= 2^29 + 1024
        unsigned cracks = 0, starts = 0;
        const int r = i < HW ? pixel_bits(p, i, &cracks, &starts) : -2;
        mine += __popc(starts);
        const unsigned packed = (unsigned)wave_scan((u64)(__popc(cracks) | __popc(starts) << 16), lane);
        const int prev = __shfl_up(r, 1);
        const u64 heads = __ballot(lane == 0 || prev != r);
        const u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int end = above ? __ffsll((long long)above) - 1 : 64;  // the run of a head lane is [lane, end)
        const unsigned upto = __shfl(packed, end - 1), before = __shfl_up(packed, 1);
        const unsigned run = upto - (lane == 0 ? 0u : before);
        if (((heads >> lane) & 1ull) && r >= 0 && run) {
            u64* row = shape + ((size_t)f * R + r) * 3;
            atomicAdd(&row[0], (u64)(run & 0xFFFFu));
            if (run >> 16) atomicAdd(&row[2], (u64)(run >> 16));
        }
    }
    u64 all;
    block_scan<256>((u64)mine, part, &all);
    if (threadIdx.x == 0) space_of(ws, f, H, W, V).pchunk[blockIdx.x] = (int)all;
}

// ------------------------------------------------------------------ pass 2: the chunk counts become exclusive offsets in place
// One workgroup per frame.  The loop runs ceil(pixel chunks / 1024) <= 512 times (H W < 2^29).  hdr = (run starts, nodes): the frame's
// nodes are its run starts when they fit max_vertices, else none -- flag bit 0, decided here, on the device.
__global__ __launch_bounds__(1024) void outline_offsets_kernel(int H, int W, int V, u64* ws) {
    __shared__ u64 part[16];
    const Space sp = space_of(ws, blockIdx.x, H, W, V);
    const int chunks = (int)pixel_chunks(H, W);
    u64 carry = 0;
    for (int base = 0; base < chunks; base += 1024) {
        const int c = base + threadIdx.x;
        const u64 v = c < chunks ? (u64)(unsigned)sp.pchunk[c] : 0ull;
        u64 all;
        const u64 before = block_scan<1024>(v, part, &all);
        if (c < chunks) sp.pchunk[c] = (int)(carry + before);  // <= 4 H W < 2^31
        carry += all;
    }
    if (threadIdx.x == 0) {
        sp.hdr[0] = (int)carry;
        sp.hdr[1] = carry <= (u64)V ? (int)carry : 0;
        sp.hdr[2] = sp.hdr[3] = 0;
    }
}

// ------------------------------------------------------------------ pass 3: the run starts in slot order = the node list
// grid = (pixel chunks, frames).  Thread t owns the chunk's pixels 4 t .. 4 t + 3, that is 16 consecutive slots, so an exclusive scan of
// the threads' counts on top of the chunk's offset places every run start in ascending slot order.
__global__ __launch_bounds__(256) void outline_compact_kernel(const int* __restrict__ index, int H, int W, int R, int V, u64* ws) {
    __shared__ u64 part[4];
    const int f = blockIdx.y, HW = H * W;
    const Space sp = space_of(ws, f, H, W, V);
    if (sp.hdr[1] == 0) return;  // nothing to list, or too much: the same for the whole workgroup
    const otl::Plane p = {index + (size_t)f * HW, H, W, R};
    const int first = blockIdx.x * otl::CHUNK + 4 * threadIdx.x;
    unsigned bits = 0;  // the run-start bits of the four pixels, 4 bits each
    for (int k = 0; k < 4; ++k) {
        unsigned cracks, starts;
        if (first + k < HW) {
            pixel_bits(p, first + k, &cracks, &starts);
            bits |= starts << (4 * k);
        }
    }
    u64 all;
    int at = sp.pchunk[blockIdx.x] + (int)block_scan<256>((u64)__popc(bits), part, &all);
    for (int b = 0; b < 16; ++b) {
        if (bits >> b & 1u) {
            if (at < V) sp.slot[at] = 4 * first + b;  // always: the frame's run starts fit V (hdr[1] != 0)
            ++at;
        }
    }
}

// ------------------------------------------------------------------ pass 4: every node's next node
// One node per thread.  A straight walk of at most max(H, W) cracks (outline_defs.h, next_run_start) ends on the next run start; its
// node is found by bisection of the sorted slot list, at most 23 steps (V <= 2^22).  next is a permutation of the nodes, so the
// scatter jump[next] = node gives every node its predecessor without a conflict; the ranking cell starts as (node, 0 steps).
__global__ __launch_bounds__(256) void outline_link_kernel(const int* __restrict__ index, int H, int W, int R, int V, int connectivity, u64* ws) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, H, W, V);
    const int m = sp.hdr[1];
    if (i >= m) return;
    const otl::Plane p = {index + (size_t)f * H * W, H, W, R};
    const int target = otl::next_run_start(p, sp.slot[i], connectivity);
    int lo = 0, hi = m - 1;
    for (int step = 0; step < 32 && lo < hi; ++step) {  // bounded: the interval halves
        const int mid = (lo + hi) >> 1;
        if (sp.slot[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    sp.next[i] = lo;
    sp.jump_a[lo] = i;
    sp.val_a[i] = otl::pack_rank((uint32_t)i, 0u);
}

// ------------------------------------------------------------------ pass 5: ranking by pointer jumping, one launch per round
// Before round k a node's cell covers the 2^k nodes that end at it and its jump names the node 2^k back; the round joins the cell with
// the jump's cell and doubles the jump, from one buffer into the other.  ceil(log2 V) rounds, fixed by the cap: a contour has at most
// V nodes, so afterwards every cell holds the contour's smallest node -- its anchor -- and the node's steps behind it.
__global__ __launch_bounds__(256) void outline_jump_kernel(int H, int W, int V, int round, u64* ws) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, H, W, V);
    const int m = sp.hdr[1];
    if (i >= m) return;
    const bool odd = round & 1;
    const u64* vin = odd ? sp.val_b : sp.val_a;
    u64* vout = odd ? sp.val_a : sp.val_b;
    const int* jin = odd ? sp.jump_b : sp.jump_a;
    int* jout = odd ? sp.jump_a : sp.jump_b;
    const int j = min(max(jin[i], 0), m - 1);  // a node of this frame whatever the cell holds
    vout[i] = otl::join_rank(vin[i], vin[j], 1u << round);
    jout[i] = min(max(jin[j], 0), m - 1);
}

// the buffer the last ranking round wrote (by value: a reference would put the whole Space into scratch)
__device__ __forceinline__ const u64* ranked(const u64* val_a, const u64* val_b, int rounds) { return rounds & 1 ? val_b : val_a; }
__device__ __forceinline__ int anchor_of(u64 cell, int m) { return min((int)otl::rank_node(cell), m - 1); }

// ------------------------------------------------------------------ pass 6: a contour's vertex count, written by its last node
__global__ __launch_bounds__(256) void outline_length_kernel(int H, int W, int V, int rounds, u64* ws) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, H, W, V);
    const int m = sp.hdr[1];
    if (i >= m) return;
    const u64 cell = ranked(sp.val_a, sp.val_b, rounds)[i];
    const int a = anchor_of(cell, m);
    if (sp.next[i] == a) sp.len[a] = (int)otl::rank_steps(cell) + 1;
}

// what a node adds to the scan over the nodes: an anchor counts one contour (high half) and its contour's vertices (low half)
__device__ __forceinline__ u64 anchor_weight(const u64* __restrict__ val, const int* __restrict__ len, int i, int m) {
    if (i >= m || anchor_of(val[i], m) != i) return 0ull;
    return 1ull << 32 | (u64)(unsigned)min(max(len[i], 0), m);
}

// ------------------------------------------------------------------ pass 7: per chunk of 1024 nodes the contours and their vertices
__global__ __launch_bounds__(1024) void outline_anchor_count_kernel(int H, int W, int V, int rounds, u64* ws) {
    __shared__ u64 part[16];
    const Space sp = space_of(ws, blockIdx.y, H, W, V);
    u64 all;
    block_scan<1024>(anchor_weight(ranked(sp.val_a, sp.val_b, rounds), sp.len, blockIdx.x * otl::CHUNK + threadIdx.x, sp.hdr[1]), part, &all);
    if (threadIdx.x == 0) sp.nchunk[blockIdx.x] = all;
}

// ------------------------------------------------------------------ pass 8: the node chunks' offsets; the frame's counts
// One workgroup per frame: ceil(node chunks / 1024) <= 4 rounds of the first loop, ceil(R / 1024) <= 64 of the second, which runs for an
// overflowing frame only and marks the contours column of every row that has cracks with -1.
__global__ __launch_bounds__(1024) void outline_counts_kernel(int H, int W, int R, int V, int max_contours, u64* ws, long long* __restrict__ shape,
                                                              long long* __restrict__ counts) {
    __shared__ u64 part[16];
    const int f = blockIdx.x;
    const Space sp = space_of(ws, f, H, W, V);
    const int chunks = (int)node_chunks(V);
    u64 carry = 0;
    for (int base = 0; base < chunks; base += 1024) {
        const int c = base + threadIdx.x;
        const u64 v = c < chunks ? sp.nchunk[c] : 0ull;
        u64 all;
        const u64 before = block_scan<1024>(v, part, &all);
        if (c < chunks) sp.nchunk[c] = carry + before;
        carry += all;
    }
    const int total = sp.hdr[0];
    const bool overflow = total > V;
    if (threadIdx.x == 0) {
        const long long contours = (long long)(carry >> 32);
        long long* out = counts + 4 * (size_t)f;
        out[0] = overflow ? 0 : contours;
        out[1] = overflow ? 0 : min(contours, (long long)max_contours);
        out[2] = total;
        out[3] = overflow ? 1 : (contours > max_contours ? 2 : 0);
    }
    if (overflow) {
        for (int r = threadIdx.x; r < R; r += 1024) {
            long long* row = shape + ((size_t)f * R + r) * 3;
            if (row[0] > 0) row[1] = -1;
        }
    }
}

// ------------------------------------------------------------------ pass 9: every contour's row and place
// The exclusive scan of the anchors' weights inside the chunk on top of the chunk's offset is (contours before, vertices before): the
// contour's row and its first vertex offset.  Both are kept per anchor for pass 10; the first max_contours contours get their rows'
// columns 0, 1, 2 and 5 here, and every contour counts once for its region (one atomic per contour).
__global__ __launch_bounds__(1024) void outline_place_kernel(const int* __restrict__ index, int H, int W, int R, int V, int max_contours, int rounds, u64* ws,
                                                             long long* __restrict__ contours, u64* __restrict__ shape) {
    __shared__ u64 part[16];
    const int f = blockIdx.y, i = blockIdx.x * otl::CHUNK + threadIdx.x;
    const Space sp = space_of(ws, f, H, W, V);
    const int m = sp.hdr[1];
    if (m == 0) return;  // the whole workgroup
    const u64 w = anchor_weight(ranked(sp.val_a, sp.val_b, rounds), sp.len, i, m);
    u64 all;
    const u64 at = sp.nchunk[blockIdx.x] + block_scan<1024>(w, part, &all);
    if (!w) return;
    const int c = (int)(at >> 32), off = (int)(at & 0xFFFFFFFFu);
    sp.crank[i] = c;
    sp.coff[i] = off;
    int x, y, d;
    const int slot = sp.slot[i];
    otl::unpack_slot(slot, W, &x, &y, &d);
    const otl::Plane p = {index + (size_t)f * H * W, H, W, R};
    const int r = p.at(x, y);
    if (r >= 0) atomicAdd(&shape[((size_t)f * R + r) * 3 + 1], 1ull);
    if (c < max_contours) {
        long long* row = contours + ((size_t)f * max_contours + c) * 6;
        row[0] = r;
        row[1] = off;
        row[2] = (long long)(w & 0xFFFFFFFFu);
        row[5] = slot;
    }
}

// ------------------------------------------------------------------ pass 10: the vertices; a contour's length and area
// One node per thread: its vertex goes to its contour's offset + its steps behind the anchor.  The node is one straight run of cracks from
// its vertex to the next node's: the run's length and its term x0 y1 - x1 y0 are added to the contour's row, two atomics per run.
__global__ __launch_bounds__(256) void outline_scatter_kernel(int H, int W, int V, int max_contours, int rounds, u64* ws, int* __restrict__ vertices,
                                                              u64* __restrict__ contours) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const Space sp = space_of(ws, f, H, W, V);
    const int m = sp.hdr[1];
    if (i >= m) return;
    const u64 cell = ranked(sp.val_a, sp.val_b, rounds)[i];
    const int a = anchor_of(cell, m);
    const int c = sp.crank[a], at = sp.coff[a] + (int)otl::rank_steps(cell);
    int x, y, d, x0, y0, x1, y1;
    otl::unpack_slot(sp.slot[i], W, &x, &y, &d);
    otl::start_corner(x, y, d, &x0, &y0);
    otl::unpack_slot(sp.slot[min(max(sp.next[i], 0), m - 1)], W, &x, &y, &d);
    otl::start_corner(x, y, d, &x1, &y1);
    if (at >= 0 && at < V) {
        int* v = vertices + ((size_t)f * V + at) * 2;
        v[0] = x0;
        v[1] = y0;
    }
    if (c >= 0 && c < max_contours) {
        u64* row = contours + ((size_t)f * max_contours + c) * 6;
        atomicAdd(&row[3], (u64)(abs(x1 - x0) + abs(y1 - y0)));
        atomicAdd(&row[4], (u64)((long long)x0 * y1 - (long long)x1 * y0));
    }
}

}  // namespace

int launch_region_outlines(const int* index, int n, int H, int W, int max_regions, int connectivity, int max_contours, int max_vertices,
                           long long* contours, int* vertices, long long* shape, long long* counts, void* workspace, hipStream_t s) {
    FS_REQUIRE(index && contours && vertices && shape && counts && workspace, "region_outlines: null pointer");
    FS_REQUIRE(n >= 1 && H >= 1 && W >= 1, "region_outlines: sizes must be >= 1, got n=%d %dx%d", n, H, W);
    FS_REQUIRE(n <= 65535, "region_outlines: at most 65535 frames, got n=%d", n);
    FS_REQUIRE((int64_t)H * W < otl::MAX_PIXELS, "region_outlines: a frame of 2^29 pixels or more (%dx%d): slot ids are 32-bit", H, W);
    FS_REQUIRE(max_regions >= 1 && max_regions <= 65536, "region_outlines: max_regions=%d out of range (1..65536)", max_regions);
    FS_REQUIRE(connectivity == 4 || connectivity == 8, "region_outlines: connectivity must be 4 or 8, got %d", connectivity);
    FS_REQUIRE(max_contours >= 1 && max_contours <= otl::MAX_CONTOURS, "region_outlines: max_contours=%d out of range (1..2^20)", max_contours);
    FS_REQUIRE(max_vertices >= otl::MIN_VERTICES && max_vertices <= otl::MAX_VERTICES, "region_outlines: max_vertices=%d out of range (4..2^22)",
               max_vertices);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "region_outlines: the workspace is not aligned to 8 bytes");
    u64* ws = static_cast<u64*>(workspace);
    const int R = max_regions, V = max_vertices, rounds = otl::rank_rounds(V);
    const unsigned pchunks = (unsigned)pixel_chunks(H, W), nchunks = (unsigned)node_chunks(V), nblocks = (unsigned)cdiv(V, 256), frames = (unsigned)n;
    const size_t zc = (size_t)n * max_contours * 6, zv = (size_t)n * V, zs = (size_t)n * R * 3, zn = (size_t)n * 4;
    hipLaunchKernelGGL(outline_zero_kernel, dim3((unsigned)std::min<size_t>((zc + zv + zs + zn + 255) / 256, 1u << 16)), dim3(256), 0, s,
                       reinterpret_cast<u64*>(contours), zc, reinterpret_cast<u64*>(vertices), zv, reinterpret_cast<u64*>(shape), zs,
                       reinterpret_cast<u64*>(counts), zn);
    hipLaunchKernelGGL(outline_mark_kernel, dim3(pchunks, frames), dim3(256), 0, s, index, H, W, R, V, ws, reinterpret_cast<u64*>(shape));
    hipLaunchKernelGGL(outline_offsets_kernel, dim3(frames), dim3(1024), 0, s, H, W, V, ws);
    hipLaunchKernelGGL(outline_compact_kernel, dim3(pchunks, frames), dim3(256), 0, s, index, H, W, R, V, ws);
    hipLaunchKernelGGL(outline_link_kernel, dim3(nblocks, frames), dim3(256), 0, s, index, H, W, R, V, connectivity, ws);
    for (int k = 0; k < rounds; ++k)  // ceil(log2 max_vertices) <= 22
        hipLaunchKernelGGL(outline_jump_kernel, dim3(nblocks, frames), dim3(256), 0, s, H, W, V, k, ws);
    hipLaunchKernelGGL(outline_length_kernel, dim3(nblocks, frames), dim3(256), 0, s, H, W, V, rounds, ws);
    hipLaunchKernelGGL(outline_anchor_count_kernel, dim3(nchunks, frames), dim3(1024), 0, s, H, W, V, rounds, ws);
    hipLaunchKernelGGL(outline_counts_kernel, dim3(frames), dim3(1024), 0, s, H, W, R, V, max_contours, ws, shape, counts);
    hipLaunchKernelGGL(outline_place_kernel, dim3(nchunks, frames), dim3(1024), 0, s, index, H, W, R, V, max_contours, rounds, ws, contours,
                       reinterpret_cast<u64*>(shape));
    hipLaunchKernelGGL(outline_scatter_kernel, dim3(nblocks, frames), dim3(256), 0, s, H, W, V, max_contours, rounds, ws, vertices,
                       reinterpret_cast<u64*>(contours));
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
