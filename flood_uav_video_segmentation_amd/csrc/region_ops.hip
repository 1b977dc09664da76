// Connected regions of a hard mask (include/floodseg_test.h: mask_regions, region_table, region_filter).  OUR DEFINITION
// -- the reference emits hard masks only.  Opt-in passes behind the tails: nothing on the shipped routes calls them.
//   mask_regions    uint8 mask [n,H,W]                 -> int32 canonical labels [n,H,W]: 1 + the raster index of the region's first pixel
//   region_table    mask, labels (+ confidence)        -> int64 [n][max_regions][10] rows in anchor order, counts [n][2], int32 index plane
//   region_filter   mask, index plane, table           -> the mask with every region below min_area re-classed by its neighbours' vote
// Integers throughout, and every result is a function of the inputs alone: union by minimum index makes the root of a set its smallest
// index whatever the order threads arrive in, integer sums / minima / maxima are exact in any order.  The union-find primitives and
// the per-pixel step of each labelling pass are region_uf.h's (__host__ __device__, also run on the CPU by the tests); every loop in
// them is bounded by a strictly decreasing index (stated there).  Nothing here allocates or synchronises: workspaces are arguments.
#include "kernels.h"
#include "region_uf.h"

#include <algorithm>

namespace fs {

namespace {

constexpr int RANK_CHUNK = 1024;  // pixels per workgroup of the anchor counting / ranking passes (region_rank_chunks)

__global__ __launch_bounds__(256) void region_zero_kernel(unsigned* __restrict__ p, size_t words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = 0u;
}
inline void launch_zero(void* p, size_t bytes, hipStream_t s) {  // bytes % 4 == 0
    const size_t words = bytes / 4;
    const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1u << 20);
    hipLaunchKernelGGL(region_zero_kernel, dim3(blocks), dim3(256), 0, s, static_cast<unsigned*>(p), words);
}

// ------------------------------------------------------------------ labelling, pass 1: one tile in LDS
// grid = (tiles of a frame, frames).  Thread t owns tile pixels t, t + 256, ...: a wave is one tile row of 64 pixels, so the mask
// loads and the cell stores of a wave are 64 consecutive elements.  Every tile pixel inside the frame gets its cell written.
__global__ __launch_bounds__(256) void region_tile_kernel(const uint8_t* __restrict__ mask, int K, int H, int W, int tiles_x, int conn8,
                                                          int* __restrict__ cells) {
    __shared__ uint8_t cls[uf::TILE_H * uf::TILE_W];
    __shared__ int parent[uf::TILE_H * uf::TILE_W];
    const size_t fbase = (size_t)blockIdx.y * H * W;
    const int ty0 = (int)(blockIdx.x / tiles_x) * uf::TILE_H, tx0 = (int)(blockIdx.x % tiles_x) * uf::TILE_W;
    constexpr int PER = uf::TILE_H * uf::TILE_W / 256;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = k * 256 + threadIdx.x, y = ty0 + i / uf::TILE_W, x = tx0 + i % uf::TILE_W;
        cls[i] = (y < H && x < W) ? (uint8_t)uf::region_class(mask[fbase + (size_t)y * W + x], K) : (uint8_t)255;
        parent[i] = i;
    }
    __syncthreads();
    for (int k = 0; k < PER; ++k) {
        const int i = k * 256 + threadIdx.x;
        uf::tile_link(cls, parent, i / uf::TILE_W, i % uf::TILE_W, conn8);  // bounded: region_uf.h, unite
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = k * 256 + threadIdx.x, y = ty0 + i / uf::TILE_W, x = tx0 + i % uf::TILE_W;
        if (y < H && x < W) cells[fbase + (size_t)y * W + x] = uf::tile_cell(cls, parent, i, ty0, tx0, W);  // bounded: find
    }
}

// ------------------------------------------------------------------ pass 2: unite across tile edges, one border pixel per thread
__global__ __launch_bounds__(256) void region_border_kernel(const uint8_t* __restrict__ mask, int K, int H, int W, int conn8, int border,
                                                            int* __restrict__ cells) {
    const size_t fbase = (size_t)blockIdx.y * H * W;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < border) uf::border_walk(mask + fbase, cells + fbase, K, H, W, conn8, t);  // bounded: region_uf.h, unite
}

// ------------------------------------------------------------------ pass 3: cells become canonical labels, in place
__global__ __launch_bounds__(256) void region_flatten_kernel(int HW, int* __restrict__ cells) {
    const size_t fbase = (size_t)blockIdx.y * HW;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < HW) uf::flatten(cells + fbase, i);  // bounded: find
}

// ------------------------------------------------------------------ anchors, ranks, index plane, table
// a label the caller handed in is trusted as far as memory safety allows: outside 1..HW it is background
__device__ __forceinline__ bool is_anchor(int label, int i) { return label == i + 1; }

// per chunk of RANK_CHUNK pixels: the number of anchors
__global__ __launch_bounds__(256) void region_count_kernel(const int* __restrict__ labels, int HW, int chunks, int* __restrict__ chunk_count) {
    const size_t fbase = (size_t)blockIdx.y * HW;
    const int begin = blockIdx.x * RANK_CHUNK;  // < HW (grid)
    int total = 0;
    for (int k = 0; k < RANK_CHUNK / 256; ++k) {
        const int i = begin + k * 256 + threadIdx.x;  // < ceil(HW / RANK_CHUNK) * RANK_CHUNK <= 2^31 - 1 + 1: fits an int
        total += __syncthreads_count(i < HW && is_anchor(labels[fbase + min(i, HW - 1)], i));
    }
    if (threadIdx.x == 0) chunk_count[(size_t)blockIdx.y * chunks + blockIdx.x] = total;
}

// one workgroup per frame: the chunk counts become exclusive offsets in place; counts[f] = (regions, rows written)
__global__ __launch_bounds__(256) void region_scan_kernel(int* __restrict__ chunk_count, int chunks, int max_regions, long long* __restrict__ counts) {
    __shared__ int part[256];
    int* mine = chunk_count + (size_t)blockIdx.x * chunks;
    int carry = 0;
    for (int base = 0; base < chunks; base += 256) {
        const int c = base + threadIdx.x;
        const int v = c < chunks ? mine[c] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {  // inclusive scan of the 256 values
            const int add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < chunks) mine[c] = carry + part[threadIdx.x] - v;
        carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[2 * blockIdx.x] = carry;
        counts[2 * blockIdx.x + 1] = min(carry, max_regions);
    }
}

// per chunk: the rank of every anchor = chunk offset + anchors before it in the chunk.  The anchor's cell of the index plane gets the
// rank (-1 past the cap), and its table row its start values: the class, and the anchor's own coordinates as x0, y0, x1, y1 (y0 is
// final -- the anchor is the region's first pixel; the others are bounds the accumulation lowers / raises).
__global__ __launch_bounds__(256) void region_rank_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, int HW, int W, int chunks,
                                                          const int* __restrict__ chunk_offset, int max_regions, int* __restrict__ index,
                                                          long long* __restrict__ table) {
    __shared__ int wave_total[4];
    const size_t fbase = (size_t)blockIdx.y * HW;
    const int begin = blockIdx.x * RANK_CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank0 = chunk_offset[(size_t)blockIdx.y * chunks + blockIdx.x];
    for (int k = 0; k < RANK_CHUNK / 256; ++k) {
        const int i = begin + k * 256 + threadIdx.x;
        const bool anchor = i < HW && is_anchor(labels[fbase + min(i, HW - 1)], i);
        const unsigned long long b = __ballot(anchor);
        if (lane == 0) wave_total[wave] = __popcll(b);
        __syncthreads();
        int before = __popcll(b & ((1ull << lane) - 1ull));
        for (int v = 0; v < wave; ++v) before += wave_total[v];
        const int all = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        __syncthreads();
        if (anchor) {
            const int rank = rank0 + before;
            index[fbase + i] = rank < max_regions ? rank : -1;
            if (rank < max_regions) {
                long long* row = table + ((size_t)blockIdx.y * max_regions + rank) * 10;
                const int y = i / W, x = i - y * W;
                row[0] = mask[fbase + i];
                row[2] = x;
                row[3] = y;
                row[4] = x;
                row[5] = y;
            }
        }
        rank0 += all;
    }
}

// per pixel: its index = the rank at its anchor; then the table.  grid = (256-pixel row pieces, rows, frames): a wave is 64
// consecutive pixels of one row.  Runs of equal index inside the wave are reduced across lanes -- a run of consecutive x needs no
// data for its area, box and coordinate sums, and the confidence figures come from one inclusive wave scan -- and the run's first
// lane issues the atomics: 4 to 7 per run, not per pixel.  The box atomics are skipped when a plain read of the row shows they cannot
// change it (the columns move one way only, so a stale read errs towards issuing the atomic, never towards skipping one that counts).
template <bool CONF>
__global__ __launch_bounds__(256) void region_accumulate_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ conf, int H, int W,
                                                                int low, int max_regions, int* index, unsigned long long* table) {
    const int HW = H * W;
    const size_t fbase = (size_t)blockIdx.z * HW;
    const int x = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = x < W;
    const int xc = min(x, W - 1);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const int i = y * W + xc;
        const int lab = labels[fbase + i];
        int idx = -1;
        if (lab >= 1 && lab <= HW) {
            idx = index[fbase + lab - 1];                                    // the anchor's cell: written by the launch in front
            if (idx < -1 || idx >= max_regions) idx = -1;                    // a label that names no anchor (a caller's plane, not ours)
        }
        if (valid && lab != i + 1) index[fbase + i] = idx;  // anchors keep theirs; nobody reads a non-anchor's cell in this launch
        const int key = valid ? idx : -2;
        const int prev = __shfl_up(key, 1);
        const unsigned long long heads = __ballot(lane == 0 || prev != key);
        unsigned packed = 0;  // bits 0..15 the sum of confidence codes (<= 64 * 255), 16..22 the pixels below `low` (<= 64)
        if (CONF) {
            const unsigned c = conf[fbase + i];
            if (key >= 0) packed = c | ((c < (unsigned)low ? 1u : 0u) << 16);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(packed, d);
                if (lane >= d) packed += t;
            }
        }
        const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
        const int end = above ? __ffsll((long long)above) - 1 : 64;  // the run of a head lane is [lane, end)
        unsigned run_conf = 0;
        if (CONF) {
            const unsigned upto = __shfl(packed, end - 1), before = __shfl_up(packed, 1);
            run_conf = upto - (lane == 0 ? 0u : before);
        }
        if (((heads >> lane) & 1ull) && key >= 0) {
            unsigned long long* row = table + ((size_t)blockIdx.z * max_regions + key) * 10;
            const unsigned long long len = (unsigned long long)(end - lane), x1 = (unsigned long long)x + len - 1;
            atomicAdd(&row[1], len);
            if ((unsigned long long)x < row[2]) atomicMin(&row[2], (unsigned long long)x);
            if (x1 > row[4]) atomicMax(&row[4], x1);
            if ((unsigned long long)y > row[5]) atomicMax(&row[5], (unsigned long long)y);
            atomicAdd(&row[6], len * (unsigned long long)x + len * (len - 1) / 2);
            atomicAdd(&row[7], len * (unsigned long long)y);
            if (CONF) {
                if (run_conf & 0xFFFFu) atomicAdd(&row[8], (unsigned long long)(run_conf & 0xFFFFu));
                if (run_conf >> 16) atomicAdd(&row[9], (unsigned long long)(run_conf >> 16));
            }
        }
    }
}

// ------------------------------------------------------------------ despeckle
__device__ __forceinline__ int row_of(const int* __restrict__ index, size_t at, int max_regions) {
    const int r = index[at];
    return r >= 0 && r < max_regions ? r : -1;
}

// one pixel per thread: a pixel of a speckle votes once per in-frame 4-neighbour whose region has a row and area >= min_area
__global__ __launch_bounds__(256) void region_vote_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ index,
                                                          const long long* __restrict__ table, int H, int W, int K, int max_regions,
                                                          long long min_area, int* __restrict__ votes) {
    const int HW = H * W;
    const size_t fbase = (size_t)blockIdx.y * HW;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const int r = row_of(index, fbase + i, max_regions);
    if (r < 0) return;
    const long long* tab = table + (size_t)blockIdx.y * max_regions * 10;
    if (tab[(size_t)r * 10 + 1] >= min_area) return;
    const int y = i / W, x = i - y * W;
    const int dy[4] = {-1, 0, 0, 1}, dx[4] = {0, -1, 1, 0};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int qy = y + dy[d], qx = x + dx[d];
        if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
        const size_t q = fbase + (size_t)qy * W + qx;
        const int rq = row_of(index, q, max_regions);
        if (rq < 0 || tab[(size_t)rq * 10 + 1] < min_area) continue;
        const int cq = mask[q];
        if (cq < K) atomicAdd(&votes[((size_t)blockIdx.y * max_regions + r) * K + cq], 1);
    }
}

// one row per thread: the class with the most votes, the lowest id on a tie, -1 without a vote; left in the row's first vote cell
__global__ __launch_bounds__(256) void region_decide_kernel(int K, int max_regions, int* __restrict__ votes) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= max_regions) return;  // a row nobody voted for (no speckle, or no region at all) decides -1
    int* v = votes + ((size_t)blockIdx.y * max_regions + r) * K;
    int best = 0, arg = -1;
    for (int k = 0; k < K; ++k)
        if (v[k] > best) { best = v[k]; arg = k; }
    v[0] = arg;
}

// the output mask: a pixel of a row with a decision takes it, every other pixel its input.  Stores as conf_ops.hip's store_pair.
template <bool WIDE>
__global__ __launch_bounds__(256) void region_apply_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ index, int H, int W, int K,
                                                           int max_regions, const int* __restrict__ votes, uint8_t* __restrict__ out) {
    const size_t fbase = (size_t)blockIdx.z * H * W;
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int xc = min(x, W - 1);
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const size_t at = fbase + (size_t)y * W + xc;
        unsigned m = mask[at];
        const int r = row_of(index, at, max_regions);
        if (r >= 0) {
            const int d = votes[((size_t)blockIdx.z * max_regions + r) * K];
            if (d >= 0) m = (unsigned)d;
        }
        if (WIDE) {
            const unsigned p1 = __shfl_down(m, 1), p2 = __shfl_down(m, 2), p3 = __shfl_down(m, 3);
            if ((threadIdx.x & 3) == 0 && x < W)  // W % 4 == 0: x + 3 < W as well
                *reinterpret_cast<unsigned*>(out + fbase + (size_t)y * W + x) = (m & 255u) | ((p1 & 255u) << 8) | ((p2 & 255u) << 16) | ((p3 & 255u) << 24);
        } else if (x < W) {
            out[at] = (uint8_t)m;
        }
    }
}

int region_args(const char* what, int n, int H, int W, int K) {
    FS_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "%s: sizes must be >= 1 (at most 65535 frames), got n=%d %dx%d", what, n, H, W);
    FS_REQUIRE(K >= 1 && K <= 255, "%s: K=%d out of range (1..255)", what, K);
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 1, "%s: a frame of 2^31 - 1 pixels or more (%dx%d)", what, H, W);
    return 0;
}

}  // namespace

int region_rank_chunks(int H, int W) { return (int)cdiv64((int64_t)H * W, RANK_CHUNK); }

int launch_mask_regions(const uint8_t* mask, int n, int H, int W, int K, int connectivity, int* labels, hipStream_t s) {
    FS_REQUIRE(mask && labels, "mask_regions: null pointer");
    if (int rc = region_args("mask_regions", n, H, W, K)) return rc;
    FS_REQUIRE(connectivity == 4 || connectivity == 8, "mask_regions: connectivity must be 4 or 8, got %d", connectivity);
    const int conn8 = connectivity == 8, HW = H * W;
    const int tiles_x = cdiv(W, uf::TILE_W), tiles_y = cdiv(H, uf::TILE_H);  // tiles_x * tiles_y <= HW
    // a grid dimension holds fewer than 2^32 threads: 256 per tile.  Only frames thinner than a tile and 2^29 pixels long come near it.
    FS_REQUIRE((int64_t)tiles_x * tiles_y < ((int64_t)1 << 24), "mask_regions: %dx%d is %lld tiles of %dx%d, 2^24 or more", H, W,
               (long long)tiles_x * tiles_y, uf::TILE_H, uf::TILE_W);
    hipLaunchKernelGGL(region_tile_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(256), 0, s, mask, K, H, W, tiles_x, conn8, labels);
    const int border = (int)uf::border_count(H, W);  // < HW
    if (border > 0)
        hipLaunchKernelGGL(region_border_kernel, dim3((unsigned)cdiv(border, 256), (unsigned)n), dim3(256), 0, s, mask, K, H, W, conn8, border, labels);
    hipLaunchKernelGGL(region_flatten_kernel, dim3((unsigned)cdiv64(HW, 256), (unsigned)n), dim3(256), 0, s, HW, labels);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_region_table(const uint8_t* mask, const int* labels, const uint8_t* conf, int n, int H, int W, int K, int low, int max_regions,
                        long long* table, long long* counts, int* index, int* workspace, hipStream_t s) {
    FS_REQUIRE(mask && labels && table && counts && index && workspace, "region_table: null pointer");
    if (int rc = region_args("region_table", n, H, W, K)) return rc;
    FS_REQUIRE(low >= 0 && low <= 255, "region_table: low=%d out of range (0..255)", low);
    FS_REQUIRE(max_regions >= 1 && max_regions <= 65536, "region_table: max_regions=%d out of range (1..65536)", max_regions);
    const int HW = H * W, chunks = region_rank_chunks(H, W);
    launch_zero(table, (size_t)n * max_regions * 10 * sizeof(long long), s);
    hipLaunchKernelGGL(region_count_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, s, labels, HW, chunks, workspace);
    hipLaunchKernelGGL(region_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, workspace, chunks, max_regions, counts);
    hipLaunchKernelGGL(region_rank_kernel, dim3((unsigned)chunks, (unsigned)n), dim3(256), 0, s, mask, labels, HW, W, chunks, workspace, max_regions, index,
                       table);
    const dim3 grid((unsigned)cdiv(W, 256), (unsigned)std::min(H, 65535), (unsigned)n);
    unsigned long long* t = reinterpret_cast<unsigned long long*>(table);
    if (conf) hipLaunchKernelGGL((region_accumulate_kernel<true>), grid, dim3(256), 0, s, labels, conf, H, W, low, max_regions, index, t);
    else hipLaunchKernelGGL((region_accumulate_kernel<false>), grid, dim3(256), 0, s, labels, conf, H, W, low, max_regions, index, t);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_region_filter(const uint8_t* mask, const int* index, const long long* table, int n, int H, int W, int K,
                         int max_regions, int min_area, uint8_t* out, int* votes, hipStream_t s) {
    FS_REQUIRE(mask && index && table && out && votes, "region_filter: null pointer");
    if (int rc = region_args("region_filter", n, H, W, K)) return rc;
    FS_REQUIRE(max_regions >= 1 && max_regions <= 65536, "region_filter: max_regions=%d out of range (1..65536)", max_regions);
    FS_REQUIRE(min_area >= 0, "region_filter: min_area=%d must be >= 0", min_area);
    const int HW = H * W;
    launch_zero(votes, (size_t)n * max_regions * K * sizeof(int), s);
    hipLaunchKernelGGL(region_vote_kernel, dim3((unsigned)cdiv64(HW, 256), (unsigned)n), dim3(256), 0, s, mask, index, table, H, W, K, max_regions,
                       (long long)min_area, votes);
    hipLaunchKernelGGL(region_decide_kernel, dim3((unsigned)cdiv(max_regions, 256), (unsigned)n), dim3(256), 0, s, K, max_regions, votes);
    const bool wide = W % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
    const dim3 grid((unsigned)cdiv(W, 256), (unsigned)std::min(H, 65535), (unsigned)n);
    if (wide) hipLaunchKernelGGL((region_apply_kernel<true>), grid, dim3(256), 0, s, mask, index, H, W, K, max_regions, votes, out);
    else hipLaunchKernelGGL((region_apply_kernel<false>), grid, dim3(256), 0, s, mask, index, H, W, K, max_regions, votes, out);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
