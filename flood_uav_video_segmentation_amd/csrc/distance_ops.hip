// Distance to a class on the GPU (include/floodseg_test.h: mask_distance, region_proximity).  OUR DEFINITION -- the
// reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.  Integers throughout; the packing of a candidate, the
// stop rule of the row scan, the column tie rule and the threshold bins are distance_defs.h's (__host__ __device__, also run on the CPU
// by the tests).
//   mask_distance     the exact squared Euclidean distance to the nearest source pixel, in separable form, three launches:
//     1 column summary  per column and chunk of 64 rows the first and the last source row (one dword; 4 B per 64 pixels)
//     2 column fill     per pixel the row of the nearest source of its own column, the upper one on a tie: the chunk's 64 mask bytes
//                       become one 64-bit word, the rows above and below come from the summaries (at most H / 64 of them each way)
//     3 row scan        one workgroup per row stages the row's 2-byte entries in LDS; a thread scans outwards from its own x and
//                       stops at the first offset d with d * d > best (distance_defs.h: scan_stops); a frame without a source is
//                       recognised by the row being empty (every column's entry covers the whole column) and is not scanned
//   region_proximity  the field tabulated per class (exposure) and per region (near), three launches: set up the rows (the minimum
//                     starts at all ones), accumulate (LDS histogram per workgroup; per region a 64-bit atomic minimum of
//                     d2 << 32 | raster index and an atomic sum, both taken once per run of a row along the 1024 consecutive pixels a wave
//                     owns, and the minimum only where it would lower the word), finish (the word becomes the row's columns).
// Every loop bound follows from the arguments; no thread waits for another; sums and minima of integers: the order does not matter.
#include "kernels.h"
#include "distance_defs.h"

#include <algorithm>

namespace fs {

namespace {

constexpr int COL_THREADS = 256;   // columns per workgroup of the two column kernels
constexpr int ROW_THREADS = 256;   // threads of the workgroup that scans one row
constexpr int ACC_THREADS = 256;   // of the accumulate pass: four waves
constexpr int ACC_STEPS = 16;      // 64-pixel steps of a wave of the accumulate pass: it owns 1024 consecutive pixels

struct Thresholds {
    int t[dst::MAX_THRESHOLDS];
};

// bit r = row y0 + r of column x is a source; rows = the chunk's rows inside the frame (1..64)
__device__ __forceinline__ uint64_t chunk_bits(const uint8_t* __restrict__ col, int rows, int W, uint32_t set) {
    uint64_t bits = 0;
    for (int r = 0; r < rows; ++r)
        if (dst::in_set(col[(size_t)r * W], set)) bits |= (uint64_t)1 << r;
    return bits;
}

// ------------------------------------------------------------------ mask_distance 1: first | last << 16 per column and chunk
__global__ __launch_bounds__(COL_THREADS) void distance_summary_kernel(const uint8_t* __restrict__ mask, int H, int W, uint32_t set,
                                                                       uint32_t* __restrict__ summary) {
    const int x = blockIdx.x * COL_THREADS + threadIdx.x, c = blockIdx.y, f = blockIdx.z, chunks = gridDim.y;
    if (x >= W) return;
    const int y0 = c * dst::CHUNK, rows = min(dst::CHUNK, H - y0);
    const uint64_t bits = chunk_bits(mask + ((size_t)f * H + y0) * W + x, rows, W, set);
    const uint32_t first = bits ? (uint32_t)dst::chunk_down(bits, y0, 0) : dst::NO_ROW;
    const uint32_t last = bits ? (uint32_t)dst::chunk_up(bits, y0, 63) : dst::NO_ROW;
    summary[((size_t)f * chunks + c) * W + x] = first | (last << 16);
}

// ------------------------------------------------------------------ mask_distance 2: the nearest source row of the own column
__global__ __launch_bounds__(COL_THREADS) void distance_column_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ summary, int H,
                                                                      int W, uint32_t set, uint16_t* __restrict__ nearest_row) {
    const int x = blockIdx.x * COL_THREADS + threadIdx.x, c = blockIdx.y, f = blockIdx.z, chunks = gridDim.y;
    if (x >= W) return;
    const int y0 = c * dst::CHUNK, rows = min(dst::CHUNK, H - y0);
    const uint64_t bits = chunk_bits(mask + ((size_t)f * H + y0) * W + x, rows, W, set);
    const uint32_t* col = summary + (size_t)f * chunks * W + x;
    int above = -1, below = -1;  // the carries: the last source row of the chunks above, the first of the chunks below
    for (int k = c - 1; k >= 0 && above < 0; --k) {
        const uint32_t last = col[(size_t)k * W] >> 16;
        if (last != dst::NO_ROW) above = min((int)last, H - 1);  // a workspace value is clamped before use
    }
    for (int k = c + 1; k < chunks && below < 0; ++k) {
        const uint32_t first = col[(size_t)k * W] & 0xffffu;
        if (first != dst::NO_ROW) below = min((int)first, H - 1);
    }
    uint16_t* out = nearest_row + ((size_t)f * H + y0) * W + x;
    for (int r = 0; r < rows; ++r) {
        int up = dst::chunk_up(bits, y0, r), down = dst::chunk_down(bits, y0, r);
        if (up < 0) up = above;
        if (down < 0) down = below;
        const int pick = dst::column_pick(y0 + r, up, down);
        out[(size_t)r * W] = pick < 0 ? (uint16_t)dst::NO_ROW : (uint16_t)pick;
    }
}

// ------------------------------------------------------------------ mask_distance 3: one row per workgroup, lds = W entries
template <bool NEAREST>
__global__ __launch_bounds__(ROW_THREADS) void distance_row_kernel(const uint16_t* __restrict__ nearest_row, int H, int W, int R,
                                                                   uint32_t* __restrict__ d2, int32_t* __restrict__ nearest) {
    extern __shared__ uint16_t row_lds[];
    const int y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const size_t at = ((size_t)f * H + y) * W;
    int any = 0;
    for (int x = tid; x < W; x += ROW_THREADS) {
        const uint16_t v = nearest_row[at + x];
        row_lds[x] = v;
        any |= v != dst::NO_ROW;
    }
    any = __syncthreads_or(any);  // no entry in this row: no source in any column, the frame is empty
    const uint16_t* entries = row_lds;
    for (int x = tid; x < W; x += ROW_THREADS) {
        const uint64_t best = any ? dst::scan_row(entries, y, x, W, H, R, NEAREST) : dst::NO_CANDIDATE;
        uint32_t v;
        int32_t q;
        dst::report(best, R, &v, &q);
        d2[at + x] = v;
        if (NEAREST) nearest[at + x] = q;
    }
}

// ------------------------------------------------------------------ region_proximity 1: the rows before the sums
// near word 0 of every row = all ones (the minimum's start), the other seven and the exposure table 0
__global__ __launch_bounds__(256) void proximity_setup_kernel(unsigned long long* __restrict__ exposure, int exposure_words,
                                                              unsigned long long* __restrict__ near, int near_words) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i < exposure_words) exposure[(size_t)f * exposure_words + i] = 0ull;
    if (i < near_words) near[(size_t)f * near_words + i] = (i & 7) == 0 ? dst::NO_CANDIDATE : 0ull;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int clamped_rows(const long long* __restrict__ counts, int f, int max_regions) {
    const long long rows = counts[2 * (size_t)f + 1];
    return (int)(rows < 0 ? 0 : rows > max_regions ? max_regions : rows);
}

// ------------------------------------------------------------------ region_proximity 2: one pass over the frame's pixels
// A wave owns ACC_STEPS x 64 CONSECUTIVE pixels and walks them 64 at a time, so what it meets is runs of the same row: it keeps one
// (row, minimum, count) in registers -- the same value in every lane -- and sends it to memory only when the row changes and at its end.
__device__ __forceinline__ void proximity_flush(unsigned long long* table, int lane, int r, unsigned long long key, unsigned close) {
    if (lane != 0 || r < 0) return;
    unsigned long long* row = table + (size_t)r * 8;
    if (key < __atomic_load_n(row, __ATOMIC_RELAXED)) atomicMin(row, key);  // the word only falls: an old value costs one atomic more
    if (close) atomicAdd(row + 6, (unsigned long long)close);
}

__global__ __launch_bounds__(ACC_THREADS) void proximity_accumulate_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ d2,
                                                                           const int* __restrict__ index, const long long* __restrict__ counts,
                                                                           unsigned HW, int K, int max_regions, uint32_t targets, Thresholds thr, int B,
                                                                           unsigned long long* exposure, unsigned long long* near) {
    __shared__ unsigned hist[dst::MAX_SOURCE_CLASSES * dst::MAX_THRESHOLDS];  // [class][first threshold reached]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.y;
    for (int i = tid; i < dst::MAX_SOURCE_CLASSES * dst::MAX_THRESHOLDS; i += ACC_THREADS) hist[i] = 0u;
    __syncthreads();
    const int rows = clamped_rows(counts, f, max_regions);
    const uint32_t near_d2 = (uint32_t)thr.t[0] * (uint32_t)thr.t[0];
    const size_t frame = (size_t)f * HW;
    unsigned long long* table = near + (size_t)f * max_regions * 8;
    const uint64_t first = ((uint64_t)blockIdx.x * (ACC_THREADS / 64) + wave) * (uint64_t)(ACC_STEPS * 64);  // < HW + 64 ACC_STEPS ACC_THREADS
    int run_row = -1;                                    // the run the wave is in: its row, its minimum, its pixels within thresholds[0]
    unsigned long long run_key = dst::NO_CANDIDATE;
    unsigned run_close = 0;
    for (int step = 0; step < ACC_STEPS; ++step) {       // uniform in the wave: the ballots and shuffles below are whole
        const uint64_t p = first + (uint64_t)step * 64 + lane;
        int bin = -1, r = -1;
        unsigned long long key = dst::NO_CANDIDATE;
        bool close = false;
        if (p < HW) {
            const uint32_t d = d2[frame + p];
            if (d != dst::NONE) {
                const int m = mask[frame + p];
                if (m < K && dst::in_set(m, targets)) {
                    const int b = dst::first_bin(d, thr.t, B);
                    if (b < B) bin = m * dst::MAX_THRESHOLDS + b;
                }
                const int i = index[frame + p];
                if (i >= 0 && i < rows) {  // an index read from memory is checked before use
                    r = i;
                    key = dst::pack(d, (uint32_t)p);
                    close = d <= near_d2;
                }
            }
        }
        // the class histogram: one LDS atomic per wave where all its counted pixels fall into one cell, one per pixel otherwise
        const unsigned long long counted = __ballot(bin >= 0);
        if (counted) {
            const int lead = __ffsll((long long)counted) - 1, cell = __shfl(bin, lead);
            if (__ballot(bin >= 0 && bin != cell) == 0ull) {
                if (lane == lead) atomicAdd(hist + cell, (unsigned)__popcll(counted));
            } else if (bin >= 0) {
                atomicAdd(hist + bin, 1u);
            }
        }
        // the region rows: the wave's 64 pixels row by row (at most 64 different ones), each joined to the run or starting a new one
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1, r0 = __shfl(r, lead);
            const bool own = r == r0;
            const unsigned long long k = wave_min(own ? key : dst::NO_CANDIDATE);
            const unsigned c = (unsigned)__popcll(__ballot(own && close));
            if (r0 == run_row) {
                run_key = k < run_key ? k : run_key;
                run_close += c;
            } else {
                proximity_flush(table, lane, run_row, run_key, run_close);
                run_row = r0, run_key = k, run_close = c;
            }
            todo &= ~__ballot(own);
        }
    }
    proximity_flush(table, lane, run_row, run_key, run_close);
    __syncthreads();
    for (int i = tid; i < dst::MAX_SOURCE_CLASSES * dst::MAX_THRESHOLDS; i += ACC_THREADS) {
        const int k = i / dst::MAX_THRESHOLDS, b = i % dst::MAX_THRESHOLDS;
        if (k >= K || b >= B) continue;
        unsigned sum = 0;  // cumulative in b
        for (int j = 0; j <= b; ++j) sum += hist[k * dst::MAX_THRESHOLDS + j];
        if (sum) atomicAdd(exposure + ((size_t)f * K + k) * B + b, (unsigned long long)sum);
    }
}

// ------------------------------------------------------------------ region_proximity 3: the minimum's word becomes the row
__global__ __launch_bounds__(256) void proximity_finish_kernel(const int* __restrict__ nearest, const int* __restrict__ index,
                                                               const long long* __restrict__ counts, int W, unsigned HW, int max_regions,
                                                               long long* __restrict__ near) {
    const int r = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (r >= max_regions) return;
    const int rows = clamped_rows(counts, f, max_regions);
    long long* row = near + ((size_t)f * max_regions + r) * 8;
    const unsigned long long key = (unsigned long long)row[0];
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < rows) {
        v[6] = row[6];
        if (key == dst::NO_CANDIDATE) {
            v[0] = v[1] = v[2] = v[3] = v[4] = v[5] = -1;
            v[6] = 0;
        } else {
            const unsigned p = min(dst::cand_raster(key), HW - 1u);
            v[0] = (long long)dst::cand_d2(key);
            v[1] = p % (unsigned)W, v[2] = p / (unsigned)W;
            v[3] = v[4] = v[5] = -1;
            if (nearest) {
                const int q = nearest[(size_t)f * HW + p];
                if (q >= 0 && (unsigned)q < HW) {  // an index read from memory is checked before use
                    const int i = index[(size_t)f * HW + q];
                    v[3] = q % W, v[4] = q / W;
                    v[5] = i >= 0 && i < rows ? i : -1;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = v[j];
}

}  // namespace

int launch_mask_distance(const uint8_t* mask, int n, int H, int W, uint32_t source_set, int max_dist, uint32_t* d2, int32_t* nearest, void* workspace,
                         hipStream_t s) {
    FS_REQUIRE(mask && d2 && workspace, "mask_distance: null pointer");
    FS_REQUIRE(n >= 1, "mask_distance: at least one frame, got n=%d", n);
    FS_REQUIRE(n <= 65535, "mask_distance: at most 65535 frames per call, got n=%d", n);
    FS_REQUIRE(H >= 1 && W >= 1, "mask_distance: sizes must be >= 1, got %dx%d", H, W);
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 1, "mask_distance: a frame of 2^31 - 1 pixels or more (%dx%d)", H, W);
    FS_REQUIRE(H <= dst::MAX_SIDE && W <= dst::MAX_SIDE, "mask_distance: sizes must be <= %d (d2 stays below 2^31), got %dx%d", dst::MAX_SIDE, H, W);
    FS_REQUIRE(source_set != 0u, "mask_distance: source_set is empty (bit k set: class k is a source)");
    FS_REQUIRE(max_dist >= 0 && max_dist <= dst::MAX_DIST, "mask_distance: max_dist=%d out of range (0..%d, 0: unbounded)", max_dist, dst::MAX_DIST);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(d2) % 4 == 0, "mask_distance: d2 is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(nearest) % 4 == 0, "mask_distance: nearest is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "mask_distance: the workspace is not aligned to 4 bytes");
    const int chunks = cdiv(H, dst::CHUNK);
    uint32_t* summary = static_cast<uint32_t*>(workspace);
    uint16_t* rows = reinterpret_cast<uint16_t*>(summary + (size_t)n * chunks * W);
    const dim3 col_grid((unsigned)cdiv(W, COL_THREADS), (unsigned)chunks, (unsigned)n);
    hipLaunchKernelGGL(distance_summary_kernel, col_grid, dim3(COL_THREADS), 0, s, mask, H, W, source_set, summary);
    hipLaunchKernelGGL(distance_column_kernel, col_grid, dim3(COL_THREADS), 0, s, mask, summary, H, W, source_set, rows);
    const size_t lds = ((size_t)W * sizeof(uint16_t) + 3) / 4 * 4;  // at most 64 KiB
    auto kernel = nearest ? distance_row_kernel<true> : distance_row_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)H, (unsigned)n), dim3(ROW_THREADS), lds, s, rows, H, W, max_dist, d2, nearest);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_region_proximity(const uint8_t* mask, const uint32_t* d2, const int32_t* nearest, const int32_t* index, const long long* counts, int n, int H,
                            int W, int K, int max_regions, uint32_t target_set, const int32_t* thresholds, int B, long long* exposure, long long* near,
                            hipStream_t s) {
    FS_REQUIRE(mask && d2 && index && counts && thresholds && exposure && near, "region_proximity: null pointer");
    FS_REQUIRE(n >= 1, "region_proximity: at least one frame, got n=%d", n);
    FS_REQUIRE(n <= 65535, "region_proximity: at most 65535 frames per call, got n=%d", n);
    FS_REQUIRE(H >= 1 && W >= 1, "region_proximity: sizes must be >= 1, got %dx%d", H, W);
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 1, "region_proximity: a frame of 2^31 - 1 pixels or more (%dx%d)", H, W);
    FS_REQUIRE(H <= dst::MAX_SIDE && W <= dst::MAX_SIDE, "region_proximity: sizes must be <= %d, got %dx%d", dst::MAX_SIDE, H, W);
    FS_REQUIRE(K >= 1 && K <= 255, "region_proximity: classes=%d out of range (1..255)", K);
    FS_REQUIRE(max_regions >= 1 && max_regions <= 65536, "region_proximity: max_regions=%d out of range (1..65536)", max_regions);
    FS_REQUIRE(B >= 1 && B <= dst::MAX_THRESHOLDS, "region_proximity: %d thresholds, out of range (1..%d)", B, dst::MAX_THRESHOLDS);
    Thresholds thr = {};
    for (int b = 0; b < B; ++b) {  // the caller's host array
        FS_REQUIRE(thresholds[b] >= 0 && thresholds[b] <= dst::MAX_DIST, "region_proximity: thresholds[%d]=%d out of range (0..%d)", b, thresholds[b],
                   dst::MAX_DIST);
        FS_REQUIRE(b == 0 || thresholds[b] > thresholds[b - 1], "region_proximity: thresholds must be strictly ascending, got %d behind %d", thresholds[b],
                   thresholds[b - 1]);
        thr.t[b] = thresholds[b];
    }
    FS_REQUIRE(reinterpret_cast<uintptr_t>(d2) % 4 == 0 && reinterpret_cast<uintptr_t>(nearest) % 4 == 0 && reinterpret_cast<uintptr_t>(index) % 4 == 0,
               "region_proximity: d2, nearest or index is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(counts) % 8 == 0 && reinterpret_cast<uintptr_t>(exposure) % 8 == 0 && reinterpret_cast<uintptr_t>(near) % 8 == 0,
               "region_proximity: counts, exposure or near is not aligned to 8 bytes");
    const unsigned HW = (unsigned)H * (unsigned)W;
    const int exposure_words = K * B, near_words = max_regions * 8;
    unsigned long long* exp_u = reinterpret_cast<unsigned long long*>(exposure);
    unsigned long long* near_u = reinterpret_cast<unsigned long long*>(near);
    hipLaunchKernelGGL(proximity_setup_kernel, dim3((unsigned)cdiv(std::max(exposure_words, near_words), 256), (unsigned)n), dim3(256), 0, s, exp_u,
                       exposure_words, near_u, near_words);
    const unsigned acc_grid = (HW + ACC_THREADS * ACC_STEPS - 1u) / (ACC_THREADS * ACC_STEPS);  // <= 2^19
    hipLaunchKernelGGL(proximity_accumulate_kernel, dim3(acc_grid, (unsigned)n), dim3(ACC_THREADS), 0, s, mask, d2, index, counts, HW, K, max_regions,
                       target_set, thr, B, exp_u, near_u);
    hipLaunchKernelGGL(proximity_finish_kernel, dim3((unsigned)cdiv(max_regions, 256), (unsigned)n), dim3(256), 0, s, nearest, index, counts, W, HW,
                       max_regions, near);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
