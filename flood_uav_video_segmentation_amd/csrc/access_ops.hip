// Dry-route reachability on the GPU (include/floodseg_test.h: mask_access, region_access).  OUR DEFINITION -- the
// reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.  Integers throughout; the move table, the allowed-move
// test, the key (cost, then origin), the bound and the gather of one pixel are access_defs.h's (__host__ __device__, also run on the CPU
// by the tests).
//   mask_access     the cheapest route from any seed over passable ground, as a fixed point of gathers, 2 + rounds launches:
//     1 init          every pixel's 64-bit key (cost << 32 | origin) into the workspace: from the seeds, or from the planes of an earlier
//                     call (resume); every tile dirty; the status row and the round words
//     2 round (x rounds)  one workgroup of 256 per 32 x 32 tile.  A tile that is not dirty returns at once.  A dirty one stages its keys
//                     and a ring of one pixel in LDS, turns the classes into the eight move costs of each owned pixel (registers; the
//                     classes are not looked at again), and sweeps: every thread gathers its four pixels from LDS, a barrier, the
//                     lowered keys are written to LDS, a barrier that also says whether anything was lowered.  At most SWEEPS sweeps; a
//                     tile that is still changing then marks itself dirty.  The lowered keys go back to memory as 64-bit words, and
//                     every neighbour tile whose ring holds one of them is marked dirty for the next round.
//     3 finish        the keys become the d and origin planes; the status row
//   Between workgroups of one round nothing is handed over: a tile that reads a neighbour's key while the neighbour lowers it sees the
//   old or the new 64-bit word, both costs of real routes, and is marked dirty by that neighbour either way; what a round wrote is
//   read for certain from the next launch on.  The dirty flags and the round words alternate between two sets by the round's parity, so a
//   round only reads and clears the one and only sets the other.
//   region_access   the field tabulated per class (reach) and per region (rows), three launches in the form of region_proximity.
// Every loop bound follows from the arguments or is a constant; no thread waits for another workgroup; minima, maxima and sums of
// integers: the order does not matter.
#include "kernels.h"
#include "access_defs.h"

#include <algorithm>

namespace fs {

namespace {

constexpr int T = 32;                  // the tile's edge: FS_ACCESS_TILE
constexpr int LW = T + 2;              // with the ring
constexpr int THREADS = 256;           // four waves; a thread owns the pixels (tid % 32, tid / 32 + 8 j), j = 0..3
constexpr int OWN = T * T / THREADS;   // 4
constexpr int SWEEPS = 4 * T;          // the cap of the inner loop: 128
constexpr int ACC_THREADS = 256;       // of region_access' accumulate pass: four waves
constexpr int ACC_STEPS = 16;          // 64-pixel steps of a wave of that pass: it owns 1024 consecutive pixels

struct KindTable {
    uint16_t kind[acc::MAX_CLASSES];  // acc::kind_of per class id
};

__device__ __forceinline__ uint64_t load_key(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_key(unsigned long long* p, uint64_t v) {
    __hip_atomic_store(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ mask_access 1: keys, flags, words, status
__global__ __launch_bounds__(256) void access_init_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ seeds, KindTable table, unsigned HW,
                                                          unsigned tiles, int resume, const uint32_t* __restrict__ d, const int32_t* __restrict__ origin,
                                                          unsigned long long* __restrict__ keys, uint32_t* __restrict__ flags, uint32_t* __restrict__ words,
                                                          int32_t* __restrict__ status) {
    __shared__ uint16_t kinds[acc::MAX_CLASSES];
    const unsigned i = blockIdx.x * 256u + threadIdx.x, f = blockIdx.y, n = gridDim.y;
    if (threadIdx.x < acc::MAX_CLASSES) kinds[threadIdx.x] = table.kind[threadIdx.x];
    __syncthreads();
    if (i < HW) {
        const size_t at = (size_t)f * HW + i;
        uint64_t key;
        if (resume) {
            key = acc::plane_key(d[at], origin ? origin[at] : 0, origin != nullptr);
        } else {
            const int m = mask[at];
            key = acc::seed_key(m < acc::MAX_CLASSES ? kinds[m] : 0u, seeds[at], i, origin != nullptr);
        }
        keys[at] = key;
    }
    if (i < tiles) {
        flags[(size_t)f * tiles + i] = 1u;                       // this round's set: every tile is looked at once
        flags[((size_t)n + f) * tiles + i] = 0u;                 // the next round's
    }
    if (i < 4u) {
        words[f * 4u + i] = 0u;
        status[f * 4u + i] = i == 0u ? 1 : 0;
    }
}

// ------------------------------------------------------------------ mask_access 2: one round
template <bool CONN8>
__global__ __launch_bounds__(THREADS) void access_round_kernel(const uint8_t* __restrict__ mask, KindTable table, int H, int W, uint32_t bound, int round,
                                                               unsigned long long* keys, uint32_t* flags, uint32_t* words) {
    __shared__ unsigned long long key_lds[LW * LW];
    __shared__ uint16_t kind_lds[LW * LW];
    __shared__ uint16_t kinds[acc::MAX_CLASSES];
    __shared__ unsigned marks;
    constexpr int NM = CONN8 ? 8 : 4;
    const int tid = threadIdx.x, bx = blockIdx.x, by = blockIdx.y, f = blockIdx.z;
    const int tiles_x = gridDim.x, tiles_y = gridDim.y, n = gridDim.z;
    const unsigned tiles = (unsigned)tiles_x * (unsigned)tiles_y, tile = (unsigned)by * tiles_x + bx;
    const int par = round & 1;
    uint32_t* mine = flags + ((size_t)par * n + f) * tiles;
    uint32_t* next = flags + ((size_t)(par ^ 1) * n + f) * tiles;
    const uint32_t dirty = mine[tile];  // every thread reads the one word: a tile that is not dirty leaves without a barrier
    if (tid == 0 && tile == 0u && round > 0) {  // the frame's first tile keeps the count of the rounds that lowered something
        uint32_t* w = words + (size_t)f * 4;
        w[2] += w[par ^ 1];
        w[par ^ 1] = 0u;
    }
    if (!dirty) return;
    if (tid == 0) marks = 0u;
    if (tid < acc::MAX_CLASSES) kinds[tid] = table.kind[tid];
    __syncthreads();                 // every thread has read the flag
    if (tid == 0) mine[tile] = 0u;   // nobody else touches this word in this round

    const int x0 = bx * T, y0 = by * T;
    const size_t frame = (size_t)f * H * W;
    for (int i = tid; i < LW * LW; i += THREADS) {
        const int gx = x0 + i % LW - 1, gy = y0 + i / LW - 1;
        const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
        uint64_t key = acc::NO_KEY;
        uint32_t kind = 0u;
        if (inside) {
            const size_t at = frame + (size_t)gy * W + gx;
            const int m = mask[at];
            key = load_key(keys + at);
            kind = m < acc::MAX_CLASSES ? kinds[m] : 0u;
        }
        key_lds[i] = key;
        kind_lds[i] = (uint16_t)kind;
    }
    __syncthreads();

    const int lx = tid % T, ly0 = tid / T;
    uint64_t cur[OWN], was[OWN];
    uint16_t w[OWN][NM];
    bool live[OWN];
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int li = (ly0 + (THREADS / T) * j + 1) * LW + lx + 1;
        const uint32_t to = kind_lds[li];
        cur[j] = was[j] = key_lds[li];
        bool any = false;
#pragma unroll
        for (int k = 0; k < NM; ++k) {
            const int dx = acc::move_dx(k), dy = acc::move_dy(k);
            const uint32_t c = acc::move_cost(k, kind_lds[li + dy * LW + dx], to, kind_lds[li + dx], kind_lds[li + dy * LW]);
            w[j][k] = (uint16_t)c;
            any |= c != 0u;
        }
        live[j] = any;
    }

    int changed = 0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        uint64_t best[OWN];
#pragma unroll
        for (int j = 0; j < OWN; ++j) {
            best[j] = cur[j];
            if (!live[j]) continue;
            const int li = (ly0 + (THREADS / T) * j + 1) * LW + lx + 1;
#pragma unroll
            for (int k = 0; k < NM; ++k)
                best[j] = acc::better(best[j], acc::offer(key_lds[li + acc::move_dy(k) * LW + acc::move_dx(k)], w[j][k], bound));
        }
        __syncthreads();  // every gather of this sweep has read
        changed = 0;
#pragma unroll
        for (int j = 0; j < OWN; ++j) {
            if (best[j] < cur[j]) {
                cur[j] = best[j];
                key_lds[(ly0 + (THREADS / T) * j + 1) * LW + lx + 1] = best[j];
                changed = 1;
            }
        }
        changed = __syncthreads_or(changed);
        if (!changed) break;
    }

    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        if (cur[j] < was[j]) {  // only a pixel inside the frame has a move, so only such a pixel is lowered
            const int ly = ly0 + (THREADS / T) * j;
            store_key(keys + frame + (size_t)(y0 + ly) * W + (x0 + lx), cur[j]);
            const bool left = lx == 0, right = lx == T - 1, up = ly == 0, down = ly == T - 1;
            m |= 0x100u | (left ? 1u : 0u) | (right ? 2u : 0u) | (up ? 4u : 0u) | (down ? 8u : 0u) | (left && up ? 16u : 0u) | (right && up ? 32u : 0u) |
                 (left && down ? 64u : 0u) | (right && down ? 128u : 0u);
        }
    }
    if (m) atomicOr(&marks, m);
    __syncthreads();
    const unsigned all = marks;
    if (tid < acc::MOVES) {  // the neighbour tile in direction tid of the move table holds a lowered pixel in its ring
        const int nx = bx + acc::move_dx(tid), ny = by + acc::move_dy(tid);
        if (((all >> tid) & 1u) && nx >= 0 && nx < tiles_x && ny >= 0 && ny < tiles_y) next[(unsigned)ny * tiles_x + nx] = 1u;
    } else if (tid == 8) {
        if (all & 0x100u) words[(size_t)f * 4 + par] = 1u;
    } else if (tid == 9) {
        if (changed) next[tile] = 1u;  // the cap was reached: this tile goes on in the next round
    }
}

// ------------------------------------------------------------------ mask_access 3: the planes and the status row
__global__ __launch_bounds__(256) void access_finish_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ words, unsigned HW, unsigned tiles, int rounds,
                                                            uint32_t* __restrict__ d, int32_t* __restrict__ origin, int32_t* status) {
    __shared__ unsigned valued;
    const unsigned i = blockIdx.x * 256u + threadIdx.x, f = blockIdx.y, n = gridDim.y;
    if (threadIdx.x == 0) valued = 0u;
    __syncthreads();
    bool has = false;
    if (i < HW) {
        const size_t at = (size_t)f * HW + i;
        const uint64_t key = keys[at];
        has = key != acc::NO_KEY;
        d[at] = acc::key_cost(key);
        if (origin) origin[at] = has ? acc::key_origin(key) : -1;
    }
    const unsigned long long b = __ballot(has);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&valued, (unsigned)__popcll(b));
    if (i < tiles && flags[((size_t)(rounds & 1) * n + f) * tiles + i] != 0u) status[f * 4u] = 0;  // a tile is still dirty: not converged
    if (i == 0u) status[f * 4u + 1] = (int32_t)(words[f * 4u + 2] + words[f * 4u + ((rounds - 1) & 1)]);
    __syncthreads();
    if (threadIdx.x == 0 && valued) atomicAdd(status + f * 4u + 2, (int)valued);
}

// ------------------------------------------------------------------ region_access 1: the rows before the sums
// row word 0 = all ones (the minimum's start), the other seven and the reach table 0
__global__ __launch_bounds__(256) void reach_setup_kernel(unsigned long long* __restrict__ reach, int reach_words, unsigned long long* __restrict__ rows,
                                                          int row_words) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i < reach_words) reach[(size_t)f * reach_words + i] = 0ull;
    if (i < row_words) rows[(size_t)f * row_words + i] = (i & 7) == 0 ? acc::NO_KEY : 0ull;
}

__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_max32(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d));
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// pixels of one class join its cell of the LDS table: (pixels, pixels with a value, the sum of the values, the largest)
__device__ __forceinline__ void reach_cell(unsigned long long* cell, unsigned pixels, unsigned valued, unsigned long long sum, unsigned most) {
    atomicAdd(cell, (unsigned long long)pixels);
    if (valued) {
        atomicAdd(cell + 1, (unsigned long long)valued);
        atomicAdd(cell + 2, sum);
        atomicMax(cell + 3, (unsigned long long)most);
    }
}

__device__ __forceinline__ int written_rows(const long long* __restrict__ counts, int f, int max_regions) {
    const long long rows = counts[2 * (size_t)f + 1];
    return (int)(rows < 0 ? 0 : rows > max_regions ? max_regions : rows);
}

// one run of a region's pixels goes to its row: the minimum only where it would lower the word
__device__ __forceinline__ void reach_flush(unsigned long long* table, int lane, int r, unsigned long long key, unsigned count, unsigned most) {
    if (lane != 0 || r < 0) return;
    unsigned long long* row = table + (size_t)r * 8;
    if (key < __atomic_load_n(row, __ATOMIC_RELAXED)) atomicMin(row, key);
    atomicAdd(row + 6, (unsigned long long)count);
    if ((unsigned long long)most > __atomic_load_n(row + 7, __ATOMIC_RELAXED)) atomicMax(row + 7, (unsigned long long)most);
}

// ------------------------------------------------------------------ region_access 2: one pass over the frame's pixels
// As region_proximity's: a wave owns ACC_STEPS x 64 CONSECUTIVE pixels, so what it meets is runs of the same row; it keeps one
// (row, minimum, count, maximum) in registers and sends it to memory when the row changes and at its end.  The class table is summed in
// LDS: [class][pixels, pixels with a value, the sum of the values, the largest value].
__global__ __launch_bounds__(ACC_THREADS) void reach_accumulate_kernel(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ d,
                                                                       const int* __restrict__ index, const long long* __restrict__ counts, unsigned HW,
                                                                       int K, int max_regions, unsigned long long* reach, unsigned long long* rows_out) {
    extern __shared__ unsigned long long cells[];  // [K][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.y;
    for (int i = tid; i < K * 4; i += ACC_THREADS) cells[i] = 0ull;
    __syncthreads();
    const int rows = written_rows(counts, f, max_regions);
    const size_t frame = (size_t)f * HW;
    unsigned long long* table = rows_out + (size_t)f * max_regions * 8;
    const uint64_t first = ((uint64_t)blockIdx.x * (ACC_THREADS / 64) + wave) * (uint64_t)(ACC_STEPS * 64);
    int run_row = -1;
    unsigned long long run_key = acc::NO_KEY;
    unsigned run_count = 0, run_most = 0;
    for (int step = 0; step < ACC_STEPS; ++step) {  // uniform in the wave: the ballots and shuffles below are whole
        const uint64_t p = first + (uint64_t)step * 64 + lane;
        int r = -1;
        unsigned long long key = acc::NO_KEY;
        unsigned v = 0, val = 0;
        int cls = -1;
        bool valued = false;
        if (p < HW) {
            const uint32_t dv = d[frame + p];
            const int m = mask[frame + p];
            const bool has = dv != acc::NONE;
            cls = m < K ? m : -1;
            val = has ? dv : 0u, valued = has;
            if (has) {
                const int i = index[frame + p];
                if (i >= 0 && i < rows) {  // an index read from memory is checked before use
                    r = i;
                    key = acc::make_key(dv, (uint32_t)p);
                    v = dv;
                }
            }
        }
        // the class table: one set of LDS atomics per wave where all its pixels are of one class, one per pixel otherwise
        const unsigned long long counted = __ballot(cls >= 0);
        if (counted) {
            const int lead = __ffsll((long long)counted) - 1, cell = __shfl(cls, lead);
            if (__ballot(cls >= 0 && cls != cell) == 0ull) {
                const bool in = cls >= 0 && valued;
                const unsigned long long with = __ballot(in), sum = wave_sum64(in ? val : 0u);
                const unsigned most = wave_max32(in ? val : 0u);
                if (lane == lead) reach_cell(cells + cell * 4, (unsigned)__popcll(counted), (unsigned)__popcll(with), sum, most);
            } else if (cls >= 0) {
                reach_cell(cells + cls * 4, 1u, valued ? 1u : 0u, val, val);
            }
        }
        unsigned long long todo = __ballot(r >= 0);
        while (todo) {  // at most 64 turns: every turn takes at least the leading lane out
            const int lead = __ffsll((long long)todo) - 1, r0 = __shfl(r, lead);
            const bool own = r == r0;
            const unsigned long long k = wave_min64(own ? key : acc::NO_KEY);
            const unsigned most = wave_max32(own ? v : 0u);
            const unsigned c = (unsigned)__popcll(__ballot(own));
            if (r0 == run_row) {
                run_key = k < run_key ? k : run_key;
                run_most = max(run_most, most);
                run_count += c;
            } else {
                reach_flush(table, lane, run_row, run_key, run_count, run_most);
                run_row = r0, run_key = k, run_count = c, run_most = most;
            }
            todo &= ~__ballot(own);
        }
    }
    reach_flush(table, lane, run_row, run_key, run_count, run_most);
    __syncthreads();
    for (int i = tid; i < K * 4; i += ACC_THREADS) {
        const unsigned long long v = cells[i];
        if (!v) continue;
        unsigned long long* out = reach + (size_t)f * K * 4 + i;
        if ((i & 3) == 3) atomicMax(out, v);
        else atomicAdd(out, v);
    }
}

// ------------------------------------------------------------------ region_access 3: the minimum's word becomes the row
__global__ __launch_bounds__(256) void reach_finish_kernel(const int* __restrict__ origin, const int* __restrict__ index, const long long* __restrict__ counts,
                                                           int W, unsigned HW, int max_regions, long long* __restrict__ rows_out) {
    const int r = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (r >= max_regions) return;
    const int rows = written_rows(counts, f, max_regions);
    long long* row = rows_out + ((size_t)f * max_regions + r) * 8;
    const unsigned long long key = (unsigned long long)row[0];
    long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < rows) {
        if (key == acc::NO_KEY) {
            v[0] = v[1] = v[2] = v[3] = v[4] = v[5] = v[7] = -1;
        } else {
            const unsigned p = min((unsigned)(uint32_t)key, HW - 1u);
            v[0] = (long long)acc::key_cost(key);
            v[1] = p % (unsigned)W, v[2] = p / (unsigned)W;
            v[3] = v[4] = v[5] = -1;
            v[6] = row[6], v[7] = row[7];
            if (origin) {
                const int q = origin[(size_t)f * HW + p];
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

int check_frames(const char* op, int n, int H, int W) {
    FS_REQUIRE(n >= 1, "%s: at least one frame, got n=%d", op, n);
    FS_REQUIRE(n <= 65535, "%s: at most 65535 frames per call, got n=%d", op, n);
    FS_REQUIRE(H >= 1 && W >= 1, "%s: sizes must be >= 1, got %dx%d", op, H, W);
    FS_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 1, "%s: a frame of 2^31 - 1 pixels or more (%dx%d)", op, H, W);
    FS_REQUIRE(H <= acc::MAX_SIDE && W <= acc::MAX_SIDE, "%s: sizes must be <= %d, got %dx%d", op, acc::MAX_SIDE, H, W);
    return 0;
}

}  // namespace

int launch_mask_access(const uint8_t* mask, const uint8_t* seeds, int n, int H, int W, const uint8_t* cost, uint32_t terminal_set, int connectivity,
                       uint32_t max_cost, int rounds, int resume, uint32_t* d, int32_t* origin, int32_t* status, void* workspace, hipStream_t s) {
    FS_REQUIRE(mask && seeds && cost && d && status && workspace, "mask_access: null pointer");
    FS_TRY(check_frames("mask_access", n, H, W));
    FS_REQUIRE(connectivity == 4 || connectivity == 8, "mask_access: connectivity must be 4 or 8, got %d", connectivity);
    FS_REQUIRE(max_cost <= acc::MAX_COST, "mask_access: max_cost=%u out of range (0..%u, 0: the largest)", max_cost, acc::MAX_COST);
    FS_REQUIRE(rounds >= 1 && rounds <= acc::MAX_ROUNDS, "mask_access: rounds=%d out of range (1..%d)", rounds, acc::MAX_ROUNDS);
    FS_REQUIRE(resume == 0 || resume == 1, "mask_access: resume must be 0 or 1, got %d", resume);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(d) % 4 == 0, "mask_access: d is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(origin) % 4 == 0, "mask_access: origin is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(status) % 4 == 0, "mask_access: status is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "mask_access: the workspace is not aligned to 8 bytes");
    KindTable table = {};
    bool any = false;
    for (int k = 0; k < acc::MAX_CLASSES; ++k) {  // the caller's host array
        table.kind[k] = (uint16_t)acc::kind_of(k, cost, terminal_set);
        any |= table.kind[k] != 0;
    }
    FS_REQUIRE(any, "mask_access: the cost table is all zero (cost[k] > 0: class k can be walked on)");
    const int tiles_x = cdiv(W, T), tiles_y = cdiv(H, T);  // <= 1024 each
    const unsigned HW = (unsigned)H * (unsigned)W, tiles = (unsigned)tiles_x * (unsigned)tiles_y;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace);
    uint32_t* flags = reinterpret_cast<uint32_t*>(keys + (size_t)n * HW);
    uint32_t* words = flags + 2 * (size_t)n * tiles;
    const dim3 pixel_grid((HW + 255u) / 256u, (unsigned)n);  // HW >= tiles, 4
    hipLaunchKernelGGL(access_init_kernel, pixel_grid, dim3(256), 0, s, mask, seeds, table, HW, tiles, resume, d, origin, keys, flags, words, status);
    const uint32_t bound = acc::bound_of(max_cost);
    auto round_kernel = connectivity == 8 ? access_round_kernel<true> : access_round_kernel<false>;
    const dim3 tile_grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)n);
    for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(round_kernel, tile_grid, dim3(THREADS), 0, s, mask, table, H, W, bound, r, keys, flags, words);
    hipLaunchKernelGGL(access_finish_kernel, pixel_grid, dim3(256), 0, s, keys, flags, words, HW, tiles, rounds, d, origin, status);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_region_access(const uint8_t* mask, const uint32_t* d, const int32_t* origin, const int32_t* index, const long long* counts, int n, int H, int W,
                         int K, int max_regions, long long* reach, long long* rows, hipStream_t s) {
    FS_REQUIRE(mask && d && index && counts && reach && rows, "region_access: null pointer");
    FS_TRY(check_frames("region_access", n, H, W));
    FS_REQUIRE(K >= 1 && K <= 255, "region_access: classes=%d out of range (1..255)", K);
    FS_REQUIRE(max_regions >= 1 && max_regions <= 65536, "region_access: max_regions=%d out of range (1..65536)", max_regions);
    FS_REQUIRE(reinterpret_cast<uintptr_t>(d) % 4 == 0 && reinterpret_cast<uintptr_t>(origin) % 4 == 0 && reinterpret_cast<uintptr_t>(index) % 4 == 0,
               "region_access: d, origin or index is not aligned to 4 bytes");
    FS_REQUIRE(reinterpret_cast<uintptr_t>(counts) % 8 == 0 && reinterpret_cast<uintptr_t>(reach) % 8 == 0 && reinterpret_cast<uintptr_t>(rows) % 8 == 0,
               "region_access: counts, reach or rows is not aligned to 8 bytes");
    const unsigned HW = (unsigned)H * (unsigned)W;
    const int reach_words = K * 4, row_words = max_regions * 8;
    unsigned long long* reach_u = reinterpret_cast<unsigned long long*>(reach);
    unsigned long long* rows_u = reinterpret_cast<unsigned long long*>(rows);
    hipLaunchKernelGGL(reach_setup_kernel, dim3((unsigned)cdiv(std::max(reach_words, row_words), 256), (unsigned)n), dim3(256), 0, s, reach_u, reach_words,
                       rows_u, row_words);
    const unsigned acc_grid = (HW + ACC_THREADS * ACC_STEPS - 1u) / (ACC_THREADS * ACC_STEPS);  // <= 2^19
    hipLaunchKernelGGL(reach_accumulate_kernel, dim3(acc_grid, (unsigned)n), dim3(ACC_THREADS), (size_t)K * 4 * sizeof(unsigned long long), s, mask, d, index,
                       counts, HW, K, max_regions, reach_u, rows_u);
    hipLaunchKernelGGL(reach_finish_kernel, dim3((unsigned)cdiv(max_regions, 256), (unsigned)n), dim3(256), 0, s, origin, index, counts, W, HW, max_regions,
                       rows);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
