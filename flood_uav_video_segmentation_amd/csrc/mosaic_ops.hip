// The flood-extent mosaic on the GPU (include/floodseg_test.h: global_motion, pose_chain, mosaic_accumulate, mosaic_resolve; DESIGN
// §3.18).  OUR DEFINITION -- the reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.  Every rule -- what a
// usable row is, the mode's order, a round's tolerance and inlier test, the float64 solve and the conversion to mask pixels, the
// composition, the chain's bridge and lost rules, the gather's rounding, a vote's saturation, the resolve's tie -- is mosaic_defs.h's
// (__host__ __device__, also run on the CPU by the tests); this file is the launches:
//   global_motion      one workgroup of 1024 threads per frame pair: the 65 x 65 histogram of the usable vectors in LDS, its mode by a
//                      wave-then-workgroup maximum of a packed key, then per round one strided pass over the table (re-read from L2)
//                      that classifies and takes twelve int64 sums, reduced by shuffles and across the waves in LDS; thread 0 solves
//                      and broadcasts through LDS.  No global atomics, no scratch buffer, nothing between workgroups.
//   pose_chain         one wave; lane 0 walks the n <= 64 frames through pose_step.
//   mosaic_accumulate  one workgroup per 64 x 16 canvas tile: the first wave tests every frame's pose against the tile (status, bounds,
//                      the bounding box of the tile's four corners under from_anchor) and keeps the frames that can touch it in LDS; a
//                      tile that no frame touches reads and writes nothing more.  A thread owns its canvas pixels: no atomics.
//   mosaic_resolve     one pass over the canvas; the per-class totals through an LDS histogram per workgroup, flushed with one 64-bit
//                      atomic per non-zero cell (integer sums: the order does not matter).
// Every loop bound follows from the arguments; no thread waits for another workgroup; every value read from device memory that becomes
// an index or an operand of a product is tested first (mask ids, a row's block centre and vector, a model's and a pose's status and
// magnitudes, the state's phase).
#include "kernels.h"
#include "map_checks.h"
#include "mosaic_defs.h"

namespace fs {

namespace {

constexpr int GM_THREADS = 1024, GM_WAVES = GM_THREADS / 64;
constexpr int TILE_W = 64, TILE_H = 16, ACC_THREADS = 256;  // a thread owns column tid & 63 of rows tid >> 6, + 4, + 8, + 12
constexpr int RES_THREADS = 256, RES_PIXELS = 4;            // canvas pixels per thread of the resolve pass

// ------------------------------------------------------------------ workgroup reductions of global_motion (all 1024 threads call them)
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

struct GmShared {
    unsigned hist[mos::HIST_BINS];
    long long part[GM_WAVES][mos::SUMS];  // one row per wave
    long long sums[mos::SUMS];            // the workgroup's
    unsigned long long key_part[GM_WAVES];
    unsigned long long key;
    long long model[6];
    int stop;
};

// usable: the vector, the block coordinates; false otherwise
__device__ __forceinline__ bool usable_row(const int32_t* __restrict__ row, const uint8_t* __restrict__ mask, uint32_t exclude_set, int FH, int FW, int H, int W,
                                           int hb, int wb, int* p, int* q, int* dx, int* dy) {
    if (!mos::row_vector(row, FH, FW, dx, dy)) return false;
    const int tx = row[5], ty = row[6];  // inside the frame: row_vector tested them
    if (mask && mos::excluded(mask[(size_t)mos::centre_y(ty, H, FH) * W + mos::centre_x(tx, W, FW)], exclude_set)) return false;
    *p = mos::block_p(tx, wb), *q = mos::block_q(ty, hb);
    return true;
}

__global__ __launch_bounds__(GM_THREADS) void global_motion_kernel(const int32_t* __restrict__ tables, const int32_t* __restrict__ pair_stats,
                                                                   const uint8_t* __restrict__ mask, uint32_t exclude_set, int blocks, int FH, int FW, int H,
                                                                   int W, int rounds, long long tol_q20, int min_inliers, long long* __restrict__ model_out) {
    __shared__ GmShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
    const int hb = FH / 16, wb = FW / 16;
    int64_t* out = reinterpret_cast<int64_t*>(model_out) + (size_t)f * mos::MODEL_WORDS;
    int64_t fwd[6], inv[6];
    if (pair_stats && pair_stats[4 * (size_t)f + 2] != 0) {  // uniform in the workgroup: a cut is not fitted
        if (tid == 0) {
            mos::identity(fwd), mos::identity(inv);
            mos::write_model(out, fwd, inv, mos::MODEL_CUT, 0, 0, 0);
        }
        return;
    }
    const int32_t* table = tables + (size_t)f * blocks * 7;
    const uint8_t* plane = mask ? mask + (size_t)f * H * W : nullptr;
    for (int i = tid; i < mos::HIST_BINS; i += GM_THREADS) sh.hist[i] = 0u;
    __syncthreads();
    long long mine = 0;
    for (int i = tid; i < blocks; i += GM_THREADS) {
        int p, q, dx, dy;
        if (usable_row(table + (size_t)i * 7, plane, exclude_set, FH, FW, H, W, hb, wb, &p, &q, &dx, &dy)) {
            atomicAdd(&sh.hist[mos::hist_bin(dx, dy)], 1u);
            ++mine;
        }
    }
    mine = wave_sum(mine);
    if (lane == 0) sh.part[wave][0] = mine;
    __syncthreads();
    unsigned long long key = 0ull;
    for (int i = tid; i < mos::HIST_BINS; i += GM_THREADS) {
        const unsigned long long k = mos::mode_key(sh.hist[i], i);
        key = k > key ? k : key;
    }
    key = wave_max(key);
    if (lane == 0) sh.key_part[wave] = key;
    __syncthreads();
    if (tid == 0) {
        long long usable = 0;
        unsigned long long best = 0ull;
        for (int w = 0; w < GM_WAVES; ++w) {
            usable += sh.part[w][0];
            best = sh.key_part[w] > best ? sh.key_part[w] : best;
        }
        sh.sums[0] = usable;
        sh.key = best;
        sh.model[0] = (long long)mos::key_dx(best) * mos::ONE, sh.model[1] = 0, sh.model[2] = 0;
        sh.model[3] = (long long)mos::key_dy(best) * mos::ONE, sh.model[4] = 0, sh.model[5] = 0;
        sh.stop = 0;
    }
    __syncthreads();
    const long long usable = sh.sums[0];
    long long inliers = (long long)mos::key_count(sh.key);  // rounds == 0: the mode's count
    int status = usable < min_inliers ? mos::MODEL_FEW : mos::MODEL_OK, done = 0;
    for (int r = 0; r < rounds && status == mos::MODEL_OK; ++r) {  // status and the exit below are uniform in the workgroup
        int64_t model[6];
        for (int i = 0; i < 6; ++i) model[i] = sh.model[i];
        const int64_t T = mos::round_tolerance(tol_q20, rounds, r);
        int64_t s[mos::SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < blocks; i += GM_THREADS) {
            int p, q, dx, dy;
            if (usable_row(table + (size_t)i * 7, plane, exclude_set, FH, FW, H, W, hb, wb, &p, &q, &dx, &dy) && mos::is_inlier(model, p, q, dx, dy, T))
                mos::add_row(s, p, q, dx, dy);
        }
#pragma unroll
        for (int j = 0; j < mos::SUMS; ++j) {
            const long long v = wave_sum((long long)s[j]);
            if (lane == 0) sh.part[wave][j] = v;
        }
        __syncthreads();
        if (tid < mos::SUMS) {
            long long v = 0;
            for (int w = 0; w < GM_WAVES; ++w) v += sh.part[w][tid];
            sh.sums[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {
            int64_t sums[mos::SUMS], next[6];
            for (int j = 0; j < mos::SUMS; ++j) sums[j] = sh.sums[j];
            int stop = 0;
            if (sums[0] < min_inliers) stop = 1;
            else if (!mos::gm_solve(sums, next)) stop = 2;
            else
                for (int i = 0; i < 6; ++i) sh.model[i] = next[i];
            sh.stop = stop;
        }
        __syncthreads();
        const int stop = sh.stop;
        if (stop) {
            if (r == 0) status = stop == 1 ? mos::MODEL_FEW : mos::MODEL_DEGENERATE;
            break;  // a later round: the model of the round before stands
        }
        inliers = sh.sums[0];
        done = r + 1;
        __syncthreads();  // sh.sums and sh.part are written again by the next round
    }
    if (tid != 0) return;
    if (status == mos::MODEL_OK) {
        int64_t model[6];
        for (int i = 0; i < 6; ++i) model[i] = sh.model[i];
        if (!mos::gm_finish(model, FH, FW, H, W, fwd, inv)) status = mos::MODEL_DEGENERATE;
    }
    if (status != mos::MODEL_OK) mos::identity(fwd), mos::identity(inv);
    mos::write_model(out, fwd, inv, status, usable, inliers, done);
}

// ------------------------------------------------------------------ pose_chain: lane 0 walks the frames
__global__ __launch_bounds__(64) void pose_chain_kernel(const long long* __restrict__ model, long long* __restrict__ state, long long* __restrict__ poses, int n,
                                                        int H, int W, int CH, int CW, int ox, int oy, int max_bridge) {
    // the wave moves the rows between memory and LDS together (one trip each way, not one per word); the walk itself is serial
    __shared__ int64_t rows[mos::MAX_FRAMES * mos::MODEL_WORDS];  // model rows in, pose rows out, in place (n <= 64 was checked)
    __shared__ int64_t st[mos::STATE_WORDS];
    static_assert(mos::MODEL_WORDS == mos::POSE_WORDS, "a pose row takes its model row's place");
    const int lane = threadIdx.x;
    for (int i = lane; i < n * mos::MODEL_WORDS; i += 64) rows[i] = model[i];
    if (lane < mos::STATE_WORDS) st[lane] = state[lane];
    __syncthreads();
    if (lane == 0) {
        for (int f = 0; f < n; ++f) {
            int64_t row[mos::MODEL_WORDS], pose[mos::POSE_WORDS];
            for (int i = 0; i < mos::MODEL_WORDS; ++i) row[i] = rows[f * mos::MODEL_WORDS + i];
            mos::pose_step(row, st, pose, H, W, CH, CW, ox, oy, max_bridge);
            for (int i = 0; i < mos::POSE_WORDS; ++i) rows[f * mos::POSE_WORDS + i] = pose[i];
        }
    }
    __syncthreads();
    for (int i = lane; i < n * mos::POSE_WORDS; i += 64) poses[i] = rows[i];
    if (lane < mos::STATE_WORDS) state[lane] = st[lane];
}

// ------------------------------------------------------------------ mosaic_accumulate: one workgroup per canvas tile
// The source pixel is computed from the products for every pixel and frame.  Stepping sx by from_anchor[0] per pixel along a row WOULD be
// bit-equal (AX advances by exactly ONE, so the sum under the rshr advances by a multiple of 2^20, which the shift passes through), but a
// thread owns one pixel of a row, not a run of them: there is no walk to save, and two 64-bit multiplies per frame are not what this
// kernel waits for.
__global__ __launch_bounds__(ACC_THREADS) void mosaic_accumulate_kernel(const uint8_t* __restrict__ mask, const long long* __restrict__ poses, int n, int H,
                                                                        int W, int K, int CH, int CW, int ox, int oy, uint16_t* __restrict__ votes) {
    __shared__ long long live_pose[mos::MAX_FRAMES][6];  // from_anchor of the frames that can touch the tile, in frame order
    __shared__ int live_frame[mos::MAX_FRAMES];
    __shared__ int live_count;
    const int tid = threadIdx.x, X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * TILE_H;
    const int X1 = min(X0 + TILE_W, CW), Y1 = min(Y0 + TILE_H, CH);
    if (tid < 64) {  // the first wave: frame tid
        int64_t pose[mos::POSE_WORDS];
        bool live = false;
        if (tid < n) {
            for (int i = 0; i < mos::POSE_WORDS; ++i) pose[i] = poses[(size_t)tid * mos::POSE_WORDS + i];
            live = mos::pose_votes(pose) && mos::touches(pose + 6, X0, Y0, X1, Y1, ox, oy, H, W);
        }
        const unsigned long long set = __ballot(live);
        if (live) {
            const int slot = __popcll(set & (((unsigned long long)1 << tid) - 1ull));
            live_frame[slot] = tid;
            for (int i = 0; i < 6; ++i) live_pose[slot][i] = pose[6 + i];
        }
        if (tid == 0) live_count = __popcll(set);
    }
    __syncthreads();
    const int count = live_count;
    if (count == 0) return;  // nothing is read or written
    const int X = X0 + (tid & 63);
    if (X >= CW) return;
    const int64_t AX = mos::anchor_coord(X, ox);
    const size_t plane = (size_t)CH * CW;
    for (int Y = Y0 + (tid >> 6); Y < Y1; Y += ACC_THREADS / 64) {
        const int64_t AY = mos::anchor_coord(Y, oy);
        uint16_t* cell = votes + (size_t)Y * CW + X;
        int run_k = -1;         // consecutive frames mostly vote for one class: the votes of a run go to memory together
        uint32_t run_votes = 0;
        for (int j = 0; j < count; ++j) {
            int64_t from_anchor[6];
            for (int i = 0; i < 6; ++i) from_anchor[i] = live_pose[j][i];
            int64_t x, y;
            mos::source_pixel(from_anchor, AX, AY, &x, &y);
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            const int k = mask[((size_t)live_frame[j] * H + (size_t)y) * W + (size_t)x];
            if (k >= K) continue;  // a mask id is tested before it becomes a plane index
            if (k != run_k) {
                if (run_votes) cell[run_k * plane] = mos::vote_add(cell[run_k * plane], run_votes);
                run_k = k, run_votes = 0;
            }
            ++run_votes;
        }
        if (run_votes) cell[run_k * plane] = mos::vote_add(cell[run_k * plane], run_votes);
    }
}

// ------------------------------------------------------------------ mosaic_resolve
__global__ __launch_bounds__(64) void mosaic_totals_clear_kernel(unsigned long long* __restrict__ totals, int K) {
    if ((int)threadIdx.x < 2 * K) totals[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(RES_THREADS) void mosaic_resolve_kernel(const uint16_t* __restrict__ votes, int K, unsigned long long pixels,
                                                                     uint8_t* __restrict__ cls, uint8_t* __restrict__ conf, uint32_t* __restrict__ seen,
                                                                     unsigned long long* totals) {
    __shared__ unsigned hist[mos::MAX_CLASSES][2];  // per class the pixels won and the votes received: at most 1024 pixels x 65535 < 2^32
    const int tid = threadIdx.x;
    if (tid < 2 * mos::MAX_CLASSES) hist[tid >> 1][tid & 1] = 0u;
    __syncthreads();
    const unsigned long long first = (unsigned long long)blockIdx.x * (RES_THREADS * RES_PIXELS);
    uint32_t most[RES_PIXELS], total[RES_PIXELS];
    int best[RES_PIXELS];
#pragma unroll
    for (int step = 0; step < RES_PIXELS; ++step) most[step] = 0u, total[step] = 0u, best[step] = 255;
    for (int k = 0; k < K; ++k) {
        uint32_t got = 0u;  // the class's votes on this thread's pixels: at most 4 x 65535
#pragma unroll
        for (int step = 0; step < RES_PIXELS; ++step) {
            const unsigned long long p = first + (unsigned long long)step * RES_THREADS + tid;
            if (p < pixels) {
                const uint32_t v = votes[(size_t)k * pixels + p];
                got += v;
                total[step] += v;
                if (v > most[step]) most[step] = v, best[step] = k;  // strictly more: the lowest id wins a tie
            }
        }
        if (got) atomicAdd(&hist[k][1], got);
    }
#pragma unroll
    for (int step = 0; step < RES_PIXELS; ++step) {
        const unsigned long long p = first + (unsigned long long)step * RES_THREADS + tid;
        if (p < pixels) {
            cls[p] = (uint8_t)best[step];
            conf[p] = mos::vote_confidence(most[step], total[step]);
            seen[p] = total[step];
            if (total[step]) atomicAdd(&hist[best[step]][0], 1u);
        }
    }
    __syncthreads();
    if (tid < 2 * K && hist[tid >> 1][tid & 1]) atomicAdd(totals + tid, (unsigned long long)hist[tid >> 1][tid & 1]);
}

}  // namespace

int launch_global_motion(const int32_t* tables, const int32_t* pair_stats, const uint8_t* mask, uint32_t exclude_set, int n, int FH, int FW, int H, int W,
                         int rounds, long long tol_q20, int min_inliers, long long* model, hipStream_t s) {
    FS_REQUIRE(tables && model, "global_motion: null pointer");
    FS_REQUIRE(n >= 1 && n <= mos::MAX_FRAMES, "global_motion: n must be 1..%d frame pairs, got n=%d", mos::MAX_FRAMES, n);
    FS_TRY(check_sides("global_motion", "the frame", 16, FH, FW));
    FS_TRY(check_sides("global_motion", "the mask", 1, H, W));
    FS_REQUIRE(rounds >= 0 && rounds <= mos::MAX_ROUNDS, "global_motion: rounds=%d out of range (0..%d)", rounds, mos::MAX_ROUNDS);
    FS_REQUIRE(tol_q20 >= 0 && tol_q20 <= mos::MAX_TOL_Q20, "global_motion: tol_q20=%lld out of range (0..%lld: 64 pixels)", tol_q20, (long long)mos::MAX_TOL_Q20);
    FS_REQUIRE(min_inliers >= 3 && min_inliers <= (1 << 20), "global_motion: min_inliers=%d out of range (3..%d)", min_inliers, 1 << 20);
    FS_REQUIRE(aligned(tables, 4) && aligned(pair_stats, 4), "global_motion: tables or pair_stats is not aligned to 4 bytes");
    FS_REQUIRE(aligned(model, 8), "global_motion: model is not aligned to 8 bytes");
    const int blocks = (FH / 16) * (FW / 16);
    hipLaunchKernelGGL(global_motion_kernel, dim3((unsigned)n), dim3(GM_THREADS), 0, s, tables, pair_stats, mask, exclude_set, blocks, FH, FW, H, W, rounds,
                       tol_q20, min_inliers, model);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_pose_chain(const long long* model, long long* state, long long* poses, int n, int H, int W, int CH, int CW, int ox, int oy, int max_bridge,
                      hipStream_t s) {
    FS_REQUIRE(model && state && poses, "pose_chain: null pointer");
    FS_REQUIRE(n >= 1 && n <= mos::MAX_FRAMES, "pose_chain: n must be 1..%d frames, got n=%d", mos::MAX_FRAMES, n);
    FS_TRY(check_mask_on_canvas("pose_chain", 1, H, W, CH, CW, ox, oy));
    FS_REQUIRE(max_bridge >= 0 && max_bridge <= mos::MAX_FRAMES, "pose_chain: max_bridge=%d out of range (0..%d)", max_bridge, mos::MAX_FRAMES);
    FS_REQUIRE(aligned(model, 8) && aligned(state, 8) && aligned(poses, 8), "pose_chain: model, state or poses is not aligned to 8 bytes");
    hipLaunchKernelGGL(pose_chain_kernel, dim3(1), dim3(64), 0, s, model, state, poses, n, H, W, CH, CW, ox, oy, max_bridge);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_mosaic_accumulate(const uint8_t* mask, const long long* poses, int n, int H, int W, int K, int CH, int CW, int ox, int oy, uint16_t* votes,
                             hipStream_t s) {
    FS_REQUIRE(mask && poses && votes, "mosaic_accumulate: null pointer");
    FS_REQUIRE(n >= 1 && n <= mos::MAX_FRAMES, "mosaic_accumulate: n must be 1..%d frames, got n=%d", mos::MAX_FRAMES, n);
    FS_TRY(check_sides("mosaic_accumulate", "the mask", 1, H, W));
    FS_REQUIRE(K >= 1 && K <= mos::MAX_CLASSES, "mosaic_accumulate: classes=%d out of range (1..%d)", K, mos::MAX_CLASSES);
    FS_TRY(check_sides("mosaic_accumulate", "the canvas", 1, CH, CW));
    FS_TRY(check_origin("mosaic_accumulate", "the origin", ox, oy));
    FS_REQUIRE(aligned(poses, 8), "mosaic_accumulate: poses is not aligned to 8 bytes");
    FS_REQUIRE(aligned(votes, 2), "mosaic_accumulate: votes is not aligned to 2 bytes");
    hipLaunchKernelGGL(mosaic_accumulate_kernel, dim3((unsigned)cdiv(CW, TILE_W), (unsigned)cdiv(CH, TILE_H)), dim3(ACC_THREADS), 0, s, mask, poses, n, H, W,
                       K, CH, CW, ox, oy, votes);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_mosaic_resolve(const uint16_t* votes, int K, int CH, int CW, uint8_t* cls, uint8_t* conf, uint32_t* seen, long long* totals, hipStream_t s) {
    FS_REQUIRE(votes && cls && conf && seen && totals, "mosaic_resolve: null pointer");
    FS_REQUIRE(K >= 1 && K <= mos::MAX_CLASSES, "mosaic_resolve: classes=%d out of range (1..%d)", K, mos::MAX_CLASSES);
    FS_TRY(check_sides("mosaic_resolve", "the canvas", 1, CH, CW));
    FS_REQUIRE(aligned(votes, 2), "mosaic_resolve: votes is not aligned to 2 bytes");
    FS_REQUIRE(aligned(seen, 4), "mosaic_resolve: seen is not aligned to 4 bytes");
    FS_REQUIRE(aligned(totals, 8), "mosaic_resolve: totals is not aligned to 8 bytes");
    const unsigned long long pixels = (unsigned long long)CH * CW;  // <= 2^28
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(totals);
    hipLaunchKernelGGL(mosaic_totals_clear_kernel, dim3(1), dim3(64), 0, s, sums, K);
    hipLaunchKernelGGL(mosaic_resolve_kernel, dim3((unsigned)((pixels + RES_THREADS * RES_PIXELS - 1) / (RES_THREADS * RES_PIXELS))), dim3(RES_THREADS), 0, s,
                       votes, K, pixels, cls, conf, seen, sums);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
