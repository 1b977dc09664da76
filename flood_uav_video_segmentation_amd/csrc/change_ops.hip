// The flood-extent change between two registered mosaics (include/floodseg_test.h: mosaic_change).  OUR DEFINITION -- the
// reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.  The rules -- a pixel's decided class, a class as a set,
// the window OR, the change code, the tally's cells -- are change_defs.h's on top of merge_defs.h, whose gather (gather_affine, b_pixel,
// b_reaches) and link test (link_merges) are called, not restated (__host__ __device__, also run on the CPU by the tests).  This file
// is the launches, three on one stream:
//   change_clear    counts = (the link's status, 0, ...) and transitions = 0.  A kernel, not a memset node.
//   change_classes  one workgroup of 256 per 64 x 16 tile of A as in mosaic_accumulate.  A thread owns a column of four rows and loops
//                   over K: per pixel K coalesced uint16 reads of A, and K gathered reads of B where the B pixel exists.  A tile that B's
//                   canvas rectangle cannot reach, and every tile under a link that does not merge, resolves A alone and writes 255 to
//                   cls_b without touching B.  Every plane pixel has one owner; no atomics.
//   change_codes    the same tiles.  1u << cls of both planes is staged in LDS for the tile plus an apron of r pixels, clipped at the
//                   canvas edge; the window OR is done separably, rows first (each thread holds its results in registers across the
//                   barrier and writes them back in place), then columns.  r = 0 is an instantiation of its own that stages nothing.  The
//                   counts and transitions go through an LDS tally of 8 + 2 K^2 dwords: a thread merges the cells of its four pixels
//                   before the LDS add (almost every pixel of a tile lands in one cell), and the workgroup flushes with one 64-bit
//                   atomic per non-zero cell.  "reached" is the gather's arithmetic on the link again; B is not read.
// Every loop bound follows from the arguments; nothing is allocated, synchronised or read back on the host.
#include "kernels.h"
#include "map_checks.h"
#include "change_defs.h"  // after the HIP runtime: FS_MOS_HD is __host__ __device__ there

namespace fs {

namespace {

constexpr int THREADS = 256;
constexpr int ROWS = chg::TILE_H / (THREADS / chg::TILE_W);  // 4: the rows of a thread's column
constexpr int STAGE = chg::APRON_W * chg::APRON_H;           // 2560 dwords a plane at r = 8
constexpr int SPANS = chg::APRON_H * chg::TILE_W / THREADS;  // 8: row-OR results a thread holds per plane
constexpr int TALLY_MAX = chg::HEAD + 2 * mos::MAX_CLASSES * mos::MAX_CLASSES;
static_assert(chg::TILE_W == 64 && THREADS % chg::TILE_W == 0 && chg::TILE_H % (THREADS / chg::TILE_W) == 0, "a wave is one row of a tile");

// ------------------------------------------------------------------ change_clear
__global__ __launch_bounds__(THREADS) void change_clear_kernel(const long long* __restrict__ link, unsigned long long* __restrict__ counts,
                                                               unsigned long long* __restrict__ transitions, int cells) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < chg::COUNT_WORDS) counts[i] = i == 0 ? (unsigned long long)link[12] : 0ull;
    if (i < cells) transitions[i] = 0ull;
}

// ------------------------------------------------------------------ change_classes
__global__ __launch_bounds__(THREADS) void change_classes_kernel(const uint16_t* __restrict__ votes_a, int CH_a, int CW_a, int ox_a, int oy_a,
                                                                 const uint16_t* __restrict__ votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                                                                 const long long* __restrict__ link_row, int min_votes, int min_conf,
                                                                 uint8_t* __restrict__ cls_a, uint8_t* __restrict__ cls_b) {
    const int tid = threadIdx.x, X0 = blockIdx.x * chg::TILE_W, Y0 = blockIdx.y * chg::TILE_H;
    const int X1 = min(X0 + chg::TILE_W, CW_a), Y1 = min(Y0 + chg::TILE_H, CH_a);
    int64_t link[mrg::LINK_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < mrg::LINK_WORDS; ++i) link[i] = link_row[i];
    int64_t g[6] = {0, 0, 0, 0, 0, 0};
    bool reach = mrg::link_merges(link);  // uniform, decided here on the device; tested before any product
    if (reach) {
        mrg::gather_affine(link, ox_b, oy_b, g);
        reach = mrg::b_reaches(g, X0, Y0, X1, Y1, ox_a, oy_a, CH_b, CW_b);  // uniform
    }
    const int X = X0 + (tid & (chg::TILE_W - 1)), Yt = Y0 + tid / chg::TILE_W;
    if (X >= CW_a) return;
    const size_t plane_a = (size_t)CH_a * CW_a, plane_b = (size_t)CH_b * CW_b;
    chg::Winner wa[ROWS], wb[ROWS];
    size_t cell_b[ROWS];
    bool has_b[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int Y = Yt + i * (THREADS / chg::TILE_W);
        int bx = 0, by = 0;
        wa[i] = chg::no_votes(), wb[i] = chg::no_votes();
        has_b[i] = reach && Y < Y1 && mrg::b_pixel(g, X, Y, ox_a, oy_a, CH_b, CW_b, &bx, &by);
        cell_b[i] = has_b[i] ? (size_t)by * CW_b + (size_t)bx : 0;
    }
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int Y = Yt + i * (THREADS / chg::TILE_W);
            if (Y < Y1) chg::take_votes(&wa[i], k, votes_a[(size_t)k * plane_a + (size_t)Y * CW_a + X]);
            if (has_b[i]) chg::take_votes(&wb[i], k, votes_b[(size_t)k * plane_b + cell_b[i]]);
        }
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int Y = Yt + i * (THREADS / chg::TILE_W);
        if (Y >= Y1) continue;
        const size_t cell = (size_t)Y * CW_a + X;
        cls_a[cell] = chg::decided_class(wa[i], min_votes, min_conf);
        cls_b[cell] = has_b[i] ? chg::decided_class(wb[i], min_votes, min_conf) : chg::NONE;
    }
}

// ------------------------------------------------------------------ change_codes
// One plane's window sets of the tile: stage (TILE_H + 2 r) x (TILE_W + 2 r) sets, OR the rows in place, leave the columns to the caller.
// After it, sets[y * PW + x] for y < TILE_H + 2 r, x < TILE_W is the OR over the canvas pixels X0 + x - r .. X0 + x + r of row Y0 + y - r.
__device__ void stage_row_sets(const uint8_t* __restrict__ plane, int CH, int CW, int X0, int Y0, int r, uint32_t* sets) {
    const int tid = threadIdx.x, PW = chg::TILE_W + 2 * r, PH = chg::TILE_H + 2 * r;
    // all 256 threads over the staged cells: a wave per staged row leaves most lanes idle in the apron's columns and measured 10 % slower
    for (int i = tid; i < PW * PH; i += THREADS) sets[i] = chg::staged_bit(plane, CH, CW, X0 - r + i % PW, Y0 - r + i / PW);
    __syncthreads();
    uint32_t span[SPANS];  // (y, x) = (tid / 64 + 4 j, tid % 64): PH <= APRON_H rows of TILE_W
#pragma unroll
    for (int j = 0; j < SPANS; ++j) {
        const int y = tid / chg::TILE_W + j * (THREADS / chg::TILE_W);
        span[j] = y < PH ? chg::span_or(sets + y * PW + (tid & (chg::TILE_W - 1)), 1, r) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SPANS; ++j) {
        const int y = tid / chg::TILE_W + j * (THREADS / chg::TILE_W);
        if (y < PH) sets[y * PW + (tid & (chg::TILE_W - 1))] = span[j];
    }
    __syncthreads();
}

template <bool WINDOW>
__global__ __launch_bounds__(THREADS) void change_codes_kernel(const uint8_t* __restrict__ cls_a, const uint8_t* __restrict__ cls_b, int CH_a, int CW_a,
                                                               int ox_a, int oy_a, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                                                               const long long* __restrict__ link_row, int r, uint32_t watch_set,
                                                               uint8_t* __restrict__ change, unsigned long long* transitions, unsigned long long* counts) {
    __shared__ uint32_t tally[TALLY_MAX];
    __shared__ uint32_t sets_a[WINDOW ? STAGE : 1], sets_b[WINDOW ? STAGE : 1];
    const int tid = threadIdx.x, X0 = blockIdx.x * chg::TILE_W, Y0 = blockIdx.y * chg::TILE_H;
    const int X1 = min(X0 + chg::TILE_W, CW_a), Y1 = min(Y0 + chg::TILE_H, CH_a);
    const int cells = chg::tally_cells(K);
    for (int i = tid; i < cells; i += THREADS) tally[i] = 0u;
    int64_t link[mrg::LINK_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < mrg::LINK_WORDS; ++i) link[i] = link_row[i];
    int64_t g[6] = {0, 0, 0, 0, 0, 0};
    bool reach = mrg::link_merges(link);  // uniform
    if (reach) {
        mrg::gather_affine(link, ox_b, oy_b, g);
        reach = mrg::b_reaches(g, X0, Y0, X1, Y1, ox_a, oy_a, CH_b, CW_b);
    }
    if (WINDOW) {
        stage_row_sets(cls_a, CH_a, CW_a, X0, Y0, r, sets_a);
        stage_row_sets(cls_b, CH_a, CW_a, X0, Y0, r, sets_b);
    } else {
        __syncthreads();  // the tally is clear
    }
    const int tx = tid & (chg::TILE_W - 1), X = X0 + tx, PW = chg::TILE_W + 2 * r;
    uint32_t reached = 0u, codes = 0u;  // codes: six 4-bit counters of this thread's four pixels
    int run_cell = -1;                  // the transitions cell of the pixels before this one, and how many they were
    uint32_t run = 0u, run_changed = 0u;
    if (X < CW_a) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int ty = tid / chg::TILE_W + i * (THREADS / chg::TILE_W), Y = Y0 + ty;
            if (Y >= Y1) continue;
            const size_t cell = (size_t)Y * CW_a + X;
            const uint8_t ca = cls_a[cell], cb = cls_b[cell];
            int bx, by;
            reached += reach && mrg::b_pixel(g, X, Y, ox_a, oy_a, CH_b, CW_b, &bx, &by) ? 1u : 0u;
            uint32_t win_a = 0u, win_b = 0u;  // with r = 0 code 2 cannot occur: change_code tests the sets only where ca != cb
            if (WINDOW && ca != cb) win_a = chg::span_or(sets_a + ty * PW + tx, PW, r), win_b = chg::span_or(sets_b + ty * PW + tx, PW, r);
            const int code = chg::change_code(ca, cb, win_a, win_b, watch_set);
            change[cell] = (uint8_t)code;
            codes += 1u << (4 * code);
            if (code == chg::NOT_COMPARABLE) continue;
            const int here = chg::transition_cell(0, ca, cb, K);
            if (here != run_cell) {
                if (run) atomicAdd(&tally[chg::HEAD + run_cell], run);
                if (run_changed) atomicAdd(&tally[chg::HEAD + K * K + run_cell], run_changed);
                run_cell = here, run = 0u, run_changed = 0u;
            }
            run += 1u, run_changed += code >= chg::CHANGED_OTHER ? 1u : 0u;
        }
    }
    if (run) atomicAdd(&tally[chg::HEAD + run_cell], run);
    if (run_changed) atomicAdd(&tally[chg::HEAD + K * K + run_cell], run_changed);
    if (reached) atomicAdd(&tally[1], reached);
    uint32_t comparable = 0u;
#pragma unroll
    for (int c = chg::SAME; c < chg::CODES; ++c) {
        const uint32_t n = (codes >> (4 * c)) & 15u;
        comparable += n;
        if (n) atomicAdd(&tally[2 + c], n);  // counts[3..7]: same, explained, changed-other, gained, lost
    }
    if (comparable) atomicAdd(&tally[2], comparable);
    __syncthreads();
    for (int i = tid; i < cells; i += THREADS) {  // tally[0] stays 0: the status is change_clear's
        const uint32_t n = tally[i];
        if (n == 0u) continue;
        if (i < chg::HEAD)
            atomicAdd(counts + i, (unsigned long long)n);
        else
            atomicAdd(transitions + (i - chg::HEAD), (unsigned long long)n);
    }
}

bool overlaps(const void* p, size_t p_bytes, const void* q, size_t q_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + q_bytes && b < a + p_bytes;
}

}  // namespace

int launch_mosaic_change(const uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                         const long long* link, int min_votes, int min_conf, int tolerance, uint32_t watch_set, uint8_t* change, uint8_t* cls_a, uint8_t* cls_b,
                         long long* transitions, long long* counts, hipStream_t s) {
    FS_REQUIRE(votes_a && votes_b && link && change && cls_a && cls_b && transitions && counts, "mosaic_change: null pointer");
    FS_REQUIRE(K >= 1 && K <= mos::MAX_CLASSES, "mosaic_change: classes=%d out of range (1..%d)", K, mos::MAX_CLASSES);
    FS_TRY(check_canvases("mosaic_change", CH_a, CW_a, ox_a, oy_a, CH_b, CW_b, ox_b, oy_b));
    FS_REQUIRE(min_votes >= 1 && min_votes <= chg::MAX_VOTES, "mosaic_change: min_votes must be 1..%d, got %d", chg::MAX_VOTES, min_votes);
    FS_REQUIRE(min_conf >= 0 && min_conf <= chg::MAX_CONF, "mosaic_change: min_conf must be 0..%d, got %d", chg::MAX_CONF, min_conf);
    FS_REQUIRE(tolerance >= 0 && tolerance <= chg::MAX_TOLERANCE, "mosaic_change: tolerance must be 0..%d pixels, got %d", chg::MAX_TOLERANCE, tolerance);
    FS_REQUIRE(chg::watch_ok(watch_set, K), "mosaic_change: watch_set=0x%x has a bit at or above classes=%d", watch_set, K);
    FS_REQUIRE(votes_a != votes_b, "mosaic_change: A and B are the same memory");
    const size_t pixels = (size_t)CH_a * CW_a, cells = (size_t)2 * K * K;
    const struct { const void* p; size_t bytes; } ins[3] = {{votes_a, (size_t)K * pixels * 2}, {votes_b, (size_t)K * CH_b * CW_b * 2}, {link, mrg::LINK_WORDS * 8}},
                                                 outs[5] = {{change, pixels}, {cls_a, pixels}, {cls_b, pixels}, {transitions, cells * 8}, {counts, chg::COUNT_WORDS * 8}};
    for (const auto& o : outs)
        for (const auto& i : ins) FS_REQUIRE(!overlaps(o.p, o.bytes, i.p, i.bytes), "mosaic_change: an output overlaps an input (%p and %p)", o.p, i.p);
    FS_REQUIRE(aligned(votes_a, 2) && aligned(votes_b, 2), "mosaic_change: votes_a or votes_b is not aligned to 2 bytes");
    FS_REQUIRE(aligned(link, 8) && aligned(counts, 8) && aligned(transitions, 8), "mosaic_change: link, counts or transitions is not aligned to 8 bytes");
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* pairs = reinterpret_cast<unsigned long long*>(transitions);
    change_clear_kernel<<<dim3((unsigned)cdiv((int)cells, THREADS)), THREADS, 0, s>>>(link, sums, pairs, (int)cells);
    FS_HIP(hipGetLastError());
    const dim3 grid((unsigned)cdiv(CW_a, chg::TILE_W), (unsigned)cdiv(CH_a, chg::TILE_H));
    change_classes_kernel<<<grid, THREADS, 0, s>>>(votes_a, CH_a, CW_a, ox_a, oy_a, votes_b, CH_b, CW_b, ox_b, oy_b, K, link, min_votes, min_conf, cls_a, cls_b);
    FS_HIP(hipGetLastError());
    if (tolerance > 0)
        change_codes_kernel<true><<<grid, THREADS, 0, s>>>(cls_a, cls_b, CH_a, CW_a, ox_a, oy_a, CH_b, CW_b, ox_b, oy_b, K, link, tolerance, watch_set, change, pairs, sums);
    else
        change_codes_kernel<false><<<grid, THREADS, 0, s>>>(cls_a, cls_b, CH_a, CW_a, ox_a, oy_a, CH_b, CW_b, ox_b, oy_b, K, link, 0, watch_set, change, pairs, sums);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
