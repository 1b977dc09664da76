// Map-to-map registration and the fold of one mosaic into another (include/floodseg_test.h: merge_view, merge_gate, link_correct,
// mosaic_merge).  OUR DEFINITION -- the reference has nothing like it.  Opt-in: nothing on the shipped routes calls it.
// The rules -- when a link can draw a view or merge, which B canvas pixel lies under an A canvas pixel, which table rows survive, how a
// fit in a window becomes a correction in anchor coordinates, how a rank word is carried into A's ordinals -- are merge_defs.h's on top
// of mosaic_defs.h, ortho_defs.h and refine_defs.h (__host__ __device__, also run on the CPU by the tests).  This file is the launches:
//   merge_view    one launch; a thread per four pixels of a window row.  The link is read at a uniform address (scalar registers).  Per
//                 pixel one word of A, and one word of B where the gather lands inside B's canvas.  Four uint8 planes, a dword per
//                 thread and plane (the window is whole blocks of 16, the planes are aligned to 4).
//   merge_gate    the checks, then refine_ops.hip's gate launch (launch_gate_rows) with valid_a for the block's own window: one wave per
//                 table row, the 256 valid_a bytes under the block's own window and the 256 valid_b bytes under the winner's.
//   link_correct  one wave; the rows go through LDS together, lane 0 runs correct_step.
//   mosaic_merge  a clearing kernel for `counts` (a kernel, not a memset node: DESIGN §3.16), then one workgroup of 256 per 64 x 16 tile
//                 of A as in mosaic_accumulate.  A tile that B's canvas rectangle cannot reach, and every tile under a link that is not
//                 registered, returns before touching a canvas.  A thread owns a column of four rows: per pixel K uint16 reads of B, a
//                 read and a write of A only where B has votes, and with the orthophoto a rank word of B and of A and, where B wins,
//                 12 bytes written.  Every A pixel has one owner: no canvas takes an atomic.  The counts go through an LDS tally and
//                 one 64-bit atomic per workgroup and non-zero cell.
//   merge_patch   patch_kernels.h's two launches (cells, finish), which map_patch shares, on CanvasPatch below: the geometry is
//                 box_geometry's on the link row, a pixel is one word of B under the one gather.
//   link_place    one wave; lane 0 runs place_step.
// Every loop bound follows from the arguments; nothing is allocated, synchronised or read back on the host.
#include "egress_px.h"
#include "kernels.h"
#include "map_checks.h"
#include "merge_defs.h"
#include "patch_kernels.h"

namespace fs {

namespace {

constexpr int GROUP = 4;                  // merge_view: a thread owns four pixels of one row
constexpr int VIEW_TX = 64, VIEW_TY = 4;  // 256 threads: 256 pixels of a row by 4 rows
constexpr int TILE_W = 64, TILE_H = 16, THREADS = 256;
constexpr int TALLY = 4;                  // reached, voted, votes, taken

// ------------------------------------------------------------------ merge_view
__global__ __launch_bounds__(VIEW_TX* VIEW_TY) void merge_view_kernel(const uint32_t* __restrict__ rgba_a, int CW_a, int ox_a, int oy_a,
                                                                       const uint32_t* __restrict__ rgba_b, int CH_b, int CW_b, int ox_b, int oy_b,
                                                                       const long long* __restrict__ link_row, int Y0, int X0, int WH, int WW,
                                                                       uint8_t* __restrict__ cur, uint8_t* __restrict__ view, uint8_t* __restrict__ valid_a,
                                                                       uint8_t* __restrict__ valid_b) {
    int64_t link[mrg::LINK_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < mrg::LINK_WORDS; ++i) link[i] = link_row[i];
    const bool usable = mrg::link_views(link);  // uniform; tested before any product
    int64_t g[6] = {0, 0, 0, 0, 0, 0};
    if (usable) mrg::gather_affine(link, ox_b, oy_b, g);
    const int j = blockIdx.y * VIEW_TY + threadIdx.y, i0 = (blockIdx.x * VIEW_TX + threadIdx.x) * GROUP;
    if (j >= WH || i0 >= WW) return;  // WW is a multiple of 16: a group never straddles the window's edge
    uint32_t c[GROUP], va[GROUP], m[GROUP], vb[GROUP];
#pragma unroll
    for (int i = 0; i < GROUP; ++i) {
        const int X = X0 + i0 + i, Y = Y0 + j;  // inside A's canvas: the launcher tested the window
        int bx = 0, by = 0;
        const bool has_b = usable && mrg::b_pixel(g, X, Y, ox_a, oy_a, CH_b, CW_b, &bx, &by);
        const uint32_t b = has_b ? rgba_b[(size_t)by * CW_b + (size_t)bx] : 0u;
        mrg::view_pixel(rgba_a[(size_t)Y * CW_a + (size_t)X], has_b, b, &c[i], &va[i], &m[i], &vb[i]);
    }
    const size_t at = (size_t)j * WW + i0;
    *reinterpret_cast<uint32_t*>(cur + at) = pack4(c[0], c[1], c[2], c[3]);
    *reinterpret_cast<uint32_t*>(view + at) = pack4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<uint32_t*>(valid_a + at) = pack4(va[0], va[1], va[2], va[3]);
    *reinterpret_cast<uint32_t*>(valid_b + at) = pack4(vb[0], vb[1], vb[2], vb[3]);
}

// ------------------------------------------------------------------ link_correct: lane 0 runs correct_step
__global__ __launch_bounds__(64) void link_correct_kernel(const long long* __restrict__ model, long long* __restrict__ link, int X0, int Y0, int ox_a, int oy_a,
                                                          long long* __restrict__ out) {
    static_assert(mos::MODEL_WORDS == mrg::LINK_WORDS, "the model row and the link are staged by one loop");
    __shared__ int64_t sm[mos::MODEL_WORDS], sl[mrg::LINK_WORDS], so[mrg::OUT_WORDS];
    const int lane = threadIdx.x;
    if (lane < mos::MODEL_WORDS) sm[lane] = model[lane], sl[lane] = link[lane];
    __syncthreads();
    if (lane == 0) {
        int64_t m[mos::MODEL_WORDS], l[mrg::LINK_WORDS], o[mrg::OUT_WORDS];
        for (int i = 0; i < mos::MODEL_WORDS; ++i) m[i] = sm[i], l[i] = sl[i];
        mrg::correct_step(m, l, X0, Y0, ox_a, oy_a, o);
        for (int i = 0; i < mrg::LINK_WORDS; ++i) sl[i] = l[i];
        for (int i = 0; i < mrg::OUT_WORDS; ++i) so[i] = o[i];
    }
    __syncthreads();
    if (lane < mrg::LINK_WORDS) link[lane] = sl[lane];  // unchanged words are written back as they were read
    if (lane < mrg::OUT_WORDS) out[lane] = so[lane];
}

// ------------------------------------------------------------------ mosaic_merge
__global__ __launch_bounds__(64) void merge_counts_clear_kernel(const long long* __restrict__ link, unsigned long long* __restrict__ counts) {
    if ((int)threadIdx.x < mrg::COUNT_WORDS) counts[threadIdx.x] = threadIdx.x == 0 ? (unsigned long long)link[12] : 0ull;
}

template <bool ORTHO>
__global__ __launch_bounds__(THREADS) void mosaic_merge_kernel(uint16_t* __restrict__ votes_a, int CH_a, int CW_a, int ox_a, int oy_a,
                                                               const uint16_t* __restrict__ votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                                                               const long long* __restrict__ link_row, unsigned long long* __restrict__ rank_a,
                                                               uint32_t* __restrict__ rgba_a, const unsigned long long* __restrict__ rank_b,
                                                               const uint32_t* __restrict__ rgba_b, uint32_t ordinal_offset, int mode,
                                                               unsigned long long* counts) {
    __shared__ unsigned long long tally[TALLY];
    const int tid = threadIdx.x, X0 = blockIdx.x * TILE_W, Y0 = blockIdx.y * TILE_H;
    const int X1 = min(X0 + TILE_W, CW_a), Y1 = min(Y0 + TILE_H, CH_a);
    int64_t link[mrg::LINK_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < mrg::LINK_WORDS; ++i) link[i] = link_row[i];
    if (!mrg::link_merges(link)) return;  // uniform, decided here on the device: nothing else is read or written
    int64_t g[6];
    mrg::gather_affine(link, ox_b, oy_b, g);
    if (!mrg::b_reaches(g, X0, Y0, X1, Y1, ox_a, oy_a, CH_b, CW_b)) return;  // uniform
    if (tid < TALLY) tally[tid] = 0ull;
    __syncthreads();
    const int X = X0 + (tid & (TILE_W - 1));
    const size_t plane_a = (size_t)CH_a * CW_a, plane_b = (size_t)CH_b * CW_b;
    unsigned long long reached = 0, voted = 0, added = 0, taken = 0;
    if (X < CW_a) {
        for (int Y = Y0 + tid / TILE_W; Y < Y1; Y += THREADS / TILE_W) {
            int bx, by;
            if (!mrg::b_pixel(g, X, Y, ox_a, oy_a, CH_b, CW_b, &bx, &by)) continue;
            ++reached;
            const size_t cell_a = (size_t)Y * CW_a + X, cell_b = (size_t)by * CW_b + bx;
            bool any = false;
            for (int k = 0; k < K; ++k) {
                const uint32_t more = votes_b[(size_t)k * plane_b + cell_b];
                if (more == 0u) continue;  // a class B never saw there costs two bytes
                uint16_t* p = votes_a + (size_t)k * plane_a + cell_a;
                *p = mos::vote_add(*p, more);
                any = true, added += more;
            }
            voted += any ? 1 : 0;
            if (ORTHO) {
                uint64_t mine;
                if (mrg::shifted_rank(rank_b[cell_b], ordinal_offset, mode, &mine) && orth::replaces(mine, rank_a[cell_a])) {
                    rank_a[cell_a] = mine;
                    rgba_a[cell_a] = rgba_b[cell_b];
                    ++taken;
                }
            }
        }
    }
    if (reached) atomicAdd(&tally[0], reached);
    if (voted) atomicAdd(&tally[1], voted);
    if (added) atomicAdd(&tally[2], added);
    if (taken) atomicAdd(&tally[3], taken);
    __syncthreads();
    if (tid < TALLY && tally[tid]) atomicAdd(counts + 1 + tid, tally[tid]);
}

// ------------------------------------------------------------------ merge_patch: patch_kernels.h's two launches on canvas B
struct LinkBox {  // the patch of b_box under the link: the link row and box_geometry's arguments
    static constexpr int ROW_WORDS = mrg::LINK_WORDS;
    const long long* row;
    int y0, x0, y1, x1, ox_b, oy_b, CH_a, CW_a, ox_a, oy_a, S;
    __device__ int geometry(const int64_t* link, int64_t* geom) const {
        return mrg::box_geometry(link, y0, x0, y1, x1, ox_b, oy_b, CH_a, CW_a, ox_a, oy_a, S, geom);
    }
};
struct CanvasPatch : LinkBox {  // its pixels: the seen words of B's canvas under the one gather
    const uint32_t* rgba_b;
    int CH_b, CW_b;
    __device__ bool luma(const int64_t* link, int64_t X, int64_t Y, uint32_t* l) const {
        int64_t g[6];  // uniform, and the same for every pixel of the cell
        mrg::gather_affine(link, ox_b, oy_b, g);
        return mrg::patch_pixel(g, X, Y, ox_a, oy_a, rgba_b, CH_b, CW_b, l);
    }
};

// ------------------------------------------------------------------ link_place: lane 0 runs place_step
__global__ __launch_bounds__(64) void link_place_kernel(const long long* __restrict__ found_row, const long long* __restrict__ link_row, int max_mean,
                                                        int ratio_permille, int S, long long* __restrict__ cand_row, long long* __restrict__ out_row) {
    if (threadIdx.x != 0) return;
    int64_t found[relo::FOUND_WORDS], link[mrg::LINK_WORDS], cand[mrg::LINK_WORDS], out[mrg::OUT_WORDS];
    for (int i = 0; i < relo::FOUND_WORDS; ++i) found[i] = found_row[i];
    for (int i = 0; i < mrg::LINK_WORDS; ++i) link[i] = link_row[i];
    mrg::place_step(found, link, max_mean, ratio_permille, S, cand, out);
    for (int i = 0; i < mrg::LINK_WORDS; ++i) cand_row[i] = cand[i];
    for (int i = 0; i < mrg::OUT_WORDS; ++i) out_row[i] = out[i];
}

}  // namespace

int launch_merge_view(const uint32_t* rgba_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b,
                      const long long* link, int Y0, int X0, int WH, int WW, uint8_t* cur, uint8_t* view, uint8_t* valid_a, uint8_t* valid_b, hipStream_t s) {
    FS_REQUIRE(rgba_a && rgba_b && link && cur && view && valid_a && valid_b, "merge_view: null pointer");
    FS_TRY(check_canvases("merge_view", CH_a, CW_a, ox_a, oy_a, CH_b, CW_b, ox_b, oy_b));
    FS_REQUIRE(mrg::window_ok(Y0, X0, WH, WW, CH_a, CW_a),
               "merge_view: the window must be whole blocks of 16 (at least one) inside canvas A, got (Y0, X0, WH, WW) = (%d, %d, %d, %d) on %dx%d", Y0, X0, WH, WW,
               CH_a, CW_a);
    FS_REQUIRE(rgba_a != rgba_b, "merge_view: A and B are the same memory");
    FS_REQUIRE(aligned(rgba_a, 4) && aligned(rgba_b, 4), "merge_view: rgba_a or rgba_b is not aligned to 4 bytes");
    FS_REQUIRE(aligned(link, 8), "merge_view: link is not aligned to 8 bytes");
    FS_REQUIRE(aligned(cur, 4) && aligned(view, 4) && aligned(valid_a, 4) && aligned(valid_b, 4), "merge_view: cur, view, valid_a or valid_b is not aligned to 4 bytes");
    const dim3 grid((unsigned)cdiv(WW / GROUP, VIEW_TX), (unsigned)cdiv(WH, VIEW_TY));
    merge_view_kernel<<<grid, dim3(VIEW_TX, VIEW_TY), 0, s>>>(rgba_a, CW_a, ox_a, oy_a, rgba_b, CH_b, CW_b, ox_b, oy_b, link, Y0, X0, WH, WW, cur, view, valid_a,
                                                              valid_b);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_merge_gate(int32_t* table, int blocks, const uint8_t* valid_a, const uint8_t* valid_b, int H, int W, hipStream_t s) {
    FS_REQUIRE(table && valid_a && valid_b, "merge_gate: null pointer");
    FS_TRY(check_sides("merge_gate", "the planes", mrg::MIN_SIDE, H, W));
    FS_REQUIRE(blocks == (H / 16) * (W / 16), "merge_gate: blocks=%d is not the %d rows of a %dx%d plane's table", blocks, (H / 16) * (W / 16), H, W);
    FS_REQUIRE(aligned(table, 4), "merge_gate: table is not aligned to 4 bytes");
    return launch_gate_rows(table, blocks, valid_a, valid_b, H, W, s);  // refine_ops.hip's gate, with the block's own window in valid_a
}

int launch_link_correct(const long long* model, long long* link, int Y0, int X0, int WH, int WW, int ox_a, int oy_a, long long* out, hipStream_t s) {
    FS_REQUIRE(model && link && out, "link_correct: null pointer");
    FS_REQUIRE(mrg::window_ok(Y0, X0, WH, WW, mos::MAX_SIDE, mos::MAX_SIDE),
               "link_correct: the window must be whole blocks of 16 (at least one) inside a canvas of at most %d pixels a side, got (Y0, X0, WH, WW) = (%d, %d, %d, %d)",
               mos::MAX_SIDE, Y0, X0, WH, WW);
    FS_TRY(check_origin("link_correct", "origin A", ox_a, oy_a));
    FS_REQUIRE(aligned(model, 8) && aligned(link, 8) && aligned(out, 8), "link_correct: model, link or out is not aligned to 8 bytes");
    FS_REQUIRE(model != link, "link_correct: model and link are the same memory");
    link_correct_kernel<<<dim3(1), dim3(64), 0, s>>>(model, link, X0, Y0, ox_a, oy_a, out);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_mosaic_merge(uint16_t* votes_a, int CH_a, int CW_a, int ox_a, int oy_a, const uint16_t* votes_b, int CH_b, int CW_b, int ox_b, int oy_b, int K,
                        const long long* link, unsigned long long* rank_a, uint32_t* rgba_a, const unsigned long long* rank_b, const uint32_t* rgba_b,
                        uint32_t ordinal_offset, int mode, long long* counts, hipStream_t s) {
    FS_REQUIRE(votes_a && votes_b && link && counts, "mosaic_merge: null pointer");
    const bool ortho = rank_a || rgba_a || rank_b || rgba_b;
    FS_REQUIRE(!ortho || (rank_a && rgba_a && rank_b && rgba_b), "mosaic_merge: null pointer (an orthophoto takes rank and rgba of both A and B)");
    FS_TRY(check_canvases("mosaic_merge", CH_a, CW_a, ox_a, oy_a, CH_b, CW_b, ox_b, oy_b));
    FS_REQUIRE(K >= 1 && K <= mos::MAX_CLASSES, "mosaic_merge: classes=%d out of range (1..%d)", K, mos::MAX_CLASSES);
    FS_REQUIRE(mode == orth::MODE_CENTRE || mode == orth::MODE_LATEST, "mosaic_merge: mode must be 0 (centre) or 1 (latest), got mode=%d", mode);
    FS_REQUIRE(ordinal_offset != orth::ORDINAL_NONE, "mosaic_merge: ordinal_offset=%u is reserved", ordinal_offset);
    FS_REQUIRE(votes_a != votes_b && (!ortho || (rank_a != rank_b && rgba_a != rgba_b)), "mosaic_merge: A and B are the same memory");
    FS_REQUIRE(aligned(votes_a, 2) && aligned(votes_b, 2), "mosaic_merge: votes_a or votes_b is not aligned to 2 bytes");
    FS_REQUIRE(aligned(link, 8) && aligned(counts, 8), "mosaic_merge: link or counts is not aligned to 8 bytes");
    FS_REQUIRE(!ortho || (aligned(rank_a, 8) && aligned(rank_b, 8)), "mosaic_merge: rank_a or rank_b is not aligned to 8 bytes");
    FS_REQUIRE(!ortho || (aligned(rgba_a, 4) && aligned(rgba_b, 4)), "mosaic_merge: rgba_a or rgba_b is not aligned to 4 bytes");
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(counts);
    merge_counts_clear_kernel<<<dim3(1), dim3(64), 0, s>>>(link, sums);
    const dim3 grid((unsigned)cdiv(CW_a, TILE_W), (unsigned)cdiv(CH_a, TILE_H));
    if (ortho)
        mosaic_merge_kernel<true><<<grid, THREADS, 0, s>>>(votes_a, CH_a, CW_a, ox_a, oy_a, votes_b, CH_b, CW_b, ox_b, oy_b, K, link, rank_a, rgba_a, rank_b, rgba_b,
                                                           ordinal_offset, mode, sums);
    else
        mosaic_merge_kernel<false><<<grid, THREADS, 0, s>>>(votes_a, CH_a, CW_a, ox_a, oy_a, votes_b, CH_b, CW_b, ox_b, oy_b, K, link, rank_a, rgba_a, rank_b,
                                                            rgba_b, ordinal_offset, mode, sums);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_merge_patch(const uint32_t* rgba_b, int CH_b, int CW_b, int ox_b, int oy_b, const long long* link, int CH_a, int CW_a, int ox_a, int oy_a, int S, int y0,
                       int x0, int y1, int x1, uint8_t* tl, uint8_t* tv, long long* geom, hipStream_t s) {
    FS_REQUIRE(rgba_b && link && tl && tv && geom, "merge_patch: null pointer");
    FS_TRY(check_canvases("merge_patch", CH_a, CW_a, ox_a, oy_a, CH_b, CW_b, ox_b, oy_b));
    FS_TRY(check_cell_edge("merge_patch", S));
    FS_TRY(check_has_cell("merge_patch", "canvas A", CH_a, CW_a, S));
    FS_REQUIRE(mrg::box_ok(y0, x0, y1, x1, CH_b, CW_b), "merge_patch: b_box must be a non-empty (y0, x0, y1, x1) inside canvas B, got (%d, %d, %d, %d) on %dx%d", y0,
               x0, y1, x1, CH_b, CW_b);
    FS_REQUIRE(aligned(rgba_b, 4), "merge_patch: rgba_b is not aligned to 4 bytes");
    FS_REQUIRE(aligned(link, 8) && aligned(geom, 8), "merge_patch: link or geom is not aligned to 8 bytes");
    const LinkBox box = {link, y0, x0, y1, x1, ox_b, oy_b, CH_a, CW_a, ox_a, oy_a, S};
    launch_patch_cells(CanvasPatch{box, rgba_b, CH_b, CW_b}, CH_a, CW_a, tl, tv, s);
    FS_HIP(hipGetLastError());
    patch_finish_kernel<<<1, PATCH_THREADS, 0, s>>>(box, tv, geom);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_link_place(const long long* found, const long long* link, int S, int max_mean, int ratio_permille, long long* cand, long long* out, hipStream_t s) {
    FS_REQUIRE(found && link && cand && out, "link_place: null pointer");
    FS_TRY(check_cell_edge("link_place", S));
    FS_REQUIRE(max_mean >= 0 && max_mean <= 255, "link_place: max_mean must be 0..255, got %d", max_mean);
    FS_REQUIRE(ratio_permille >= 1 && ratio_permille <= 1000, "link_place: ratio_permille must be 1..1000, got %d", ratio_permille);
    FS_REQUIRE(aligned(found, 8) && aligned(link, 8) && aligned(cand, 8) && aligned(out, 8), "link_place: found, link, cand or out is not aligned to 8 bytes");
    FS_REQUIRE(cand != link, "link_place: cand is the link itself");
    link_place_kernel<<<1, WAVE, 0, s>>>(found, link, max_mean, ratio_permille, S, cand, out);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
