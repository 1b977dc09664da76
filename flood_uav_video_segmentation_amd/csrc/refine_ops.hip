// Frame-to-map registration (include/floodseg_test.h: map_view, map_gate, pose_correct).  OUR DEFINITION -- the reference
// has nothing like it.  Opt-in: nothing on the shipped routes calls it.  The rules -- when a pose can draw a view, which canvas pixel a
// frame pixel sees, when that pixel counts, which table rows survive, how the fit is folded into the chain -- are refine_defs.h's on top
// of mosaic_defs.h and ortho_defs.h (__host__ __device__, also run on the CPU by the tests); the image is ingest_src.h's resized1, the one
// ortho_accumulate samples.  This file is the launches:
//   map_view      one frame per call; a thread per four pixels of a row.  The pose row is read at a uniform address (scalar registers).
//                 Per pixel: the frame's own luma, the canvas pixel under to_anchor, one rgba word (and one rank word with an age gate)
//                 where that pixel is inside the canvas.  Three uint8 planes, written whole: dwords where W % 4 == 0 and the planes are
//                 aligned, bytes otherwise.
//   map_gate      one wave per table row; the 256 valid bytes under the winner's window, four per lane, one ballot; a row that does not
//                 survive is overwritten with the void row by lanes 0..6.  The same kernel with OWN set is merge_ops.hip's merge_gate.
// The argument checks that the map family shares are map_checks.h's.
//   pose_correct  one wave; the rows go through LDS together, lane 0 runs refine_step.
// Every loop bound follows from the arguments; nothing is allocated, synchronised or read back on the host; no atomics.  Compile with
// -ffp-contract=off (csrc/Makefile): the resize must round as ingest's, egress's and ortho's do.
#include "egress_px.h"
#include "ingest_src.h"
#include "kernels.h"
#include "map_checks.h"
#include "refine_defs.h"

namespace fs {

namespace {

constexpr int GROUP = 4;                 // map_view: a thread owns four pixels of one row
constexpr int VIEW_TX = 64, VIEW_TY = 4; // 256 threads: 256 pixels of a row by 4 rows

// ------------------------------------------------------------------ map_view
template <bool YUV, int MODE, bool WIDE>
__global__ __launch_bounds__(VIEW_TX* VIEW_TY) void map_view_kernel(IngestSrc s, const long long* __restrict__ pose_row, uint32_t ordinal, int H, int W, int CH,
                                                                     int CW, int ox, int oy, float sy, float sx,
                                                                     const unsigned long long* __restrict__ rank, const uint32_t* __restrict__ rgba,
                                                                     int min_age, uint8_t* __restrict__ cur, uint8_t* __restrict__ view,
                                                                     uint8_t* __restrict__ valid) {
    int64_t pose[mos::POSE_WORDS];  // the same address in every thread: scalar loads
#pragma unroll
    for (int i = 0; i < mos::POSE_WORDS; ++i) pose[i] = pose_row[i];
    const bool usable = refn::view_usable(pose);  // uniform; tested before any product
    const int y = blockIdx.y * VIEW_TY + threadIdx.y, x0 = (blockIdx.x * VIEW_TX + threadIdx.x) * GROUP;
    if (y >= H || x0 >= W) return;
    uint32_t c[GROUP], m[GROUP], ok[GROUP];
#pragma unroll
    for (int i = 0; i < GROUP; ++i) {
        const int x = x0 + i;
        c[i] = m[i] = ok[i] = 0u;
        if (x >= W) continue;  // the byte route's last group; never on the wide route
        float v[3];
        resized1<YUV, MODE>(s, y, x, sy, sx, v);
        c[i] = refn::luma((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]);
        if (!usable) continue;
        int64_t X, Y;
        refn::canvas_pixel(pose, x, y, ox, oy, &X, &Y);
        if (!refn::in_canvas(X, Y, CH, CW)) continue;
        const size_t cell = (size_t)Y * CW + (size_t)X;
        const uint32_t px = rgba[cell];
        if (!refn::seen(px)) continue;
        if (min_age > 0 && !refn::old_enough(rank[cell], ordinal, min_age)) continue;  // rank is read with an age gate only
        m[i] = refn::luma_of(px), ok[i] = 1u;
    }
    const size_t at = (size_t)y * W + x0;
    if (WIDE) {
        *reinterpret_cast<uint32_t*>(cur + at) = pack4(c[0], c[1], c[2], c[3]);
        *reinterpret_cast<uint32_t*>(view + at) = pack4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<uint32_t*>(valid + at) = pack4(ok[0], ok[1], ok[2], ok[3]);
    } else {
#pragma unroll
        for (int i = 0; i < GROUP; ++i)
            if (x0 + i < W) cur[at + i] = (uint8_t)c[i], view[at + i] = (uint8_t)m[i], valid[at + i] = (uint8_t)ok[i];
    }
}

template <bool YUV, int MODE>
void view_width(bool wide, dim3 grid, hipStream_t st, const IngestSrc& s, const long long* pose, uint32_t ordinal, int H, int W, int CH, int CW, int ox, int oy,
                float sy, float sx, const unsigned long long* rank, const uint32_t* rgba, int min_age, uint8_t* cur, uint8_t* view, uint8_t* valid) {
    const dim3 block(VIEW_TX, VIEW_TY);
    if (wide)
        map_view_kernel<YUV, MODE, true><<<grid, block, 0, st>>>(s, pose, ordinal, H, W, CH, CW, ox, oy, sy, sx, rank, rgba, min_age, cur, view, valid);
    else
        map_view_kernel<YUV, MODE, false><<<grid, block, 0, st>>>(s, pose, ordinal, H, W, CH, CW, ox, oy, sy, sx, rank, rgba, min_age, cur, view, valid);
}

template <bool YUV>
void view_mode(const IngestSrc& s, const long long* pose, uint32_t ordinal, int H, int W, int CH, int CW, int ox, int oy, const unsigned long long* rank,
               const uint32_t* rgba, int min_age, uint8_t* cur, uint8_t* view, uint8_t* valid, bool wide, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(cdiv(W, GROUP), VIEW_TX), (unsigned)cdiv(H, VIEW_TY));
    const float sy = resize_scale(s.H, H, 0), sx = resize_scale(s.W, W, 0);  // as egress_ops.hip and ortho_ops.hip take them
    if (s.H == H && s.W == W)
        view_width<YUV, 2>(wide, grid, st, s, pose, ordinal, H, W, CH, CW, ox, oy, sy, sx, rank, rgba, min_age, cur, view, valid);
    else if (s.W == W)
        view_width<YUV, 1>(wide, grid, st, s, pose, ordinal, H, W, CH, CW, ox, oy, sy, sx, rank, rgba, min_age, cur, view, valid);
    else
        view_width<YUV, 0>(wide, grid, st, s, pose, ordinal, H, W, CH, CW, ox, oy, sy, sx, rank, rgba, min_age, cur, view, valid);
}

// ------------------------------------------------------------------ map_gate and merge_gate: one wave per row.  OWN (merge_gate): the
// block's own 16 x 16 window, at (16 (index % wb), 16 (index / wb)) and so inside the plane, must be valid in `own` as well.
__device__ __forceinline__ bool window_valid(const uint8_t* plane, int64_t x0, int64_t y0, int W, int lane) {
    const uint8_t* p = plane + (size_t)(y0 + (lane >> 2)) * W + (size_t)(x0 + (lane & 3) * 4);  // lane: row lane / 4, four bytes at column (lane % 4) * 4
    return p[0] == 1 && p[1] == 1 && p[2] == 1 && p[3] == 1;
}
template <bool OWN>
__global__ __launch_bounds__(64) void gate_kernel(int32_t* __restrict__ table, const uint8_t* __restrict__ own, const uint8_t* __restrict__ valid, int H, int W) {
    const int index = blockIdx.x, lane = threadIdx.x;
    int32_t* row = table + (size_t)index * refn::ROW_WORDS;
    int32_t r[refn::ROW_WORDS];  // a uniform address: every lane holds the row before any lane writes it
#pragma unroll
    for (int i = 0; i < refn::ROW_WORDS; ++i) r[i] = row[i];
    int64_t x0, y0;
    bool ok = refn::window_in_plane(r, H, W, &x0, &y0);  // uniform: in 64 bits, before any byte of a plane is read
    if (ok) {
        ok = window_valid(valid, x0, y0, W, lane);
        constexpr int BLOCK = 2 * refn::HALF_BLOCK;
        if (OWN) ok = ok && window_valid(own, (index % (W / BLOCK)) * BLOCK, (index / (W / BLOCK)) * BLOCK, W, lane);
    }
    const bool keep = __ballot(ok) == ~0ull;
    if (!keep && lane < refn::ROW_WORDS) row[lane] = refn::void_word(lane);
}

// ------------------------------------------------------------------ pose_correct: lane 0 runs refine_step
__global__ __launch_bounds__(64) void pose_correct_kernel(const long long* __restrict__ model, long long* __restrict__ state, long long* __restrict__ pose, int H,
                                                          int W, int CH, int CW, int ox, int oy, long long* __restrict__ out) {
    __shared__ int64_t sm[mos::MODEL_WORDS], st[mos::STATE_WORDS], sp[mos::POSE_WORDS], so[refn::OUT_WORDS];
    const int lane = threadIdx.x;
    if (lane < mos::MODEL_WORDS) sm[lane] = model[lane], sp[lane] = pose[lane];
    if (lane < mos::STATE_WORDS) st[lane] = state[lane];
    __syncthreads();
    if (lane == 0) {
        int64_t m[mos::MODEL_WORDS], s[mos::STATE_WORDS], p[mos::POSE_WORDS], o[refn::OUT_WORDS];
        for (int i = 0; i < mos::MODEL_WORDS; ++i) m[i] = sm[i], p[i] = sp[i];
        for (int i = 0; i < mos::STATE_WORDS; ++i) s[i] = st[i];
        refn::refine_step(m, s, p, o, H, W, CH, CW, ox, oy);
        for (int i = 0; i < mos::POSE_WORDS; ++i) sp[i] = p[i];
        for (int i = 0; i < 12; ++i) st[i] = s[i];
        for (int i = 0; i < refn::OUT_WORDS; ++i) so[i] = o[i];
    }
    __syncthreads();
    if (lane < mos::POSE_WORDS) pose[lane] = sp[lane];
    if (lane < 12) state[lane] = st[lane];  // the two poses; last_fwd, last_inv, the phase and the counters are never written
    if (lane < refn::OUT_WORDS) out[lane] = so[lane];
}

}  // namespace

int launch_map_view(const uint8_t* frame, const uint8_t* u, const uint8_t* v, int format, int matrix, int full_range, int FH, int FW, const long long* pose,
                    uint32_t ordinal, int H, int W, int CH, int CW, int ox, int oy, const unsigned long long* rank, const uint32_t* rgba, int min_age,
                    uint8_t* cur, uint8_t* view, uint8_t* valid, hipStream_t s) {
    FS_REQUIRE(frame && pose && rank && rgba && cur && view && valid, "map_view: null pointer");
    FS_TRY(check_frame_source("map_view", u, v, format, matrix, full_range, FH, FW));
    FS_TRY(check_mask_on_canvas("map_view", refn::MIN_SIDE, H, W, CH, CW, ox, oy));
    FS_REQUIRE(ordinal != orth::ORDINAL_NONE, "map_view: ordinal=%u is reserved", ordinal);
    FS_REQUIRE(min_age >= 0, "map_view: min_age=%d is negative", min_age);
    FS_REQUIRE(aligned(pose, 8), "map_view: pose is not aligned to 8 bytes");
    FS_REQUIRE(aligned(rank, 8), "map_view: rank is not aligned to 8 bytes");
    FS_REQUIRE(aligned(rgba, 4), "map_view: rgba is not aligned to 4 bytes");
    const IngestSrc src = make_ingest_src(frame, u, v, format, matrix, full_range, FH, FW);
    const bool wide = W % GROUP == 0 && aligned(cur, 4) && aligned(view, 4) && aligned(valid, 4);
    if (format == 0)
        view_mode<false>(src, pose, ordinal, H, W, CH, CW, ox, oy, rank, rgba, min_age, cur, view, valid, wide, s);
    else
        view_mode<true>(src, pose, ordinal, H, W, CH, CW, ox, oy, rank, rgba, min_age, cur, view, valid, wide, s);
    FS_HIP(hipGetLastError());
    return 0;
}

// the launch behind map_gate (own == nullptr) and merge_ops.hip's merge_gate; the arguments are the caller's to check
int launch_gate_rows(int32_t* table, int blocks, const uint8_t* own, const uint8_t* valid, int H, int W, hipStream_t s) {
    if (own)
        gate_kernel<true><<<dim3((unsigned)blocks), dim3(64), 0, s>>>(table, own, valid, H, W);
    else
        gate_kernel<false><<<dim3((unsigned)blocks), dim3(64), 0, s>>>(table, own, valid, H, W);
    FS_HIP(hipGetLastError());
    return 0;
}

int launch_map_gate(int32_t* table, int blocks, const uint8_t* valid, int H, int W, hipStream_t s) {
    FS_REQUIRE(table && valid, "map_gate: null pointer");
    FS_TRY(check_sides("map_gate", "the plane", refn::MIN_SIDE, H, W));
    FS_REQUIRE(blocks == (H / 16) * (W / 16), "map_gate: blocks=%d is not the %d rows of a %dx%d plane's table", blocks, (H / 16) * (W / 16), H, W);
    FS_REQUIRE(aligned(table, 4), "map_gate: table is not aligned to 4 bytes");
    return launch_gate_rows(table, blocks, nullptr, valid, H, W, s);
}

int launch_pose_correct(const long long* model, long long* state, long long* pose, int H, int W, int CH, int CW, int ox, int oy, long long* out, hipStream_t s) {
    FS_REQUIRE(model && state && pose && out, "pose_correct: null pointer");
    FS_TRY(check_mask_on_canvas("pose_correct", 1, H, W, CH, CW, ox, oy));
    FS_REQUIRE(aligned(model, 8) && aligned(state, 8) && aligned(pose, 8) && aligned(out, 8), "pose_correct: model, state, pose or out is not aligned to 8 bytes");
    pose_correct_kernel<<<dim3(1), dim3(64), 0, s>>>(model, state, pose, H, W, CH, CW, ox, oy, out);
    FS_HIP(hipGetLastError());
    return 0;
}

}  // namespace fs
