// The rules of frame-to-map registration (refine_ops.hip; definitions: include/floodseg_test.h, map_view, map_gate and pose_correct;
// DESIGN §3.20).  Plain __host__ __device__ C++ with nothing of HIP in it, in the style of mosaic_defs.h and ortho_defs.h, which it builds
// on and leaves alone: the kernels call these functions, and a host program (tests/test_refine_cpu.py builds
// tests/refine_host_check.cpp) runs them on the CPU.  Everything here is integer arithmetic.
#ifndef FS_REFINE_DEFS_H_
#define FS_REFINE_DEFS_H_

#include "ortho_defs.h"

namespace fs {
namespace refn {

constexpr int OUT_WORDS = 8;     // pose_correct's row: status, usable, inliers, rounds done, fwd[2], fwd[5], 0, 0
constexpr int MIN_SIDE = 16;     // H, W of map_view: one block of the matcher
constexpr int HALF_BLOCK = 8;    // the matcher's 16 x 16 window about a row's src
constexpr int ROW_WORDS = 7;     // a row of the matcher's table
enum Status { REFINE_OK = 0, REFINE_NO_FIT = 2, REFINE_OUT_OF_BOUNDS = 3, REFINE_NOT_TRACKING = 4 };

// ---- THE BOUNDS of the view, beside mosaic_defs.h's.  A usable pose has |to_anchor's linear entry| < 16 ONE = 2^24 and
// |translation| < 2^14 ONE = 2^34 (view_usable tests both BEFORE any product, as pose_votes does for from_anchor).  A frame pixel:
// 0 <= x < 2^14, so |ax| = |(2x + 1) << 19| < 2^35.  One product 2^24 x 2^35 = 2^59, two of them 2^60, + 2^19 under the shift; the
// shifted sum is below 2^40, + the translation 2^34 < 2^41; >> 20 and + ox (|ox| <= 2^14) stays far inside 63 bits.
FS_MOS_HD bool view_usable(const int64_t* pose) {
    return (pose[12] == mos::POSE_OK || pose[12] == mos::POSE_BRIDGED) && mos::linear_within(pose, mos::POSE_LINEAR_LIMIT - 1) &&
           mos::shift_below(pose, mos::POSE_SHIFT_LIMIT);
}
FS_MOS_HD int64_t frame_coord(int x) { return (int64_t)(2 * x + 1) * (mos::ONE / 2); }  // (2x + 1) << 19: the pixel's centre in Q20
// the canvas pixel that holds the centre of frame pixel (x, y) under to_anchor; the caller has tested view_usable
FS_MOS_HD void canvas_pixel(const int64_t* to_anchor, int x, int y, int ox, int oy, int64_t* X, int64_t* Y) {
    const int64_t ax = frame_coord(x), ay = frame_coord(y);
    *X = ((mos::rshr(to_anchor[0] * ax + to_anchor[1] * ay) + to_anchor[2]) >> mos::FRAC) + ox;
    *Y = ((mos::rshr(to_anchor[3] * ax + to_anchor[4] * ay) + to_anchor[5]) >> mos::FRAC) + oy;
}
FS_MOS_HD bool in_canvas(int64_t X, int64_t Y, int CH, int CW) { return X >= 0 && X < CW && Y >= 0 && Y < CH; }
FS_MOS_HD bool seen(uint32_t rgba) { return (rgba >> 24) != 0u; }
// min_age > 0 only: the canvas pixel's owner is at least min_age frames older than this one.  An owner NEWER than the frame (a rank
// word may hold anything) gives a negative difference and is not old enough.
FS_MOS_HD bool old_enough(uint64_t rank, uint32_t ordinal, int min_age) {
    return (int64_t)ordinal - (int64_t)orth::rank_ordinal(rank) >= (int64_t)min_age;
}
// the matcher's luma of an RGB pixel
FS_MOS_HD uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }
FS_MOS_HD uint32_t luma_of(uint32_t rgba) { return luma(rgba & 255u, (rgba >> 8) & 255u, (rgba >> 16) & 255u); }

// ---- the gate.  A row's winner covers [src_x - 8, src_x + 8) x [src_y - 8, src_y + 8) of the view; the row may hold anything (it is
// device memory), so the window is tested against the plane in 64 bits before any byte of it is read.  A void row (src = -16) has
// no window inside any plane, so "not void" needs no test of its own.
FS_MOS_HD bool window_in_plane(const int32_t* row, int H, int W, int64_t* x0, int64_t* y0) {
    *x0 = (int64_t)row[3] - HALF_BLOCK, *y0 = (int64_t)row[4] - HALF_BLOCK;
    return *x0 >= 0 && *y0 >= 0 && *x0 + 2 * HALF_BLOCK <= W && *y0 + 2 * HALF_BLOCK <= H;
}
FS_MOS_HD int32_t void_word(int i) { return i == 0 ? -1 : i < 3 ? 16 : -16; }  // (-1, 16, 16, -16, -16, -16, -16)
FS_MOS_HD void void_row(int32_t* row) {
    for (int i = 0; i < ROW_WORDS; ++i) row[i] = void_word(i);
}
// the serial form (the kernel ballots over the same 256 bytes): true = the row stays as it is
FS_MOS_HD bool gate_keeps(const int32_t* row, const uint8_t* valid, int H, int W) {
    int64_t x0, y0;
    if (!window_in_plane(row, H, W, &x0, &y0)) return false;
    for (int j = 0; j < 2 * HALF_BLOCK; ++j)
        for (int i = 0; i < 2 * HALF_BLOCK; ++i)
            if (valid[(size_t)(y0 + j) * W + (size_t)(x0 + i)] != 1) return false;
    return true;
}

// ---- pose_correct: the fit of the frame against its view folded into the chain.  model: global_motion's row (the forward model maps a
// frame pixel to the view pixel that shows the same ground, and the view was drawn with to_anchor, so the frame's own to_anchor is
// to_anchor o fwd).  Only words 0..11 of the state (the two poses) and words 0..11 and 13 of the pose row are ever written, and only
// with status 0.  Everything read is device memory and is tested before use; the products of compose are inside mosaic_defs.h's
// bounds because pose_in_bounds and pair_in_bounds are tested first, exactly as pose_step does.
// the report row of pose_correct and merge_defs.h's link_correct: status, then the fit's usable rows, inliers, rounds and translation
FS_MOS_HD void fit_report(int status, const int64_t* model, int64_t* out) {
    out[0] = status, out[1] = model[13], out[2] = model[14], out[3] = model[15], out[4] = model[2], out[5] = model[5], out[6] = 0, out[7] = 0;
}
FS_MOS_HD int refine_step(const int64_t* model, int64_t* state, int64_t* pose, int64_t* out, int H, int W, int CH, int CW, int ox, int oy) {
    int status = REFINE_OK;
    bool same = true;
    for (int i = 0; i < 6; ++i) same = same && state[i] == pose[i];
    if ((pose[12] != mos::POSE_OK && pose[12] != mos::POSE_BRIDGED) || state[24] != mos::PHASE_TRACKING || !same) {
        status = REFINE_NOT_TRACKING;
    } else if (model[12] != mos::MODEL_OK || !mos::pair_in_bounds(model, model + 6)) {
        status = REFINE_NO_FIT;
    } else if (!mos::pose_in_bounds(state, state + 6)) {
        status = REFINE_OUT_OF_BOUNDS;
    } else {
        int64_t to_next[6], from_next[6];
        mos::compose(state, model, to_next);
        mos::compose(model + 6, state + 6, from_next);
        if (!mos::pose_in_bounds(to_next, from_next)) {
            status = REFINE_OUT_OF_BOUNDS;
        } else {
            for (int i = 0; i < 6; ++i) state[i] = pose[i] = to_next[i], state[6 + i] = pose[6 + i] = from_next[i];
            pose[13] = mos::frame_clipped(to_next, H, W, CH, CW, ox, oy) ? 1 : 0;
        }
    }
    fit_report(status, model, out);
    return status;
}

}  // namespace refn
}  // namespace fs

#endif  // FS_REFINE_DEFS_H_
