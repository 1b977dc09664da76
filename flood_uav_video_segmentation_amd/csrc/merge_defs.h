// The rules of map-to-map registration and of folding one mosaic into another (merge_ops.hip; definitions: include/floodseg_test.h,
// merge_view, merge_gate, link_correct and mosaic_merge).  Plain __host__ __device__ C++ with nothing of HIP in it, on top
// of mosaic_defs.h, ortho_defs.h, refine_defs.h and relocate_defs.h.  A rule that two ops of the family share is written once, in the
// oldest header that needs it (the corners' box; the fit's report row; the cells of a box, the placement gate and its report row), and
// called from here.  The kernels call these functions, and a host program (tests/test_merge_cpu.py builds tests/merge_host_check.cpp)
// runs them on the CPU.  Everything here is integer arithmetic.
#ifndef FS_MERGE_DEFS_H_
#define FS_MERGE_DEFS_H_

#include "relocate_defs.h"

namespace fs {
namespace mrg {

constexpr int LINK_WORDS = 16;   // b_to_a (6), a_to_b (6), status, inliers, usable rows, rounds done
constexpr int OUT_WORDS = 8;     // link_correct's row, pose_correct's layout
constexpr int COUNT_WORDS = 8;   // mosaic_merge's row: link status, reached, voted, votes, taken, 0, 0, 0
constexpr int MIN_SIDE = 16, BLOCK = 16;  // merge_view's window: whole blocks of the matcher
enum LinkStatus { LINK_REGISTERED = 0, LINK_INITIAL = 1, LINK_NO_FIT = 2, LINK_OUT_OF_BOUNDS = 3 };
enum Status { CORRECT_OK = 0, CORRECT_NO_FIT = 2, CORRECT_OUT_OF_BOUNDS = 3, CORRECT_NOT_LINKED = 4 };
constexpr uint64_t ORDINAL_LAST = 0xFFFFFFFEull;  // the largest ordinal a rank word may carry (orth::ORDINAL_NONE is refused everywhere)

// ---- THE LINK.  A link is shaped like a pose row: b_to_a takes to_anchor's place and a_to_b from_anchor's, so mosaic_defs.h's
// pose_in_bounds, touches and compose apply with their own bounds: |linear entry| < 16 ONE = 2^24 both ways, |b_to_a translation| < 2^34,
// |a_to_b translation| < 2^40.  The row is device memory: status and bounds are tested before any product.
FS_MOS_HD bool link_in_bounds(const int64_t* link) { return mos::pose_in_bounds(link, link + 6); }
FS_MOS_HD bool link_views(const int64_t* link) {   // merge_view draws B with it: registered, or a caller's guess
    return (link[12] == LINK_REGISTERED || link[12] == LINK_INITIAL) && link_in_bounds(link);
}
FS_MOS_HD bool link_merges(const int64_t* link) { return link[12] == LINK_REGISTERED && link_in_bounds(link); }  // mosaic_merge: confirmed only

// ---- THE ONE GATHER of the two-canvas ops: the B canvas pixel under the centre of A canvas pixel (X, Y).  By definition it is
//     source_pixel(a_to_b, anchor_coord(X, ox_a), anchor_coord(Y, oy_a)) + (ox_b, oy_b),
// source_pixel yielding pixel indices of B's anchor frame already.  gather_affine folds B's origin into the translation: adding a whole
// number of pixels (a multiple of ONE) under source_pixel's final >> FRAC is the same as adding the pixels after it, so
//     b_pixel(g, ...) with g = gather_affine(link, ox_b, oy_b)
// is that definition bit for bit, and touches(g, tile, ox_a, oy_a, CH_b, CW_b) asks whether B's CANVAS RECTANGLE can reach a tile of A
// exactly as mosaic_accumulate asks it of a frame.
// THE BOUNDS, beside mosaic_defs.h's: |g translation| < 2^40 + 2^14 ONE (|ox_b| <= 2^14) < 2^41.
//   an A canvas pixel:  |X - ox_a| <= 2^15, |anchor_coord| < 2^36;  2^24 x 2^36 = 2^60, two of them 2^61, + 2^19 under the shift;
//                       the shifted sum below 2^42, + 2^41 < 2^43
//   a tile corner:      corner_box's widest caller: its bounds are written for this translation
FS_MOS_HD void gather_affine(const int64_t* link, int ox_b, int oy_b, int64_t* g) {
    for (int i = 0; i < 6; ++i) g[i] = link[6 + i];
    g[2] += (int64_t)ox_b * mos::ONE, g[5] += (int64_t)oy_b * mos::ONE;
}
FS_MOS_HD bool b_pixel(const int64_t* g, int X, int Y, int ox_a, int oy_a, int CH_b, int CW_b, int* bx, int* by) {
    int64_t x, y;
    mos::source_pixel(g, mos::anchor_coord(X, ox_a), mos::anchor_coord(Y, oy_a), &x, &y);
    if (x < 0 || x >= CW_b || y < 0 || y >= CH_b) return false;
    *bx = (int)x, *by = (int)y;
    return true;
}
FS_MOS_HD bool b_reaches(const int64_t* g, int X0, int Y0, int X1, int Y1, int ox_a, int oy_a, int CH_b, int CW_b) {
    return mos::touches(g, X0, Y0, X1, Y1, ox_a, oy_a, CH_b, CW_b);
}

// ---- merge_view: one window pixel.  a: A's word there; b: B's word under it (0 where b_pixel says there is none)
FS_MOS_HD void view_pixel(uint32_t a, bool has_b, uint32_t b, uint32_t* cur, uint32_t* valid_a, uint32_t* view, uint32_t* valid_b) {
    *cur = refn::luma_of(a), *valid_a = refn::seen(a) ? 1u : 0u;
    const bool ok = has_b && refn::seen(b);
    *view = ok ? refn::luma_of(b) : 0u, *valid_b = ok ? 1u : 0u;
}
FS_MOS_HD bool window_ok(int Y0, int X0, int WH, int WW, int CH, int CW) {
    return WH >= MIN_SIDE && WW >= MIN_SIDE && WH % BLOCK == 0 && WW % BLOCK == 0 && Y0 >= 0 && X0 >= 0 && (int64_t)Y0 + WH <= CH && (int64_t)X0 + WW <= CW;
}

// ---- merge_gate: row `index` of the table of a H x W plane is the block at (16 (index % wb), 16 (index / wb)).  The block's own window
// comes from the INDEX, not from the row's dst words (the row is device memory); the winner's window is refine_defs.h's gate_keeps.
FS_MOS_HD bool own_window_valid(int index, const uint8_t* valid_a, int H, int W) {
    const int wb = W / BLOCK, x0 = (index % wb) * BLOCK, y0 = (index / wb) * BLOCK;  // inside the plane for every index below (H / 16) wb
    for (int j = 0; j < BLOCK; ++j)
        for (int i = 0; i < BLOCK; ++i)
            if (valid_a[(size_t)(y0 + j) * W + (size_t)(x0 + i)] != 1) return false;
    return true;
}
FS_MOS_HD bool merge_gate_keeps(const int32_t* row, int index, const uint8_t* valid_a, const uint8_t* valid_b, int H, int W) {
    return own_window_valid(index, valid_a, H, W) && refn::gate_keeps(row, valid_b, H, W);
}

// ---- link_correct.  model: global_motion's row fitted on (cur, view) with frame_size = mask_size = the window: its forward model F takes
// a window pixel (continuous, window-local) to the place in `view` that shows the same ground.  A window-local coordinate plus
// s = (X0 - ox_a, Y0 - oy_a) is A's anchor coordinate, so in anchor coordinates the correction is C(P) = F(P - s) + s:
//     C.linear = F.linear,   C.translation = F.t + s ONE - F.linear s,
// and the inverse model is conjugated the same way.  view was drawn with a_to_b, so a_to_b <- a_to_b o C and b_to_a <- C^-1 o b_to_a.
// THE BOUNDS: pair_in_bounds(F): |linear| <= 2^21, |t| < 2^36; |s| <= 2^15 whole pixels: F.linear s: 2^21 x 2^15 = 2^36, two of them
// 2^37, + 2^36 + 2^35 < 2^38 -- exact, no rounding (whole pixels).  The conjugated pair is then held to pair_in_bounds AGAIN (a fit of
// a few pixels at |s| <= 2^15 with |linear - 1| <= 1/4 moves at most 2^14 pixels; 2^16 is the net), so that compose keeps
// mosaic_defs.h's derivation: compose(a_to_b, C): 2^24 x 2^36 = 2^60, two 2^61, + 2^40 < 2^62; compose(C^-1, b_to_a): 2^21 x 2^34.
FS_MOS_HD void conjugate(const int64_t* f, int64_t sx, int64_t sy, int64_t* c) {
    c[0] = f[0], c[1] = f[1], c[3] = f[3], c[4] = f[4];
    c[2] = f[2] + sx * mos::ONE - (f[0] * sx + f[1] * sy);
    c[5] = f[5] + sy * mos::ONE - (f[3] * sx + f[4] * sy);
}
FS_MOS_HD int correct_step(const int64_t* model, int64_t* link, int X0, int Y0, int ox_a, int oy_a, int64_t* out) {
    int status = CORRECT_OK;
    int64_t c[6], ci[6], a_to_b[6], b_to_a[6];
    if (link[12] != LINK_REGISTERED && link[12] != LINK_INITIAL) {
        status = CORRECT_NOT_LINKED;
    } else if (model[12] != mos::MODEL_OK || !mos::pair_in_bounds(model, model + 6)) {
        status = CORRECT_NO_FIT;
    } else {
        const int64_t sx = (int64_t)X0 - ox_a, sy = (int64_t)Y0 - oy_a;
        conjugate(model, sx, sy, c);
        conjugate(model + 6, sx, sy, ci);
        if (!mos::pair_in_bounds(c, ci)) {
            status = CORRECT_NO_FIT;
        } else if (!link_in_bounds(link)) {
            status = CORRECT_OUT_OF_BOUNDS;
        } else {
            mos::compose(link + 6, c, a_to_b);
            mos::compose(ci, link, b_to_a);
            if (!mos::pose_in_bounds(b_to_a, a_to_b)) {
                status = CORRECT_OUT_OF_BOUNDS;
            } else {
                for (int i = 0; i < 6; ++i) link[i] = b_to_a[i], link[6 + i] = a_to_b[i];
                link[12] = LINK_REGISTERED, link[13] = model[14], link[14] = model[13], link[15] = model[15];
            }
        }
    }
    refn::fit_report(status, model, out);
    return status;
}

// ---- mosaic_merge, the orthophoto: B's rank word carried into A's ordinals.  false: the pixel takes nothing (B is empty there, or the
// shifted ordinal would leave 0..0xFFFFFFFE).  centre mode keeps the high word (the squared distance from the optical axis does not
// depend on which mosaic the frame was in); latest mode rebuilds it from the shifted ordinal, as frame_rank does.
FS_MOS_HD bool shifted_rank(uint64_t rank_b, uint32_t ordinal_offset, int mode, uint64_t* rank) {
    if (rank_b == orth::RANK_EMPTY) return false;
    const uint64_t ord = (uint64_t)orth::rank_ordinal(rank_b) + ordinal_offset;  // below 2^33
    if (ord > ORDINAL_LAST) return false;
    const uint64_t high = mode == orth::MODE_LATEST ? 0xFFFFFFFFull - ord : rank_b >> 32;
    *rank = (high << 32) | ord;
    return true;
}

// ---- merge_patch: B drawn into A's canvas cells under the link, for map_locate.  The geometry is map_patch's -- guard, box, reach test,
// cells -- on the corners of b_box = [x0, x1) x [y0, y1) (B canvas pixels) under b_to_a.  Status: map_patch's codes -- 1: the link is
// neither registered nor initial (nothing to place); 2: the link is out of the pose bounds, or the box lands more than 2^15 pixels from
// A's anchor; 3 and 4: relo::box_cells'.  A corner is |x - ox_b| <= 2^15 and b_to_a's translation below 2^34: inside corner_box's bounds.
// Status 2's second test then holds every pixel of the patch within 2^15 + 16 of A's anchor (the widening to whole cells adds at most
// S - 1 <= 15), so |anchor_coord| < 2^36 + 2^25 and b_pixel's products stay below 2^24 x 2^37 = 2^61, two of them 2^62.
constexpr int64_t PATCH_REACH = (int64_t)1 << 15;
FS_MOS_HD bool box_ok(int y0, int x0, int y1, int x1, int CH_b, int CW_b) { return y0 >= 0 && x0 >= 0 && y0 < y1 && x0 < x1 && y1 <= CH_b && x1 <= CW_b; }
FS_MOS_HD int box_geometry(const int64_t* link, int y0, int x0, int y1, int x1, int ox_b, int oy_b, int CH_a, int CW_a, int ox_a, int oy_a, int S, int64_t* geom) {
    for (int i = 0; i < relo::GEOM_WORDS; ++i) geom[i] = 0;
    if (link[12] != LINK_REGISTERED && link[12] != LINK_INITIAL) return (int)(geom[0] = relo::PATCH_NOT_LOST);
    if (!link_in_bounds(link)) return (int)(geom[0] = relo::PATCH_OUT_OF_BOUNDS);
    int64_t lo_x, hi_x, lo_y, hi_y;
    mos::corner_box(link, (int64_t)x0 - ox_b, (int64_t)y0 - oy_b, (int64_t)x1 - ox_b, (int64_t)y1 - oy_b, &lo_x, &hi_x, &lo_y, &hi_y);
    const int64_t sx = (int64_t)ox_a * mos::ONE, sy = (int64_t)oy_a * mos::ONE;
    const int64_t X0 = relo::floor_pixel(lo_x + sx), Y0 = relo::floor_pixel(lo_y + sy), X1 = relo::ceil_pixel(hi_x + sx), Y1 = relo::ceil_pixel(hi_y + sy);
    if (X0 - ox_a < -PATCH_REACH || X1 - ox_a > PATCH_REACH || Y0 - oy_a < -PATCH_REACH || Y1 - oy_a > PATCH_REACH) return (int)(geom[0] = relo::PATCH_OUT_OF_BOUNDS);
    return relo::box_cells(X0, Y0, X1, Y1, CH_a, CW_a, S, geom);
}
// one pixel of a cell: the luma of the seen B pixel under A canvas pixel (X, Y) -- which may lie outside A's canvas --, or false
FS_MOS_HD bool patch_pixel(const int64_t* g, int64_t X, int64_t Y, int ox_a, int oy_a, const uint32_t* rgba_b, int CH_b, int CW_b, uint32_t* luma) {
    int bx, by;
    if (!b_pixel(g, (int)X, (int)Y, ox_a, oy_a, CH_b, CW_b, &bx, &by)) return false;
    const uint32_t px = rgba_b[(size_t)by * CW_b + (size_t)bx];
    if (!refn::seen(px)) return false;
    *luma = refn::luma_of(px);
    return true;
}

// ---- link_place: map_locate's placement as a CANDIDATE link.  relo::placement_gate with the link as the holder, so relocate_step's
// acceptance and codes: 1 the link is neither registered nor initial; 2 no eligible placement; 6 an unusable found row or a link out of
// bounds; 3 the mean; 4 the uniqueness; 7 the moved link leaves the pose bounds; 0 placed: both affines moved by (S u*, S v*) A canvas
// pixels, status 1 (initial: the fine rounds have yet to confirm it), words 13..15 zero.  With any other code the candidate is the link
// as it was.  out = relocate_commit's row: the code, then relo::placement_report's words.
FS_MOS_HD int place_step(const int64_t* found, const int64_t* link, int max_mean, int ratio_permille, int S, int64_t* cand, int64_t* out) {
    int64_t to[6], from[6];
    const int decision = relo::placement_gate(found, link[12] == LINK_REGISTERED || link[12] == LINK_INITIAL, link, max_mean, ratio_permille, S, to, from);
    for (int i = 0; i < LINK_WORDS; ++i) cand[i] = link[i];
    if (decision == relo::RELOCATED) {
        for (int i = 0; i < 6; ++i) cand[i] = to[i], cand[6 + i] = from[i];
        cand[12] = LINK_INITIAL, cand[13] = 0, cand[14] = 0, cand[15] = 0;
    }
    out[0] = decision;
    relo::placement_report(found, S, out);
    return decision;
}

}  // namespace mrg
}  // namespace fs

#endif  // FS_MERGE_DEFS_H_
