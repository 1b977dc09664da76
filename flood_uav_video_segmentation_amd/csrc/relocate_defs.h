// The rules of relocalisation against the orthophoto (relocate_ops.hip; definitions: include/floodseg_test.h, map_coarse, map_patch,
// map_locate, pose_relocate and relocate_commit).  Plain __host__ __device__ C++ with nothing of HIP in it, on top of
// refine_defs.h, which it leaves alone: the kernels call these functions, and a host program (tests/test_relocate_cpu.py builds
// tests/relocate_host_check.cpp) runs them on the CPU.  Everything here is integer arithmetic.
#ifndef FS_RELOCATE_DEFS_H_
#define FS_RELOCATE_DEFS_H_

#include "refine_defs.h"

namespace fs {
namespace relo {

constexpr int GEOM_WORDS = 8;             // map_patch's row: status, pu0, pv0, tw, th, nt, 0, 0
constexpr int FOUND_WORDS = 16;           // map_locate's row, see write_found
constexpr int OUT_WORDS = 8;              // relocate_commit's row
constexpr int MAX_PATCH_CELLS = 65536;    // tw th of a patch, and the bytes of tl and of tv
constexpr int DECISION_WORD = 28;         // the CANDIDATE state's first spare word holds pose_relocate's decision; never copied into the state
constexpr int COMMIT_STATE_WORDS = 28, COMMIT_POSE_WORDS = 14;  // what relocate_commit copies: the spare words and the pair's counts stay
constexpr int MAX_EXCLUDE = 64;
enum PatchStatus { PATCH_OK = 0, PATCH_NOT_LOST = 1, PATCH_OUT_OF_BOUNDS = 2, PATCH_CELLS = 3, PATCH_WIDER_THAN_MAP = 4 };
enum FoundStatus { FOUND = 0, FOUND_NONE = 1, FOUND_BAD_GEOM = 2 };
enum Status {
    RELOCATED = 0, NOT_ATTEMPTED = 1, NO_PLACEMENT = 2, REJECTED_MEAN = 3, REJECTED_UNIQUENESS = 4, FINE_FAILED = 5, PATCH_REFUSED = 6, OUT_OF_BOUNDS = 7
};

FS_MOS_HD bool scale_ok(int S) { return S == 4 || S == 8 || S == 16; }
FS_MOS_HD int scale_shift(int S) { return S == 4 ? 2 : S == 8 ? 3 : 4; }

// ---- map_coarse: one cell from its S x S canvas words.  The sum of S^2 <= 256 lumas is at most 255 * 256 < 2^16.
FS_MOS_HD uint32_t cell_mean(uint32_t sum, int S) { return (sum + (uint32_t)(S * S) / 2u) / (uint32_t)(S * S); }
FS_MOS_HD void coarse_cell(const uint32_t* rgba, int CW, int cx, int cy, int S, uint8_t* luma, uint8_t* valid) {
    uint32_t sum = 0;
    bool all = true;
    for (int b = 0; b < S; ++b)
        for (int a = 0; a < S; ++a) {
            const uint32_t px = rgba[(size_t)(cy * S + b) * CW + (size_t)(cx * S + a)];
            all = all && refn::seen(px);
            sum += refn::luma_of(px);
        }
    *luma = all ? (uint8_t)cell_mean(sum, S) : (uint8_t)0, *valid = all ? 1 : 0;
}

// ---- THE CELLS OF A BOX, for map_patch and merge_defs.h's merge_patch alike.  A box of canvas coordinates in Q20 (mos::corner_box's,
// the origin added) covers the canvas pixels [floor(lo), ceil(hi)); box_cells widens them outwards to whole cells of the canvas's own
// grid and writes geom[1..4] = (pu0, pv0, tw, th), or refuses: 3 no cell (a box without a pixel has none) or more than 65536, 4 more
// cells than the coarse canvas.  A box edge is below 2^43 (mosaic_defs.h), so a canvas pixel is below 2^23 in magnitude and a cell below
// 2^21: tw th < 2^44 in 64 bits.
FS_MOS_HD int64_t floor_pixel(int64_t q20) { return q20 >> mos::FRAC; }  // arithmetic shifts: floor and ceiling for negative values too
FS_MOS_HD int64_t ceil_pixel(int64_t q20) { return (q20 + mos::ONE - 1) >> mos::FRAC; }
FS_MOS_HD int64_t floor_cell(int64_t px, int S) { return px >> scale_shift(S); }
FS_MOS_HD int box_cells(int64_t X0, int64_t Y0, int64_t X1, int64_t Y1, int CH, int CW, int S, int64_t* geom) {
    const int64_t pu0 = floor_cell(X0, S), pu1 = floor_cell(X1 + S - 1, S), pv0 = floor_cell(Y0, S), pv1 = floor_cell(Y1 + S - 1, S);
    const int64_t tw = X1 > X0 ? pu1 - pu0 : 0, th = Y1 > Y0 ? pv1 - pv0 : 0;
    if (tw < 1 || th < 1 || tw * th > MAX_PATCH_CELLS) return (int)(geom[0] = PATCH_CELLS);
    if (tw > CW / S || th > CH / S) return (int)(geom[0] = PATCH_WIDER_THAN_MAP);
    geom[1] = pu0, geom[2] = pv0, geom[3] = tw, geom[4] = th;
    return PATCH_OK;
}

// ---- map_patch: the geometry of the patch from the LOST state's poses: guard, box, cells.  Everything read from the state is tested
// before any product: the phase is PHASE_LOST; pose_in_bounds holds to_anchor's translation below 2^34, and the corners are 0..W <= 2^14:
// inside corner_box's bounds.
//   AFTER the patch is known to be no wider than the coarse canvas (tw S <= CW <= 2^14): corner (0, 0) lies at to_anchor's translation,
//   below 2^14 pixels from the anchor, and every pixel of the patch within 2^14 + 2 S of it, so |X - ox| < 2^15 + 32 and
//   |anchor_coord| < 2^36 + 2^25: source_pixel's products stay below 2^24 x 2^37 = 2^61, two of them 2^62, inside 63 bits, and the
//   rounded sum below 2^42, + 2^40.
FS_MOS_HD int patch_geometry(const int64_t* state, int H, int W, int CH, int CW, int ox, int oy, int S, int64_t* geom) {
    for (int i = 0; i < GEOM_WORDS; ++i) geom[i] = 0;
    if (state[24] != mos::PHASE_LOST) return (int)(geom[0] = PATCH_NOT_LOST);
    if (!mos::pose_in_bounds(state, state + 6)) return (int)(geom[0] = PATCH_OUT_OF_BOUNDS);
    int64_t lo_x, hi_x, lo_y, hi_y;
    mos::corner_box(state, 0, 0, W, H, &lo_x, &hi_x, &lo_y, &hi_y);
    const int64_t sx = (int64_t)ox * mos::ONE, sy = (int64_t)oy * mos::ONE;
    return box_cells(floor_pixel(lo_x + sx), floor_pixel(lo_y + sy), ceil_pixel(hi_x + sx), ceil_pixel(hi_y + sy), CH, CW, S, geom);
}
// the frame pixel under canvas pixel (X, Y) of the patch, or false; the caller holds a PATCH_OK geometry of this state
FS_MOS_HD bool patch_source(const int64_t* state, int64_t X, int64_t Y, int ox, int oy, int H, int W, int* x, int* y) {
    int64_t sx, sy;
    mos::source_pixel(state + 6, mos::anchor_coord((int)X, ox), mos::anchor_coord((int)Y, oy), &sx, &sy);
    if (sx < 0 || sx >= W || sy < 0 || sy >= H) return false;
    *x = (int)sx, *y = (int)sy;
    return true;
}

// ---- map_locate.  geom is device memory: tested before any product or index.  |pu0|, |pv0| < 2^18 by construction; 2^20 is the net.
FS_MOS_HD bool geom_ok(const int64_t* geom, int ch, int cw) {  // ch, cw: the coarse canvas in cells
    if (geom[0] != PATCH_OK) return false;
    if (geom[3] < 1 || geom[4] < 1 || geom[3] > cw || geom[4] > ch) return false;
    if (geom[3] * geom[4] > MAX_PATCH_CELLS) return false;  // both at most 2^12: the product is below 2^24
    if (geom[5] < 0 || geom[5] > geom[3] * geom[4]) return false;
    return mos::iabs64(geom[1]) < ((int64_t)1 << 20) && mos::iabs64(geom[2]) < ((int64_t)1 << 20);
}
struct Score {
    int64_t sad, n, u, v;  // u, v: the SHIFT in cells; n == 0: no placement
};
FS_MOS_HD Score no_score() { return Score{0, 0, 0, 0}; }
// n >= 1 and 1000 n >= permille nt: n, nt <= 2^16, the products stay below 2^26
FS_MOS_HD bool eligible(int64_t n, int64_t nt, int permille) { return n >= 1 && 1000 * n >= (int64_t)permille * nt; }
// the total order of eligible placements: the smaller mean sad_a / n_a < sad_b / n_b as sad_a n_b < sad_b n_a (sad < 2^24, n <= 2^16: the
// products stay below 2^40); then the larger n, the smaller v, the smaller u.  A score with n == 0 loses to every other.
FS_MOS_HD bool better(const Score& a, const Score& b) {
    if (a.n == 0 || b.n == 0) return a.n != 0;
    const int64_t l = a.sad * b.n, r = b.sad * a.n;
    if (l != r) return l < r;
    if (a.n != b.n) return a.n > b.n;
    if (a.v != b.v) return a.v < b.v;
    return a.u < b.u;
}
FS_MOS_HD bool outside(const Score& s, const Score& best, int exclude) {  // max(|u - u*|, |v - v*|) > exclude
    return mos::iabs64(s.u - best.u) > exclude || mos::iabs64(s.v - best.v) > exclude;
}
// one placement: the patch's origin at canvas cell (au, av), which the caller keeps inside [0, cw - tw] x [0, ch - th]
FS_MOS_HD void score_placement(const uint8_t* cl, const uint8_t* cv, int cw, const uint8_t* tl, const uint8_t* tv, int tw, int th, int au, int av, int64_t* sad,
                               int64_t* n) {
    int64_t s = 0, k = 0;
    for (int j = 0; j < th; ++j)
        for (int i = 0; i < tw; ++i) {
            const size_t c = (size_t)(av + j) * cw + (size_t)(au + i), t = (size_t)j * tw + i;
            if (cv[c] == 1 && tv[t] == 1) k += 1, s += cl[c] > tl[t] ? cl[c] - tl[t] : tl[t] - cl[c];
        }
    *sad = s, *n = k;
}
FS_MOS_HD void write_found(int64_t* found, int status, const Score& best, const Score& second, int64_t placements, int64_t eligible_count, int64_t nt) {
    for (int i = 0; i < FOUND_WORDS; ++i) found[i] = 0;
    found[0] = status, found[10] = placements, found[11] = eligible_count, found[12] = nt;
    if (status != FOUND) return;
    found[1] = best.u, found[2] = best.v, found[3] = best.sad, found[4] = best.n;
    if (second.n == 0) return;
    found[5] = 1, found[6] = second.u, found[7] = second.v, found[8] = second.sad, found[9] = second.n;
}

// ---- THE PLACEMENT GATE of pose_relocate and merge_defs.h's link_place.  holder: the twelve words (to, from) that the placement would
// move -- the state's two poses, or a link; attempted: the holder's own guard (a lost chain; a registered or initial link).  found and
// the holder are device memory: a holder out of pose_in_bounds, a count outside 1..2^16, a sum outside 0..255 n, or a shift beyond
// 2^14 cells makes the row unusable (PATCH_REFUSED).  Each test comes before the products it protects:
//   the mean test      sad* <= max_mean n*:                          255 x 2^16 < 2^24
//   the uniqueness     1000 sad* n2 <= ratio_permille sad2 n*:       1000 x 2^24 x 2^16 < 2^50
//   the translation    S u ONE: 16 x 2^14 x 2^20 = 2^38;  from[0] S u: 2^24 x 2^18 = 2^42, two of them 2^43, + 2^40
// Returns the decision; with RELOCATED (to, from) is the holder moved by (S u*, S v*) canvas pixels, and is for no use otherwise.
FS_MOS_HD bool pair_ok(int64_t sad, int64_t n) { return n >= 1 && n <= MAX_PATCH_CELLS && sad >= 0 && sad <= 255 * n; }
FS_MOS_HD void translate(const int64_t* to, const int64_t* from, int64_t dx, int64_t dy, int64_t* to_out, int64_t* from_out) {  // by whole canvas pixels: exact
    for (int i = 0; i < 6; ++i) to_out[i] = to[i], from_out[i] = from[i];
    to_out[2] += dx * mos::ONE, to_out[5] += dy * mos::ONE;
    from_out[2] -= from[0] * dx + from[1] * dy, from_out[5] -= from[3] * dx + from[4] * dy;
}
FS_MOS_HD int placement_gate(const int64_t* found, bool attempted, const int64_t* holder, int max_mean, int ratio_permille, int S, int64_t* to, int64_t* from) {
    for (int i = 0; i < 6; ++i) to[i] = 0, from[i] = 0;
    if (!attempted) return NOT_ATTEMPTED;
    if (found[0] == FOUND_NONE) return NO_PLACEMENT;
    if (found[0] != FOUND || !mos::pose_in_bounds(holder, holder + 6) || !pair_ok(found[3], found[4]) || mos::iabs64(found[1]) > mos::MAX_SIDE ||
        mos::iabs64(found[2]) > mos::MAX_SIDE || (found[5] != 0 && !pair_ok(found[8], found[9])))
        return PATCH_REFUSED;
    if (found[3] > (int64_t)max_mean * found[4]) return REJECTED_MEAN;
    if (found[5] != 0 && 1000 * found[3] * found[9] > (int64_t)ratio_permille * found[8] * found[4]) return REJECTED_UNIQUENESS;
    translate(holder, holder + 6, (int64_t)S * found[1], (int64_t)S * found[2], to, from);
    return mos::pose_in_bounds(to, from) ? RELOCATED : OUT_OF_BOUNDS;
}
// the report row of relocate_commit and link_place, words 1..7: (S u*, S v*, sad*, n*, sad2, n2, eligible placements), zero where found
// does not hold them.  S u: below 2^18.
FS_MOS_HD void placement_report(const int64_t* found, int S, int64_t* out) {
    for (int i = 1; i < OUT_WORDS; ++i) out[i] = 0;
    if (found[0] == FOUND && mos::iabs64(found[1]) <= mos::MAX_SIDE && mos::iabs64(found[2]) <= mos::MAX_SIDE) {
        out[1] = (int64_t)S * found[1], out[2] = (int64_t)S * found[2], out[3] = found[3], out[4] = found[4];
        if (found[5] != 0) out[5] = found[8], out[6] = found[9];
    }
    if (found[0] == FOUND || found[0] == FOUND_NONE) out[7] = found[11];
}

// ---- pose_relocate: the gate on a lost chain -- a chain that is not lost has nothing to do, and no caller needs to know that beforehand.
FS_MOS_HD int relocate_step(const int64_t* found, const int64_t* state, int64_t* cand_state, int64_t* cand_pose, int max_mean, int ratio_permille, int H, int W,
                            int CH, int CW, int ox, int oy, int S) {
    int64_t to[6], from[6];
    const int decision = placement_gate(found, state[24] == mos::PHASE_LOST, state, max_mean, ratio_permille, S, to, from);
    for (int i = 0; i < mos::STATE_WORDS; ++i) cand_state[i] = state[i];
    if (decision == RELOCATED) {
        for (int i = 0; i < 6; ++i) cand_state[i] = cand_pose[i] = to[i], cand_state[6 + i] = cand_pose[6 + i] = from[i];
        mos::identity(cand_state + 12), mos::identity(cand_state + 18);  // a bridge after relocation never replays the motion from before the break
        cand_state[24] = mos::PHASE_TRACKING, cand_state[27] = 0;
        cand_pose[12] = mos::POSE_OK, cand_pose[13] = mos::frame_clipped(to, H, W, CH, CW, ox, oy) ? 1 : 0;
    } else {
        mos::identity(cand_pose), mos::identity(cand_pose + 6);
        cand_pose[12] = mos::POSE_LOST, cand_pose[13] = 0;
    }
    cand_pose[14] = 0, cand_pose[15] = 0;
    cand_state[DECISION_WORD] = decision;
    return decision;
}

// ---- relocate_commit: the candidate replaces the state and the pose row iff pose_relocate accepted the placement AND pose_correct then
// reported 0 on the candidate.  Words 0..27 of the state and 0..13 of the row are copied: the state's spare words and the row's pair
// counts stay.  Nothing else is ever written, so a chain that is not relocated stays lost exactly as it was.
FS_MOS_HD int commit_step(const int64_t* cand_state, const int64_t* cand_pose, const int64_t* correct_out, int64_t* state, int64_t* pose, const int64_t* found, int S,
                          int64_t* out) {
    const int64_t d = cand_state[DECISION_WORD];
    int status = d == RELOCATED ? RELOCATED : (d >= NOT_ATTEMPTED && d <= OUT_OF_BOUNDS && d != FINE_FAILED) ? (int)d : PATCH_REFUSED;
    if (status == RELOCATED && (correct_out[0] != refn::REFINE_OK || cand_state[24] != mos::PHASE_TRACKING || cand_pose[12] != mos::POSE_OK ||
                                !mos::pose_in_bounds(cand_state, cand_state + 6)))
        status = FINE_FAILED;
    if (status == RELOCATED) {
        for (int i = 0; i < COMMIT_STATE_WORDS; ++i) state[i] = cand_state[i];
        for (int i = 0; i < COMMIT_POSE_WORDS; ++i) pose[i] = cand_pose[i];
    }
    out[0] = status;
    placement_report(found, S, out);
    return status;
}

}  // namespace relo
}  // namespace fs

#endif  // FS_RELOCATE_DEFS_H_
