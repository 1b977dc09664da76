// The rules of guide_vectors (motion_ops.hip; definition: include/floodseg_test.h, guide_vectors): the block matcher's
// table guided by global_motion's camera model.  Plain __host__ __device__ C++ with nothing of HIP in it, on mosaic_defs.h: the kernel
// calls these functions, and a host program (tests/test_guide_cpu.py builds tests/guide_host_check.cpp) runs them on the CPU.  Integers
// throughout; the third statement of the same rules is tests/guide_ref.py.
#ifndef FS_GUIDE_DEFS_H_
#define FS_GUIDE_DEFS_H_

#include "mosaic_defs.h"

namespace fs {
namespace guide {

constexpr int BLOCK = 16;        // the matcher's block edge
constexpr int ROW_WORDS = 7;     // (source, w, h, src_x, src_y, dst_x, dst_y)
constexpr int COUNT_WORDS = 8;   // counts[f]
constexpr int MIN_SIDE = 16;     // FH, FW: one block at least
constexpr int64_t MAX_OUTLIER_Q20 = mos::MAX_TOL_Q20;  // outlier_q20 of the call: -1 (off) or 0 .. 64 ONE
constexpr int MAX_PENALTY = 255, MAX_BIAS = 65535;
enum RowClass { ROW_VOID = 0, ROW_FOREIGN = 1, ROW_VECTOR = 2 };
enum Decision { COPY = 0, FILL = 1, REPLACE = 2, DROP = 3, KEEP = 4 };  // KEEP: an outlier the evidence kept; its row is copied
enum Count { C_BLOCKS = 0, C_VOID = 1, C_FILLED = 2, C_OUTLIERS = 3, C_REPLACED = 4, C_DROPPED = 5, C_KEPT = 6, C_FOREIGN = 7 };

// ---- THE BOUNDS.  A model row is device memory and may hold anything, so status and pair_in_bounds are tested BEFORE any product:
//   pair_in_bounds:  |M0|, |M1|, |M3|, |M4| <= 2 ONE = 2^21,  |M2|, |M5| < 2^16 ONE = 2^36
//   a block centre:  cx, cy < 2^14 (FH, FW <= 16384), so CX = cx ONE < 2^34
//   M0 CX + M1 CY:   2^21 x 2^34 = 2^55, two of them 2^56, + 2^19 for the rounding: far inside 63 bits
//   gx:              rshr(...) < 2^36, + M2 < 2^36, - CX < 2^34: |gx| < 2^38;  pdx = rshr(gx): |pdx| < 2^18 + 1
//   the outlier test: dx ONE with |dx| <= 32 is below 2^26, so |dx ONE - gx| < 2^39
//   the evidence:    cost_g <= 65280 + 255 x 64 < 2^17; cost is any int32 and guide_bias <= 65535: their sum is taken in 64 bits
FS_MOS_HD bool pair_guides(const int64_t* M) { return M[12] == mos::MODEL_OK && mos::pair_in_bounds(M, M + 6); }

// the camera's vector at the block centre (cx, cy): (gx, gy) in Q20, (pdx, pdy) rounded to whole pixels.  Only after pair_guides.
FS_MOS_HD void predict(const int64_t* M, int cx, int cy, int64_t* gx, int64_t* gy, int64_t* pdx, int64_t* pdy) {
    const int64_t CX = (int64_t)cx * mos::ONE, CY = (int64_t)cy * mos::ONE;
    *gx = mos::rshr(M[0] * CX + M[1] * CY) + M[2] - CX;
    *gy = mos::rshr(M[3] * CX + M[4] * CY) + M[5] - CY;
    *pdx = mos::rshr(*gx);
    *pdy = mos::rshr(*gy);
}

// the matcher's own candidate rule: |pdx|, |pdy| <= 32 and the 16 x 16 window at (cx - 8 + pdx, cy - 8 + pdy) inside the frame
FS_MOS_HD bool available(int64_t pdx, int64_t pdy, int cx, int cy, int FH, int FW) {
    if (pdx < -mos::MAX_VECTOR || pdx > mos::MAX_VECTOR || pdy < -mos::MAX_VECTOR || pdy > mos::MAX_VECTOR) return false;
    const int64_t x0 = cx - BLOCK / 2 + pdx, y0 = cy - BLOCK / 2 + pdy;
    return x0 >= 0 && y0 >= 0 && x0 + BLOCK <= FW && y0 + BLOCK <= FH;
}

// the class of a row of the block whose centre is (cx, cy): the centre comes from the block's INDEX, a void row has lost its dst.
// The differences are taken in 64 bits: a row is device memory and may hold anything.
FS_MOS_HD int classify(const int32_t* r, int cx, int cy, int* dx, int* dy) {
    *dx = 0, *dy = 0;
    if (r[3] < 0 || r[5] < 0 || r[6] < 0) return ROW_VOID;
    const int64_t ex = (int64_t)r[3] - r[5], ey = (int64_t)r[4] - r[6];
    if (r[5] != cx || r[6] != cy || ex < -mos::MAX_VECTOR || ex > mos::MAX_VECTOR || ey < -mos::MAX_VECTOR || ey > mos::MAX_VECTOR) return ROW_FOREIGN;
    *dx = (int)ex, *dy = (int)ey;
    return ROW_VECTOR;
}

// integer comparisons; equality is not an outlier; outlier_q20 < 0: off
FS_MOS_HD bool is_outlier(int dx, int dy, int64_t gx, int64_t gy, int64_t outlier_q20) {
    return outlier_q20 >= 0 && (mos::iabs64((int64_t)dx * mos::ONE - gx) > outlier_q20 || mos::iabs64((int64_t)dy * mos::ONE - gy) > outlier_q20);
}

// the decision without the frames.  *ask: the row is an outlier with an available guide -- with evidence, evidence_replaces decides
// between REPLACE (what this returns) and KEEP.
FS_MOS_HD int decide(int cls, bool outlier, bool guided, bool avail, int fill_void, bool* ask) {
    *ask = false;
    if (!guided || cls == ROW_FOREIGN) return COPY;
    if (cls == ROW_VOID) return fill_void && avail ? FILL : COPY;
    if (!outlier) return COPY;
    if (!avail) return DROP;  // the camera says its source lay outside the previous frame: whatever it matched is something else
    *ask = true;
    return REPLACE;
}
// cost_g = SAD + penalty (|pdx| + |pdy|) of the guide's window, cost = the matcher's winning cost for the block
FS_MOS_HD int64_t guide_cost(int64_t sad, int penalty, int64_t pdx, int64_t pdy) { return sad + (int64_t)penalty * (mos::iabs64(pdx) + mos::iabs64(pdy)); }
FS_MOS_HD bool evidence_replaces(int64_t cost_g, int32_t cost, int guide_bias) { return cost_g <= (int64_t)cost + guide_bias; }

// word `i` of the output row under a decision; COPY and KEEP take the input's
FS_MOS_HD int32_t void_word(int i) { return i == 0 ? -1 : i < 3 ? BLOCK : -BLOCK; }
FS_MOS_HD int32_t guide_word(int i, int cx, int cy, int64_t pdx, int64_t pdy) {
    return i == 0 ? -1 : i < 3 ? BLOCK : i == 3 ? (int32_t)(cx + pdx) : i == 4 ? (int32_t)(cy + pdy) : i == 5 ? cx : cy;
}
FS_MOS_HD int32_t out_word(int decision, int i, int32_t in, int cx, int cy, int64_t pdx, int64_t pdy) {
    return decision == FILL || decision == REPLACE ? guide_word(i, cx, cy, pdx, pdy) : decision == DROP ? void_word(i) : in;
}

}  // namespace guide
}  // namespace fs

#endif  // FS_GUIDE_DEFS_H_
