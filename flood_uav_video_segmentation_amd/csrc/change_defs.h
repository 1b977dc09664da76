// The rules of the flood-extent change map between two registered mosaics (change_ops.hip; definition: include/floodseg_test.h,
// mosaic_change).  Plain __host__ __device__ C++ with nothing of HIP in it, on top of merge_defs.h: which B canvas pixel lies
// under an A canvas pixel, and whether B's canvas can reach a tile, are mrg::gather_affine, mrg::b_pixel and mrg::b_reaches, called, not
// restated; a vote's confidence is mos::vote_confidence.  The kernels call these functions, and a host program (tests/test_change_cpu.py
// builds tests/change_host_check.cpp) runs them on the CPU.  Everything here is integer arithmetic.
#ifndef FS_CHANGE_DEFS_H_
#define FS_CHANGE_DEFS_H_

#include "merge_defs.h"

namespace fs {
namespace chg {

constexpr int COUNT_WORDS = 8;     // link status, reached, comparable, same, explained, changed-other, gained, lost
constexpr int CODES = 6;           // the values of the change plane
constexpr int MAX_TOLERANCE = 8;   // r, in canvas pixels
constexpr int MAX_VOTES = 65535, MAX_CONF = 255;
constexpr uint8_t NONE = 255;      // a class plane's "not decided" (and "no B pixel")
enum Code { NOT_COMPARABLE = 0, SAME = 1, EXPLAINED = 2, CHANGED_OTHER = 3, GAINED = 4, LOST = 5 };
constexpr int TILE_W = 64, TILE_H = 16;                       // §3.18's tile of A: what one workgroup owns
constexpr int APRON_W = TILE_W + 2 * MAX_TOLERANCE;           // 80: the widest staged row
constexpr int APRON_H = TILE_H + 2 * MAX_TOLERANCE;           // 32
constexpr int HEAD = COUNT_WORDS;                             // the tally: the counts' cells, then transitions [2][K][K]

// THE BOUNDS, beside merge_defs.h's (the gather's are there, and this header adds no product to them):
//   a pixel's total:      K <= 32 counts of at most 65535: below 2^21;  vote_confidence's 255 most + total / 2: below 2^24 + 2^20.  uint32.
//   a workgroup's tally:  a tile has TILE_W TILE_H = 1024 pixels and a pixel adds at most 1 to a cell: every cell <= 1024.  uint32.
//   counts, transitions:  a canvas has at most 2^14 x 2^14 = 2^28 pixels, so every cell <= 2^28.  int64 in memory.
//   the tally's size:     HEAD + 2 K^2 <= 8 + 2048 dwords.
FS_MOS_HD int tally_cells(int K) { return HEAD + 2 * K * K; }
FS_MOS_HD int transition_cell(int changed, int ca, int cb, int K) { return (changed * K + ca) * K + cb; }

FS_MOS_HD bool thresholds_ok(int min_votes, int min_conf, int tolerance) {
    return min_votes >= 1 && min_votes <= MAX_VOTES && min_conf >= 0 && min_conf <= MAX_CONF && tolerance >= 0 && tolerance <= MAX_TOLERANCE;
}
FS_MOS_HD bool watch_ok(uint32_t watch_set, int K) { return K >= mos::MAX_CLASSES || (watch_set >> K) == 0u; }  // no bit at or above K

// ---- THE DECIDED CLASS of one canvas pixel: mosaic_resolve's winner -- the class with strictly more votes than every class before it, so
// the lowest id on a tie -- if the pixel's total reaches min_votes and the winner's share reaches min_conf; NONE otherwise.  The K
// counts are taken one by one, in the order k = 0, 1, ...; min_votes >= 1, so a pixel without a vote is never decided.
struct Winner {
    uint32_t total, most, id;
};
FS_MOS_HD Winner no_votes() { return Winner{0u, 0u, (uint32_t)NONE}; }
FS_MOS_HD void take_votes(Winner* w, int k, uint32_t votes) {
    w->total += votes;
    if (votes > w->most) w->most = votes, w->id = (uint32_t)k;
}
FS_MOS_HD uint8_t decided_class(const Winner& w, int min_votes, int min_conf) {
    return w.total >= (uint32_t)min_votes && (int)mos::vote_confidence(w.most, w.total) >= min_conf ? (uint8_t)w.id : NONE;
}

// ---- THE WINDOW SETS.  A class plane's pixel as a set: bit cls, or nothing where the class is NONE or the pixel lies outside the canvas
// (the apron is clipped at the canvas edge).  win(X, Y) is the OR over [X - r, X + r] x [Y - r, Y + r], done separably: a staged plane of
// (rows + 2 r) x (cols + 2 r) sets with row stride `stride` whose cell (0, 0) is canvas pixel (X0 - r, Y0 - r); row_or at (x, y) of the
// staged plane is the OR over its cells x .. x + 2 r of row y, and column_or over rows y .. y + 2 r of the row_or results.
FS_MOS_HD uint32_t class_bit(uint8_t cls) { return cls == NONE ? 0u : 1u << (cls & 31); }
FS_MOS_HD uint32_t staged_bit(const uint8_t* plane, int CH, int CW, int X, int Y) {
    return X < 0 || X >= CW || Y < 0 || Y >= CH ? 0u : class_bit(plane[(size_t)Y * CW + (size_t)X]);
}
FS_MOS_HD uint32_t span_or(const uint32_t* first, int step, int r) {  // the OR of the 2 r + 1 cells first[0], first[step], ...
    uint32_t s = 0u;
    for (int d = 0; d <= 2 * r; ++d) s |= first[d * step];
    return s;
}

// ---- THE CHANGE CODE of one pixel: ca, cb its decided classes in A and in B, win_a, win_b its window sets
FS_MOS_HD int change_code(uint8_t ca, uint8_t cb, uint32_t win_a, uint32_t win_b, uint32_t watch_set) {
    if (ca == NONE || cb == NONE) return NOT_COMPARABLE;
    if (ca == cb) return SAME;
    if (((win_b >> ca) & 1u) != 0u && ((win_a >> cb) & 1u) != 0u) return EXPLAINED;  // both: B holds A's class within r, and A holds B's
    const bool watch_a = ((watch_set >> ca) & 1u) != 0u, watch_b = ((watch_set >> cb) & 1u) != 0u;
    if (watch_a == watch_b) return CHANGED_OTHER;
    return watch_b ? GAINED : LOST;
}

}  // namespace chg
}  // namespace fs

#endif  // FS_CHANGE_DEFS_H_
