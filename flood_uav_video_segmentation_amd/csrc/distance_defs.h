// The integer rules of the exact distance transform and its tabulation (distance_ops.hip; definitions: include/floodseg_test.h,
// mask_distance and region_proximity).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these
// functions, and a host program (tests/test_distance_cpu.py builds tests/distance_host_check.cpp) runs them on the CPU.
#ifndef FS_DISTANCE_DEFS_H_
#define FS_DISTANCE_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_DST_HD __host__ __device__ __forceinline__
#else
#define FS_DST_HD inline
#endif

namespace fs {
namespace dst {

constexpr int MAX_SIDE = 32768;            // H, W <= 2^15: d2 <= 2 * 32767^2 < 2^31
constexpr int MAX_DIST = 32767;            // R and the thresholds
constexpr int MAX_THRESHOLDS = 8;          // B
constexpr int MAX_SOURCE_CLASSES = 32;     // the bits of source_set / target_set
constexpr uint32_t NONE = 0xFFFFFFFFu;     // FS_DIST_NONE
constexpr int CHUNK = 64;                  // rows of a column chunk: one bit per row in a 64-bit word
constexpr uint32_t NO_ROW = 0xFFFFu;       // the workspace's "no source in this column" (rows are <= 32767)

// ---- is the mask id m a member of the class set (ids >= 32 never are)
FS_DST_HD bool in_set(int m, uint32_t set) { return m < MAX_SOURCE_CLASSES && ((set >> m) & 1u) != 0u; }

// ---- a candidate: the squared distance in the high dword, the source's raster index in the low one, so that the smaller 64-bit word
// is the nearer source and, at equal distance, the one with the smaller raster index.  NO_CANDIDATE is larger than every candidate.
constexpr uint64_t NO_CANDIDATE = ~(uint64_t)0;
FS_DST_HD uint64_t pack(uint32_t d2, uint32_t raster) { return ((uint64_t)d2 << 32) | raster; }
FS_DST_HD uint32_t cand_d2(uint64_t c) { return (uint32_t)(c >> 32); }
FS_DST_HD uint32_t cand_raster(uint64_t c) { return (uint32_t)c; }
FS_DST_HD uint64_t better(uint64_t a, uint64_t b) { return b < a ? b : a; }

// the candidate that column xs offers to a pixel of row y at horizontal offset dx: its nearest source sits in row `row` (NO_ROW: none)
FS_DST_HD uint64_t candidate(int y, int dx, uint32_t row, int xs, int W) {
    if (row == NO_ROW) return NO_CANDIDATE;
    const int64_t g = (int64_t)y - (int64_t)row;
    return pack((uint32_t)((int64_t)dx * dx + g * g), (uint32_t)((int64_t)row * W + xs));
}

// ---- the stop rule of the row scan: every candidate at horizontal offset d costs at least d * d, so offsets from the first d with
// d * d > best on cannot improve (value, raster index); without the nearest plane a tie is no improvement either.  R > 0: no value
// above R * R is ever reported, so d stops at R.
FS_DST_HD bool scan_stops(int d, uint64_t best, int R, bool want_nearest) {
    const uint64_t dd = (uint64_t)d * (uint64_t)d, b = cand_d2(best);
    if (R > 0 && d > R) return true;
    return want_nearest ? dd > b : dd >= b;
}

// one pixel of a row: `rows` = the row's W entries of the column pass (NO_ROW or the row of the column's nearest source).  Returns the
// best candidate over the whole row, NO_CANDIDATE without one inside the scan.
template <class Rows>
FS_DST_HD uint64_t scan_row(const Rows& rows, int y, int x, int W, int H, int R, bool want_nearest) {
    uint32_t r0 = rows[x];
    if (r0 != NO_ROW && r0 >= (uint32_t)H) r0 = (uint32_t)(H - 1);  // a workspace value is clamped before use
    uint64_t best = candidate(y, 0, r0, x, W);
    for (int d = 1; d < W; ++d) {
        if (scan_stops(d, best, R, want_nearest)) break;
        const int xl = x - d, xr = x + d;
        if (xl < 0 && xr >= W) break;
        if (xl >= 0) {
            uint32_t r = rows[xl];
            if (r != NO_ROW && r >= (uint32_t)H) r = (uint32_t)(H - 1);
            best = better(best, candidate(y, d, r, xl, W));
        }
        if (xr < W) {
            uint32_t r = rows[xr];
            if (r != NO_ROW && r >= (uint32_t)H) r = (uint32_t)(H - 1);
            best = better(best, candidate(y, d, r, xr, W));
        }
    }
    return best;
}

// what a pixel reports for its best candidate: *d2 and *nearest (NONE and -1 without a candidate, or beyond R > 0)
FS_DST_HD void report(uint64_t best, int R, uint32_t* d2, int32_t* nearest) {
    const uint32_t v = cand_d2(best);
    const bool none = best == NO_CANDIDATE || (R > 0 && v > (uint32_t)R * (uint32_t)R);
    *d2 = none ? NONE : v;
    *nearest = none ? -1 : (int32_t)cand_raster(best);
}

// ---- the column pass: of the nearest source above or in row y (`up`, -1: none) and the nearest below (`down`, -1: none), the nearer
// one; the UPPER one on a tie (the smaller raster index within the column)
FS_DST_HD int column_pick(int y, int up, int down) {
    if (up < 0) return down;
    if (down < 0) return up;
    return (y - up) <= (down - y) ? up : down;
}

// bit r of `bits` = row y0 + r of the column is a source.  The nearest source row at or above / at or below row y0 + r inside the
// chunk, -1 without one.
FS_DST_HD int chunk_up(uint64_t bits, int y0, int r) {
    const uint64_t at = bits & (~(uint64_t)0 >> (63 - r));
    if (!at) return -1;
    return y0 + 63 - __builtin_clzll(at);
}
FS_DST_HD int chunk_down(uint64_t bits, int y0, int r) {
    const uint64_t at = bits >> r;
    if (!at) return -1;
    return y0 + r + __builtin_ctzll(at);
}

// ---- region_proximity: the first threshold a squared distance is within (B: none), thresholds ascending
FS_DST_HD int first_bin(uint32_t d2, const int* thresholds, int B) {
    int b = 0;
    while (b < B && (uint64_t)d2 > (uint64_t)thresholds[b] * (uint64_t)thresholds[b]) ++b;
    return b;
}

}  // namespace dst
}  // namespace fs
#endif  // FS_DISTANCE_DEFS_H_
