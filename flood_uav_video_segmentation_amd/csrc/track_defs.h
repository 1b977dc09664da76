// Integer helpers of the region tracking (track_ops.hip; definitions: include/floodseg_test.h, region_links / region_tracks; DESIGN
// §3.12).  Plain __host__ __device__ C++ with nothing of HIP in it: the kernels call these functions, and a host program
// (tests/test_tracks_cpu.py builds tests/tracks_host_check.cpp) runs serial versions of the four passes through the very same
// functions, so the packing, the probe sequence and the continue / born rule are checked on the CPU.
#ifndef FS_TRACK_DEFS_H_
#define FS_TRACK_DEFS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define FS_TRK_HD __host__ __device__ __forceinline__
#else
#define FS_TRK_HD inline
#endif

namespace fs {
namespace trk {

constexpr int MIN_PAIRS = 16, MAX_PAIRS = 1 << 20;  // the pair table's size: a power of two in this range
constexpr int TRACK_BLOCK = 1024;                   // rows per piece of the track-id scan: one workgroup

// ---- the pair table.  A slot's key is 0 while it is empty; the key of the pair (row a of the frame before, row b of this frame),
// 0 <= a, b < 65536, has bit 63 set, so no pair packs to 0.
FS_TRK_HD uint64_t pack_key(int a, int b) { return (1ull << 63) | ((uint64_t)(uint32_t)a << 32) | (uint64_t)(uint32_t)b; }
FS_TRK_HD int key_a(uint64_t key) { return (int)((key >> 32) & 0x7fffffffu); }
FS_TRK_HD int key_b(uint64_t key) { return (int)(key & 0xffffffffu); }

// The probe sequence of a key: probe i = 0 .. max_pairs - 1 visits slot (hash + i) mod max_pairs, so the max_pairs probes visit EVERY
// slot once.  An insertion therefore fails only when all max_pairs slots hold other keys: whether a frame pair overflows depends on
// its number of distinct pairs alone, never on the hash or on the order of the insertions.
FS_TRK_HD uint32_t probe_slot(uint64_t key, uint32_t i, uint32_t max_pairs) {
    const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32);
    return (h + i) & (max_pairs - 1u);
}

// ---- the best partner of a row: the maximum of overlap << 32 | (0xffffffff - other row) over the row's pairs.  The larger overlap
// wins, and among equal overlaps the inverted row makes the LOWEST other row the maximum.  0 = no pair (a stored pair has overlap >= 1).
FS_TRK_HD uint64_t pack_best(uint32_t overlap, int other) { return ((uint64_t)overlap << 32) | (uint64_t)(0xffffffffu - (uint32_t)other); }
FS_TRK_HD int best_overlap(uint64_t best) { return (int)(best >> 32); }  // < 2^31: a frame has fewer pixels
FS_TRK_HD int best_row(uint64_t best) { return (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu)); }

// One (row, overlap) link from a packed best value: the partner, unless the frame pair overflowed or its best overlap is below
// min_overlap (>= 1, so the empty value 0 never qualifies): then (-1, 0).
FS_TRK_HD void unpack_link(uint64_t best, int min_overlap, bool overflow, int* row, int* overlap) {
    const bool ok = !overflow && best_overlap(best) >= min_overlap;
    *row = ok ? best_row(best) : -1;
    *overlap = ok ? best_overlap(best) : 0;
}

// ---- the continue / born rule.  Row b of this frame, whose back link names row a of the frame before, CONTINUES a's track exactly
// when a >= 0, a's forward link names b, and a has a track (prev_id >= 0; -1: no track table for the frame before, or no such row).
FS_TRK_HD bool continues(int a, int fwd_of_a, int b, long long prev_id) { return a >= 0 && fwd_of_a == b && prev_id >= 0; }

// ---- the flag word of a frame pair (column 1 of link_counts): bit 0 = the pair table overflowed, bit 1 = the pair is a scene cut
// (region_links_mc alone sets it).  Either bit means "no links at all" for the pair.
constexpr unsigned FLAG_OVERFLOW = 1u, FLAG_CUT = 2u;
FS_TRK_HD long long link_flags(unsigned word) { return (long long)(word & (FLAG_OVERFLOW | FLAG_CUT)); }
FS_TRK_HD unsigned cut_flag(const int32_t* stats_row) { return stats_row[2] != 0 ? FLAG_CUT : 0u; }  // a row of block_match_modes' stats

// ---- motion compensation of the links (region_links_mc): pixel -> block, table row -> vector, vector -> shift in mask pixels,
// shift -> source pixel.  P = the mask's extent along one axis (H or W), F = the decoded frame's (frame_h or frame_w).
// Ranges the launcher guarantees: 1 <= P, 16 <= F, P * P' < 2^31 - 1 and F * F' < 2^31 for the two axes, P <= MC_MAX_SCALE * F.
// Then (2p + 1) F < 2^32 * 2^27 and 2 |v| P + F < 2^43 fit 64 bits with room, and a scaled shift is at most
// (2 * 1024 * 31 F + F) / (2 F) = 31744 in magnitude: it fits the 16 bits it is packed into.
constexpr int MC_BLOCK = 16;         // the matcher's block
constexpr int MC_MAX_VECTOR = 1024;  // a row with a larger |vx| or |vy| counts as void (the matcher's search is +-32)
constexpr int MC_MAX_SCALE = 31;     // the mask may be at most this many times the frame along an axis
constexpr int MC_VECTOR_INTS = 7;    // ints per table row: (-1, 16, 16, src_x, src_y, dst_x, dst_y)

// the block coordinate of mask coordinate p's centre: ((2p + 1) F) // (2P) // 16.  May be >= F // 16: the remainder strip.
FS_TRK_HD int mc_block(int p, int P, int F) {
    const uint64_t num = (uint64_t)(2 * (int64_t)p + 1) * (uint64_t)F, den = 2 * (uint64_t)P;
    const uint64_t pos = (num >> 32) ? num / den : (uint64_t)((uint32_t)num / (uint32_t)den);  // den < 2^32; the short division where it does
    return (int)(pos / MC_BLOCK);
}

// a vector component scaled to mask pixels: nearest, ties away from zero.  |v| <= MC_MAX_VECTOR.
FS_TRK_HD int mc_scale(int v, int P, int F) {
    const uint64_t mag = (2 * (uint64_t)(v < 0 ? -v : v) * (uint64_t)P + (uint64_t)F) / (2 * (uint64_t)F);
    return v < 0 ? -(int)mag : (int)mag;
}

// two shifts in one dword: sy in the high half, sx in the low half, both as 16-bit two's complement.  0 = no shift.
FS_TRK_HD uint32_t mc_pack_shift(int sy, int sx) { return ((uint32_t)(uint16_t)(int16_t)sy << 16) | (uint32_t)(uint16_t)(int16_t)sx; }
FS_TRK_HD int mc_shift_y(uint32_t s) { return (int)(int16_t)(uint16_t)(s >> 16); }
FS_TRK_HD int mc_shift_x(uint32_t s) { return (int)(int16_t)(uint16_t)(s & 0xffffu); }

// The packed shift of one table row, for ANY seven ints: a void row (dst_x or dst_y < 0), or one whose vector (source minus
// destination, in 64 bits: no two ints overflow them) passes MC_MAX_VECTOR, gives 0.
FS_TRK_HD uint32_t mc_row_shift(const int32_t* r, int H, int W, int FH, int FW) {
    if (r[5] < 0 || r[6] < 0) return 0u;
    const int64_t vx = (int64_t)r[3] - (int64_t)r[5], vy = (int64_t)r[4] - (int64_t)r[6];
    if (vx > MC_MAX_VECTOR || vx < -MC_MAX_VECTOR || vy > MC_MAX_VECTOR || vy < -MC_MAX_VECTOR) return 0u;
    return mc_pack_shift(mc_scale((int)vy, H, FH), mc_scale((int)vx, W, FW));
}

// The source of pixel (y, x) under a packed shift; false when it lies outside the H x W mask, and then *ys, *xs must not be used.
// The sums are taken in 64 bits: a mask of one column may have y near 2^31.
FS_TRK_HD bool mc_source(int y, int x, uint32_t shift, int H, int W, int* ys, int* xs) {
    const int64_t sy = (int64_t)y + mc_shift_y(shift), sx = (int64_t)x + mc_shift_x(shift);
    *ys = (int)sy;
    *xs = (int)sx;
    return sy >= 0 && sy < H && sx >= 0 && sx < W;
}

}  // namespace trk
}  // namespace fs
#endif  // FS_TRACK_DEFS_H_
